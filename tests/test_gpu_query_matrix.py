"""GPU: every query and off-step kernel instantiation at its slot capacity, with a ledger of the cells that ran.

Inst<> instantiates k_observe_grid, k_navigate, k_partner, k_render, k_reset_where and k_restore_where per kernel instance and agent
count, k_action_effects per action scheme as well.  The other tests reach them through hand-picked lists that leave instantiations
out, and in none of them is the last slot lane of an instance live.  This module walks 24 cells (instance x agents x scheme), each
the same small world - crowded_6x5, natural D = 6, 8 envs - on the instance that max_dyn = 64 | 128 | 255 selects, D at its top.
Four checkpoints of one oracle trajectory at natural D, and with two or more agents one more with despawn / respawn on, are shown to
the device through set_state in two forms: widened (slots 0..5 in use) and relocated (`matrix_common.relocate_slots`: the batch's
highest alive slot in slot D - 1, held bytes up to D = 0xFF, plate references at the top).  The query kernels read the record alone.
The step and off-step kernels encode an observation through the slot table of the record's layout (Layout.obs_descriptor) and put a
fresh world into that layout's slots, so the relocated form comes with its layout pool (`matrix_common.relocated_pool`, loaded with
set_layouts: the same layouts with every class block moved up by the same shift) - with the natural pool the device would read the
six dead natural slots, which tests/test_relocate_host.py shows on the host.  For each form, into sentinel-filled guarded buffers and
compared exactly - there is no tolerance anywhere:

  observe_grid_device    all four forms, plain and extended                               grid.host_bits (GridBufs.check)
  navigate_device        T = 8, both flag values, all three outputs                       nav.host_navigate
  partner_device         all outputs                                                      partner.host_partner
  action_effects_device  mask and effects                                                 effects_common.model (the oracle's step)
  render_device          both outputs at P = 7 (row pitch 126: the one-pixel path) and    render.host_frame, render.to_chw32
                         P = 20 (two pixel bands per row of cells, the four-pixel path)
  observe_device         float64 rows, codes, float32 rows                                Oracle.observe of the same record
  save / restore         save_device, set_state to the other form, restore_device         the records word for word, Oracle.observe

get_state() equals what was set after every call, and the device's bytes for the relocated form equal its bytes for the widened form
(grid, partner, effects, render).  On the relocated form, over the natural pool, reset_device with every second env chosen gives
`vec_common.oracle_reset` (fresh layout, natural slots, top slots zero) and leaves the other envs alone; and from the relocated form
12 steps of step_device, then of step_device_f32, follow the oracle on the same relocated records and pool: observations, rewards,
flags and records at every step, restarts on the relocated layout among them - the first time either step kernel sees live top lanes.  What keeps a cell from passing vacuously is asserted on the oracle's records
in tests/test_relocate_host.py, which also shows that each comparison made here fails for an answer with one element changed."""
import numpy as np
import pytest

import matrix_common as mc
from effects_common import OUTPUTS as EFFECT_OUTPUTS, EffectBufs
from grid_common import FORMS as GRID_FORMS, GridBufs
from nav_common import OUTPUTS as NAV_OUTPUTS, NavBufs
from partner_common import OUTPUTS as PARTNER_OUTPUTS, PartnerBufs
from render_common import FORMS as RENDER_FORMS, RenderBufs
from vec_common import SENT64, SENTINEL, Bufs, check_rows, env_of, instance, last_lean, oracle_for, oracle_reset, strip

pytestmark = pytest.mark.gpu

STARTED, LEDGER = set(), set()            # (instance, agents, scheme) of the cells that started / ran to their end


class Device:
    """one handle of the cell (plain, or with despawn / respawn on) and its sentinel-filled buffers"""

    def __init__(self, tables, inst):
        self.tables, self.inst = tables, inst
        self.env = env = env_of(tables)
        d = env.dims
        assert d.D == mc.INSTANCES[inst][0] and instance(env) == inst, f"D = {d.D}: instance {instance(env)}, not {inst}"
        env.reset(return_obs=False)
        env.load_sprites(mc.sheet())
        self.orc = oracle_for(tables)
        self.grid = {x: GridBufs(env, mc.N, x) for x in (False, True)}
        self.nav, self.partner, self.effects = NavBufs(env, mc.N, mc.NAV_T), PartnerBufs(env, mc.N), EffectBufs(env, mc.N)
        self.render = {P: RenderBufs(env, mc.N, P) for P in mc.TILES}
        self.obs = Bufs(env)
        self.archive = env.alloc((mc.N, d.RW), np.uint32)
        self.table = env.obs_table()
        self.pool_shift = 0

    def use_pool(self, shift):
        """the layout pool that goes with records relocated by `shift`: the step kernels and the off-step kernels encode an
        observation through the slot table of the record's layout, and a restart puts the fresh world into that layout's slots"""
        if shift != self.pool_shift:
            self.env.set_layouts(mc.relocated_pool(self.tables, shift))
            self.pool_shift = shift

    def unchanged(self, ctx, form):
        mc.check_records(f"{ctx}: get_state after the call", self.env.get_state(), form.records)

    def observe(self, ctx, records):
        """observe_device in all three forms against Oracle.observe of `records`"""
        b, env = self.obs, self.env
        b.fill()
        env.observe_device(b.obs, b.codes, d_obs32=b.rows32.buf)
        env.sync()
        mc.check_obs_forms(ctx, b.read(), mc.oracle_rows(self.orc, records), self.table, env.F)

    def queries(self, form, want):
        """every query kernel on one form against `want`, the host models' answers -> the bytes of the outputs that do not depend
        on where the slots sit"""
        env, dims, recs = self.env, self.env.dims, form.records
        self.use_pool(form.shift)
        env.set_state(recs)
        self.unchanged(f"{form.name}: set_state", form)
        bytes_of = {}
        for extended, b in self.grid.items():
            ctx = f"{form.name}: observe_grid_device extended={extended}"
            b.fill()
            env.observe_grid_device(extended=extended, **b.args(GRID_FORMS))
            b.check(ctx, GRID_FORMS, dims, recs)
            self.unchanged(ctx, form)
            bytes_of.update({f"grid {extended} {f}": b.buf[f].to_host() for f in GRID_FORMS})
        b = self.nav
        for wb in (False, True):
            ctx = f"{form.name}: navigate_device walkable_blocks={wb}"
            b.fill()
            b.target.from_host(want["targets"])
            env.navigate_device(b.target, walkable_blocks=wb, **b.args(NAV_OUTPUTS))
            b.check(ctx, NAV_OUTPUTS, want["nav"][wb])
            self.unchanged(ctx, form)
        b, ctx = self.partner, f"{form.name}: partner_device"
        b.fill()
        env.partner_device(**b.args(PARTNER_OUTPUTS))
        b.check(ctx, PARTNER_OUTPUTS, want["partner"])
        self.unchanged(ctx, form)
        bytes_of.update({f"partner {f}": b.buf[f].to_host() for f in PARTNER_OUTPUTS})
        b, ctx = self.effects, f"{form.name}: action_effects_device"
        b.fill()
        env.action_effects_device(**b.args(EFFECT_OUTPUTS))
        b.check(ctx, EFFECT_OUTPUTS, want["effects"])
        self.unchanged(ctx, form)
        bytes_of.update({f"effects {f}": b.buf[f].to_host() for f in EFFECT_OUTPUTS})
        for P, b in self.render.items():
            ctx = f"{form.name}: render_device P={P}"
            b.fill()
            env.render_device(P=P, vis=mc.VIS, **b.args(RENDER_FORMS))
            b.check(ctx, RENDER_FORMS, want["render"][P])
            self.unchanged(ctx, form)
            bytes_of.update({f"render {P} {f}": b.buf[f].to_host() for f in RENDER_FORMS})
        assert env.partner_bad_recipes() == 0
        ctx = f"{form.name}: observe_device"
        self.observe(ctx, recs)
        self.unchanged(ctx, form)
        return bytes_of

    def save_restore(self, kept, other):
        """save_device of `kept`, set_state to `other`, restore_device: `kept` is back word for word, with its rows"""
        env, b = self.env, self.obs
        ctx = f"{kept.name}: save, set_state({other.name}), restore"
        self.use_pool(kept.shift)
        env.set_state(kept.records)
        self.archive.from_host(np.full(self.archive.shape, 0xA5C3F00D, dtype=np.uint32))
        env.save_device(self.archive)
        mc.check_records(f"{ctx}: the archive", self.archive.to_host(), kept.records)
        env.set_state(other.records)
        self.unchanged(f"{ctx}: set_state", other)
        b.fill()
        env.restore_device(self.archive, None, b.obs, b.rows32.buf, b.codes)
        env.sync()
        mc.check_obs_forms(f"{ctx}: the restore's rows", b.read(), mc.oracle_rows(self.orc, kept.records), self.table, env.F)
        self.unchanged(ctx, kept)
        self.observe(f"{ctx}: observe_device of the restored state", kept.records)
        assert env.restore_device_refused() == 0, f"{ctx}: {env.restore_device_refused()} envs were refused"

    def reset_where(self, form, shift):
        """reset_device of every second env from the relocated form.  Over the natural pool (shift 0) the chosen envs come back in
        the level's own six slots with every slot above them zero; over the form's own pool k_reset_where writes the top slots"""
        env, b, orc = self.env, self.obs, self.orc
        ctx = f"{form.name}: reset_device over the {'relocated' if shift else 'natural'} pool"
        chosen = np.arange(mc.N) % 2 == 1
        self.use_pool(shift)
        if shift:
            orc = oracle_for(self.tables)
            orc.update_layouts(0, mc.relocated_pool(self.tables, shift))
        env.set_state(form.records)
        orc.records[:] = form.records
        rows = {int(e): oracle_reset(orc, int(e)) for e in np.nonzero(chosen)[0]}
        b.fill()
        before = b.read()
        b.mask.from_host(chosen.astype(np.uint8) * 0x81)
        env.reset_device(b.mask, None, b.obs, b.rows32.buf, b.codes)
        env.sync()
        mc.check_reset(ctx, env.get_state(), form.records, chosen, orc.records[chosen], env.dims, shift)
        check_rows(ctx, env, before, b.read(), rows)
        assert env.reset_device_refused() == 0, f"{ctx}: {env.reset_device_refused()} envs were refused"

    def steps(self, script, name, f32):
        """the script's steps from the relocated form through step_device or step_device_f32"""
        env, b = self.env, self.obs
        self.use_pool(script.form.shift)
        env.set_state(script.start)
        for t, (acts, want) in enumerate(zip(script.acts, script.want)):
            ctx = f"{name}: {'step_device_f32' if f32 else 'step_device'} step {t}"
            b.fill()
            b.act.from_host(acts)
            b.rew.from_host(np.full(b.rew.shape, np.nan))
            b.term.from_host(np.full(b.term.shape, 0xFF, np.uint8))
            b.trunc.from_host(np.full(b.trunc.shape, 0xFF, np.uint8))
            if f32:
                env.step_device_f32(b.act, b.rows32.buf, b.rew, b.term, b.trunc)
            else:
                env.step_device(b.act, b.obs, b.rew, b.term, b.trunc)
            env.sync()
            lean = last_lean(env)
            assert lean == (1 if self.inst == 0 and not f32 and not script.spawn else 0), f"{ctx}: the launch's lean flag is {lean}"
            obs, _codes, rows32 = b.read()
            assert (rows32 == SENTINEL).all() if not f32 else (obs == SENT64).all(), f"{ctx}: the observation form that was not asked for was written"
            got = (None if f32 else obs.view(np.float64), b.rew.to_host(), b.term.to_host(), b.trunc.to_host())
            mc.check_step_outputs(ctx, got, want, rows32 if f32 else None)
            mc.check_records(ctx, strip(env.get_state()), want[4])

    def close(self):
        self.env.close()


def run_forms(dev, pairs, cell):
    """the pairs (widened, relocated) of one handle: queries on both forms and the metamorphic comparison, save / restore in both
    directions, reset and steps from the relocated form"""
    for j, wide, top in pairs:
        bytes_w, bytes_r = dev.queries(wide, mc.cell_answers(*cell, j, False)), dev.queries(top, mc.cell_answers(*cell, j, True))
        for what in bytes_w:
            mc.check_equal(f"{wide.name}: {what}: the bytes for the relocated form against those for the widened form", bytes_r[what], bytes_w[what])
        dev.save_restore(top, wide)
        dev.save_restore(wide, top)
        dev.reset_where(top, 0)
        dev.reset_where(top, top.shift)
        script = mc.step_script(*cell, j)
        for f32 in (False, True):
            dev.steps(script, top.name, f32)


@pytest.mark.parametrize("cell", range(len(mc.CELLS)), ids=mc.CELL_IDS)
def test_every_query_and_offstep_kernel_of_the_cell(cell):
    inst, agents, scheme = key = mc.CELLS[cell]
    STARTED.add(key)
    tp, tps, forms = mc.cell_forms(inst, agents, scheme)
    assert len(forms) == (mc.POINTS + 1 if agents >= 2 else mc.POINTS)
    for tables, spawn in ((tp, False), (tps, True)):
        pairs = [(j, w, r) for j, (w, r) in enumerate(forms) if w.spawn == spawn]
        if not pairs:
            continue
        dev = Device(tables, inst)
        try:
            run_forms(dev, pairs, key)
            assert instance(dev.env) == inst
        finally:
            dev.close()
    LEDGER.add(key)


def test_zz_all_24_cells_ran():
    if STARTED != set(mc.CELLS):
        pytest.skip(f"{len(STARTED)} of {len(mc.CELLS)} cells were started in this session")
    print(f"query matrix cells that ran to their end: {len(LEDGER)} of {len(mc.CELLS)}")
    assert LEDGER == set(mc.CELLS), f"cells that did not run to their end: {sorted(set(mc.CELLS) - LEDGER)}"
