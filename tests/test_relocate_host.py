"""Host side of the query matrix (tests/test_gpu_query_matrix.py): `matrix_common.relocate_slots` itself; the invariances the GPU
module leans on - the host models and Oracle.observe answer the same for a checkpoint's relocated form as for its widened form, and
the observation descriptor of the relocated layout pool, walked on the host, gives the oracle's rows for the relocated records -;
the conditions that keep the GPU module from passing vacuously, measured on the oracle's records and the host models' answers, never
on the device's (the counts a run gave and the floors made from them: profiles/r26/README.md); and, for every comparison the GPU
module makes, that it passes for the host model's answer and fails for that answer with one element changed - through the same
*Bufs classes and check functions, over host-backed buffers."""
import numpy as np
import pytest

import matrix_common as mc
from cooking_zoo_amd import grid, partner, render, soa
from effects_common import OUTPUTS as EFFECT_OUTPUTS, Census, EffectBufs
from grid_common import FORMS as GRID_FORMS, GridBufs
from nav_common import OUTPUTS as NAV_OUTPUTS, NavBufs
from partner_common import OUTPUTS as PARTNER_OUTPUTS, PartnerBufs
from render_common import FORMS as RENDER_FORMS, RenderBufs
from vec_common import SENT8, SENT64, SENTINEL, check_rows, oracle_for, oracle_reset, want32

# floors: about half of what the oracle's run gave per D (the same counts at every D: the trajectories are made at natural D)
FLOORS = dict(top_alive=69, top_held=14, top_plate=124, top_changed=1000, restarts=6)


# ---------------------------------------------------------------------------------------------------------------------------
# relocate_slots
# ---------------------------------------------------------------------------------------------------------------------------

def hand_made(dims):
    """one record: slot 0 a plate, slots 1 and 2 foods in it, slot 3 a food agent 1 holds, slot 4 dead with its class left"""
    rec = soa.new_record(dims)
    rec[soa.W_T], rec[soa.W_MARKS] = 17, 0x0103
    rec[soa.AGENT_WORD0] = soa.pack_agent(1, 2, 3, -1)
    rec[soa.AGENT_WORD0 + 1] = soa.pack_agent(4, 1, 2, 3)
    rec[dims.cells_word0] = 0x01020304
    for s, (x, y, cls, flags, plate, seq) in enumerate([(2, 2, soa.PLATE, soa.DYN_ALIVE, -1, 0), (2, 2, soa.TOMATO, soa.DYN_ALIVE | soa.DYN_CHOPPED, 0, 0),
                                                       (2, 2, soa.LETTUCE, soa.DYN_ALIVE, 0, 1), (4, 1, soa.CARROT, soa.DYN_ALIVE | soa.DYN_FREE, -1, 0),
                                                       (5, 4, soa.ONION, 0, -1, 0)]):
        rec[dims.dyn0_word0 + s] = soa.pack_dyn0(x, y, cls, flags)
        rec[dims.dyn1_word0 + s] = soa.pack_dyn1(plate, seq)
    return rec


@pytest.mark.parametrize("D", [8, 64, 128, 255])
def test_relocate_slots_on_a_hand_made_record(D):
    dims = soa.Dims(6, 5, D, 2, 128)
    rec = hand_made(dims)
    shift = D - 4                                                       # the highest alive slot, 3, goes to D - 1; the dead slot 4 falls off
    assert mc.top_shift(dims, rec[None]) == shift
    out = mc.relocate_slots(dims, rec, shift)
    assert out.shape == rec.shape and out.dtype == np.uint32
    assert np.array_equal(out[:dims.dyn0_word0], np.r_[rec[:soa.AGENT_WORD0 + 1], rec[soa.AGENT_WORD0 + 1] + (shift << 24), rec[soa.AGENT_WORD0 + 2:dims.dyn0_word0]])
    assert soa.unpack_agent(out[soa.AGENT_WORD0]) == (1, 2, 3, -1), "empty hands stay empty"
    assert soa.unpack_agent(out[soa.AGENT_WORD0 + 1]) == (4, 1, 2, D - 1) and int(out[soa.AGENT_WORD0 + 1]) >> 24 == D
    for s in range(D):
        d0, d1 = soa.unpack_dyn0(out[dims.dyn0_word0 + s]), soa.unpack_dyn1(out[dims.dyn1_word0 + s])
        if s < shift:
            assert d0 == (0, 0, 0, 0) and d1 == (-1, 0), f"slot {s} is not zero"
        else:
            w0, (plate, seq) = soa.unpack_dyn0(rec[dims.dyn0_word0 + s - shift]), soa.unpack_dyn1(rec[dims.dyn1_word0 + s - shift])
            assert d0 == w0 and d1 == (plate + shift if plate >= 0 else -1, seq), f"slot {s}"
    assert not out[dims.dyn1_word0 + D:].any(), "padding words"
    assert np.array_equal(mc.relocate_slots(dims, rec, 0), rec)
    assert np.array_equal(mc.relocate_slots(dims, np.stack([rec, rec]), shift), np.stack([out, out]))
    with pytest.raises(AssertionError, match="alive"):
        mc.relocate_slots(dims, rec, shift + 1)                         # slot 3 would leave the record


# ---------------------------------------------------------------------------------------------------------------------------
# the invariances, per cell
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", range(len(mc.CELLS)), ids=mc.CELL_IDS)
def test_the_host_models_do_not_see_where_the_slots_sit(cell):
    inst, agents, scheme = mc.CELLS[cell]
    tp, tps, forms = mc.cell_forms(inst, agents, scheme)
    D = mc.INSTANCES[inst][0]
    assert len(forms) == (mc.POINTS + 1 if agents >= 2 else mc.POINTS) and tp.dims.D == D and tp.dims.huge == (inst == 2)
    for j, (wide, top) in enumerate(forms):
        tables = tps if wide.spawn else tp
        dims = tables.dims
        alive_w, alive_t = mc.alive_slots(dims, wide.records), mc.alive_slots(dims, top.records)
        assert alive_t[:, D - 1].any() and not alive_w[:, 6:].any(), f"{top.name}: no env has an alive object in slot {D - 1}"
        assert np.array_equal(alive_t.sum(axis=1), alive_w.sum(axis=1)) and not alive_t[:, :D - 6].any()
        assert np.array_equal(mc.held_bytes(dims, top.records) != 0, mc.held_bytes(dims, wide.records) != 0)
        if wide.spawn:
            assert ((wide.records[:, soa.W_STATUS] >> 8) & 0xF).any(), f"{wide.name}: no agent is despawned"
        for extended in (False, True):
            mc.check_equal(f"{top.name}: grid.host_bits extended={extended}", grid.host_bits(dims, top.records, extended),
                           grid.host_bits(dims, wide.records, extended))
        mc.check_equal(f"{top.name}: grid.agent_xy", grid.agent_xy(dims, top.records), grid.agent_xy(dims, wide.records))
        a_w, a_t = mc.cell_answers(inst, agents, scheme, j, False), mc.cell_answers(inst, agents, scheme, j, True)
        mc.check_equal(f"{top.name}: the targets", a_t["targets"], a_w["targets"])
        for wb in (False, True):
            for name, x, y in zip(NAV_OUTPUTS, a_t["nav"][wb], a_w["nav"][wb]):
                mc.check_equal(f"{top.name}: nav.host_navigate walkable_blocks={wb} {name}", x, y)
        for name, x, y in zip(PARTNER_OUTPUTS, a_t["partner"], a_w["partner"]):
            mc.check_equal(f"{top.name}: partner.host_partner {name}", x, y)
        mc.check_equal(f"{top.name}: effects_common.model", a_t["effects"], a_w["effects"])
        for P in mc.TILES:
            mc.check_equal(f"{top.name}: render.host_frame P={P}", a_t["render"][P], a_w["render"][P])
        orc = oracle_for(tables)
        rows = mc.oracle_rows(orc, top.records)
        mc.check_equal(f"{top.name}: Oracle.observe", rows.view(np.uint64), mc.oracle_rows(orc, wide.records).view(np.uint64))
        # the device encodes a record through the slot table of its layout: the relocated pool's descriptor gives the oracle's rows
        # for the relocated records, the natural pool's for the widened ones - and the natural pool's would miss the relocated objects
        assert top.shift == mc.top_shift(dims, wide.records) >= D - 6 and wide.shift == 0
        mc.check_equal(f"{top.name}: the relocated pool's descriptor", mc.descriptor_rows(tables, top.records, top.shift).view(np.uint64), rows.view(np.uint64))
        mc.check_equal(f"{wide.name}: the natural pool's descriptor", mc.descriptor_rows(tables, wide.records, 0).view(np.uint64), rows.view(np.uint64))
        assert not np.array_equal(mc.descriptor_rows(tables, top.records, 0), rows), f"{top.name}: the natural pool's descriptor sees the relocated objects"
        for lay, moved in zip(tables.layouts, mc.relocated_pool(tables, top.shift)):
            assert moved.slots_used <= D and all(moved.slot_base[c] == lay.slot_base[c] + top.shift for c in moved.slot_base)
            # (a fresh world's last slot may be the Bread's clone head-room, and two of the four layouts have no Lettuce behind it)
            assert mc.alive_slots(dims, moved.init_record(dims, 0)[None])[0, D - 3:].any(), f"{top.name}: a fresh world of the relocated pool is not at the top"
            assert np.array_equal(moved.init_record(dims, 0), mc.relocate_slots(dims, np.where(np.arange(dims.RW) < dims.dyn0_word0 + D - top.shift,
                                  lay.init_record(dims, 0), 0).astype(np.uint32), top.shift)), "the relocated layout's fresh record"


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU module does not pass vacuously
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inst", range(3), ids=["D64", "D128", "D255"])
def test_the_cells_of_an_instance_reach_the_top_lanes(inst):
    D = mc.INSTANCES[inst][0]
    total = dict(top_alive=0, top_held=0, top_plate=0, top_changed=0, restarts=0)
    codes, effects_seen = set(), Census()
    for i, agents, scheme in mc.CELLS:
        if i != inst:
            continue
        c = mc.census(i, agents, scheme)
        for k in total:
            total[k] += c[k]
        codes |= c["codes"]
        assert partner.WALK in c["statuses"], f"{agents} agents {scheme}: partner statuses {sorted(c['statuses'])}"
        assert agents == 1 or len(c["statuses"]) >= 2, f"{agents} agents {scheme}: partner statuses {sorted(c['statuses'])}"
        for eff, live in c["effects"]:
            effects_seen.add(scheme, eff, live)
    print(f"D = {D}: {total}, walk codes {sorted(codes)}")
    print({s: dict(zip(("MOVED", "TURNED", "HAND", "OBJECTS", "CELLS"), effects_seen.bits[s].tolist())) for s in sorted(effects_seen.bits)})
    assert codes == {0, 1, 2, 3, 4}, f"walk codes seen: {sorted(codes)}"
    effects_seen.check(f"D = {D}", ("scheme3", "scheme1"))
    for k, floor in FLOORS.items():
        assert total[k] >= floor, f"D = {D}: {k} = {total[k]}, below the floor {floor}"


# ---------------------------------------------------------------------------------------------------------------------------
# every comparison of the GPU module fails when it should
# ---------------------------------------------------------------------------------------------------------------------------

CELL = (2, 4, "scheme1")                  # D = 255: the held byte 0xFF
J = 3


def fails(match, fn, *args, **kw):
    with pytest.raises(AssertionError, match=match):
        fn(*args, **kw)


def one_form():
    tp, _tps, forms = mc.cell_forms(*CELL)
    return tp, mc.HostEnv(tp), forms[J][0], forms[J][1]


def top_object(dims, records):
    """(env, x, y, class) of an alive object in slot D - 1"""
    e = int(np.nonzero(mc.alive_slots(dims, records)[:, dims.D - 1])[0][0])
    x, y, cls, _flags = soa.unpack_dyn0(records[e, dims.dyn0_word0 + dims.D - 1])
    return e, x, y, cls


def test_grid_check_fails_for_the_top_slots_bit():
    tp, env, _wide, top = one_form()
    dims, recs = tp.dims, top.records
    e, x, y, cls = top_object(dims, recs)
    ch = grid.DYN_CHANNEL[cls]
    for extended in (False, True):
        b = GridBufs(env, mc.N, extended)
        bits = grid.host_bits(dims, recs, extended)
        good = dict(bits=bits, grid8=grid.expand(bits, np.uint8), grid32=grid.expand(bits, np.float32), agent_xy=grid.agent_xy(dims, recs))

        def load(**changed):
            b.fill()
            for f in GRID_FORMS:
                mc.put(b.buf[f], changed.get(f, good[f]))

        load()
        b.check("host model", GRID_FORMS, dims, recs)
        assert bits[e, x, y, ch >> 5] >> (ch & 31) & 1, "the top slot's class bit is not set in the host model"
        wrong = bits.copy()
        wrong[e, x, y, ch >> 5] &= ~np.uint32(1 << (ch & 31))
        load(bits=wrong)
        fails("bits differs", b.check, "top bit", GRID_FORMS, dims, recs)
        wrong = good["grid8"].copy()
        wrong[e, x, y, ch] = 0
        load(grid8=wrong)
        fails("grid8 differs", b.check, "top byte", GRID_FORMS, dims, recs)
        wrong = good["grid32"].copy()
        wrong[e, x, y, ch] = 0.0
        load(grid32=wrong)
        fails("grid32 differs", b.check, "top float", GRID_FORMS, dims, recs)
        wrong = good["agent_xy"].copy()
        wrong[-1, -1, 1] += 1
        load(agent_xy=wrong)
        fails("agent_xy differs", b.check, "agent", GRID_FORMS, dims, recs)
        load()
        b.buf["bits"].data[b.size["bits"]] = 0
        fails("behind the last cell", b.check, "guard", GRID_FORMS, dims, recs)


def test_nav_partner_effects_and_render_checks_fail_for_one_element():
    tp, env, _wide, top = one_form()
    ans = mc.cell_answers(*CELL, J, True)
    cases = [(NavBufs(env, mc.N, mc.NAV_T), NAV_OUTPUTS, ans["nav"][False], lambda b, w: b.check("nav", NAV_OUTPUTS, w)),
             (PartnerBufs(env, mc.N), PARTNER_OUTPUTS, ans["partner"], lambda b, w: b.check("partner", PARTNER_OUTPUTS, w))]
    for b, outputs, want, check in cases:
        for k, f in enumerate(outputs):
            b.fill()
            for g, w in zip(outputs, want):
                mc.put(b.buf[g], w)
            check(b, want)
            wrong = np.array(want[k]).copy()
            wrong.reshape(-1)[-1] = (int(wrong.reshape(-1)[-1]) + 1) % 5          # a walk code, a coordinate, a distance, a status: one off
            mc.put(b.buf[f], wrong)
            fails(f"{f} differs", check, b, want)
    # the mask follows the effects: one effect byte cleared changes it too when it was the action's only effect
    b, eff = EffectBufs(env, mc.N), ans["effects"]
    from cooking_zoo_amd import effects
    for f in EFFECT_OUTPUTS:
        b.fill()
        mc.put(b.buf["mask"], effects.mask_of(eff))
        mc.put(b.buf["effects"], eff)
        b.check("effects", EFFECT_OUTPUTS, eff)
        at = tuple(np.argwhere(eff != 0)[-1])
        wrong = (effects.mask_of(eff) if f == "mask" else eff).copy()
        wrong[at] = 0
        mc.put(b.buf[f], wrong)
        fails(f"{f} differs", b.check, "effects", EFFECT_OUTPUTS, eff)
    for P in mc.TILES:
        b, frames = RenderBufs(env, mc.N, P), ans["render"][P]
        for f in RENDER_FORMS:
            b.fill()
            mc.put(b.buf["rgb8"], frames)
            mc.put(b.buf["chw32"], render.to_chw32(frames))
            b.check("render", RENDER_FORMS, frames)
            wrong = frames.copy()
            wrong[-1, -1, -1, 2] ^= 1                                             # the last byte of the last frame, off by one
            mc.put(b.buf[f], wrong if f == "rgb8" else render.to_chw32(wrong))
            fails(f"{f} differs", b.check, "render", RENDER_FORMS, frames)
            mc.put(b.buf[f], frames if f == "rgb8" else render.to_chw32(frames))
            b.buf[f].data[b.size[f]] = 0
            fails("behind the last frame", b.check, "render", RENDER_FORMS, frames)


def table_of(*rows):
    """a table of 256 float64 that holds every value of `rows`, and the function that gives the codes of rows in it"""
    values = np.unique(np.concatenate([np.asarray(r).reshape(-1) for r in rows]))
    assert 2 <= len(values) < 255
    table = np.zeros(256)
    table[:len(values)] = values
    return table, lambda r: np.searchsorted(values, r).astype(np.uint8)


def fresh_records(orc, records, chosen):
    """the oracle's fresh records of the chosen envs (`vec_common.oracle_reset`)"""
    orc.records[:] = records
    for e in np.nonzero(chosen)[0]:
        oracle_reset(orc, int(e))
    return orc.records[chosen].copy()


def test_record_row_reset_and_step_checks_fail_for_one_element():
    tp, env, wide, top = one_form()
    dims, F = tp.dims, tp.F
    orc = oracle_for(tp)
    rows = mc.oracle_rows(orc, top.records)
    chosen = np.arange(mc.N) % 2 == 1
    fresh = fresh_records(orc, top.records, chosen)
    assert mc.alive_slots(dims, fresh)[:, :6].any() and not fresh[:, dims.dyn0_word0 + 6:dims.dyn0_word0 + dims.D].any(), "the natural pool's fresh worlds"
    fresh_rows = {int(e): mc.oracle_rows(orc, fresh[k:k + 1])[0] for k, e in enumerate(np.nonzero(chosen)[0])}
    table, code = table_of(rows, *fresh_rows.values())
    codes = code(rows)
    assert np.array_equal(table[codes], rows)
    inexact = np.argwhere(rows.astype(np.float32).astype(np.float64) != rows)
    assert len(inexact), "no element of the rows is inexact in float32"
    # records: get_state after a call, the archive, the restored batch, the metamorphic comparison
    mc.check_records("records", top.records.copy(), top.records)
    wrong = top.records.copy()
    wrong[-1, dims.dyn1_word0 + dims.D - 1] ^= 0x100
    fails("records: differs", mc.check_records, "records", wrong, top.records)
    mc.check_equal("bytes", wide.records.view(np.uint8), wide.records.view(np.uint8).copy())
    fails("bytes: differs", mc.check_equal, "bytes", wrong.view(np.uint8), top.records.view(np.uint8))
    # the three observation forms
    good = (rows.view(np.uint64), codes, want32(rows))
    mc.check_obs_forms("rows", good, rows, table, F)
    for k, what in enumerate(("float64 rows", "codes", "float32 rows")):
        changed = [g.copy() for g in good]
        if k == 1:
            changed[1][tuple(np.argwhere(codes == 0)[-1])] = 1                    # the table's smallest value for the next one
        else:
            changed[k][tuple(inexact[-1])] += 1                                   # one unit in the last place
        fails(f"{what}: differs", mc.check_obs_forms, "rows", tuple(changed), rows, table, F)
    fails("padding bytes", mc.check_obs_forms, "rows", (good[0], np.concatenate([codes, np.full(codes.shape[:2] + (16,), 7, np.uint8)], axis=2), good[2]),
          rows, table, F)
    # reset_device: records, and the rows through vec_common.check_rows
    after = top.records.copy()
    after[chosen] = fresh
    mc.check_reset("reset", after, top.records, chosen, fresh, dims)
    wrong = after.copy()
    wrong[0, soa.W_T] += 1
    fails("not chosen: differs", mc.check_reset, "reset", wrong, top.records, chosen, fresh, dims)
    wrong = after.copy()
    wrong[1, soa.AGENT_WORD0] ^= 1
    fails("chosen envs: differs", mc.check_reset, "reset", wrong, top.records, chosen, fresh, dims)
    wrong, stale = after.copy(), fresh.copy()
    wrong[1, dims.dyn0_word0 + dims.D - 1] = stale[0, dims.dyn0_word0 + dims.D - 1] = soa.pack_dyn0(2, 2, soa.TOMATO, soa.DYN_ALIVE)
    fails("is not zero after the reset", mc.check_reset, "reset", wrong, top.records, chosen, stale, dims)
    # ... and over the relocated pool, whose fresh worlds sit at the top
    orc_top = oracle_for(tp)
    orc_top.update_layouts(0, mc.relocated_pool(tp, top.shift))
    fresh_top = fresh_records(orc_top, top.records, chosen)
    assert mc.alive_slots(dims, fresh_top)[:, dims.D - 3:].any(axis=1).all() and not mc.alive_slots(dims, fresh_top)[:, :top.shift].any()
    after_top = top.records.copy()
    after_top[chosen] = fresh_top
    mc.check_reset("reset", after_top, top.records, chosen, fresh_top, dims, top.shift)
    fails("is not zero after the reset", mc.check_reset, "reset", after_top, top.records, chosen, fresh_top, dims, 0)
    env.obs_table = lambda: table
    n, A = mc.N, dims.A
    before = (np.full((n, A, F), SENT64, np.uint64), np.full((n, A, F), SENT8, np.uint8), np.full((n, A, F), SENTINEL, np.uint32))
    got = [x.copy() for x in before]
    for e, r in fresh_rows.items():
        got[0][e], got[1][e], got[2][e] = r.view(np.uint64), code(r), want32(r)
    check_rows("reset rows", env, before, tuple(got), fresh_rows)
    for k, what in enumerate(("float64 rows", "codes of env", "float32 rows")):
        changed = [g.copy() for g in got]
        changed[k][1, -1, 0] += 1
        fails(what, check_rows, "reset rows", env, before, tuple(changed), fresh_rows)
        changed = [g.copy() for g in got]
        changed[k][0, 0, 0] += 1                                                  # a row of an env that was not chosen
        fails(what if k != 1 else "were touched", check_rows, "reset rows", env, before, tuple(changed), fresh_rows)
    # the steps
    script = mc.step_script(*CELL, J)
    obs, rew, term, trunc, _recs = script.want[0]
    mc.check_step_outputs("step", (obs, rew, term, trunc), script.want[0])
    mc.check_step_outputs("step", (None, rew, term, trunc), script.want[0], want32(obs))
    at = tuple(np.argwhere(obs.astype(np.float32).astype(np.float64) != obs)[-1])
    wrong = obs.copy().view(np.uint64)
    wrong[at] += 1
    fails("observation: differs", mc.check_step_outputs, "step", (wrong.view(np.float64), rew, term, trunc), script.want[0])
    wrong = want32(obs).copy()
    wrong[at] += 1
    fails("float32 observation: differs", mc.check_step_outputs, "step", (None, rew, term, trunc), script.want[0], wrong)
    wrong = rew.copy().view(np.uint64)
    wrong[-1, -1] ^= 1
    fails("rewards: differs", mc.check_step_outputs, "step", (obs, wrong.view(np.float64), term, trunc), script.want[0])
    fails("terminations: differs", mc.check_step_outputs, "step", (obs, rew, term ^ np.uint8(1), trunc), script.want[0])
    fails("truncations: differs", mc.check_step_outputs, "step", (obs, rew, term, trunc ^ np.uint8(1)), script.want[0])
