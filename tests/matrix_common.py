"""Helpers of the query matrix (tests/test_relocate_host.py on the host, tests/test_gpu_query_matrix.py on the device): the 24 cells
(kernel instance x agents x scheme) over one small world, slot relocation of records and of the layout pool that goes with them, the
oracle's checkpoints in the two forms the device is shown, the step scripts, the host models' answers, exact comparisons with messages
of their own, and host-backed stand-ins for device buffers, so that every comparison the GPU module makes can be shown to fail on the
host.  Nothing here touches the device library."""
import functools

import numpy as np

from cooking_zoo_amd import effects, nav, partner, render, soa
from effects_common import live_rows, model as effects_model
from grid_common import SPAWN
from nav_common import draw_targets
from partner_common import book_of
from render_common import random_sheet
from vec_common import CROWDED4, oracle_for, tables_of, want32, widen

LEVEL = META = "crowded_6x5"
N, LAYOUTS, POINTS, STEPS, MAX_STEPS = 8, 4, 4, 120, 200        # (no episode is cut by the clock: the worlds stay worked on)
INSTANCES = [(64, 0), (128, 1), (255, 2)]                        # (max_dyn, kernel instance): D at the top of the instance
CELLS = [(inst, agents, scheme) for inst in range(3) for agents in (1, 2, 3, 4) for scheme in ("scheme3", "scheme1")]
CELL_IDS = [f"inst{i}-{a}agents-{s}" for i, a, s in CELLS]
NAV_T, TILES, SHEET_M, VIS = 8, (7, 20), 8, 0b0110
STEP_T = 12                                                      # steps taken from the relocated form


def seed_of(agents, scheme):
    """the policy's seed of a trajectory: one per (agents, scheme), the same on every instance"""
    return 260 + 2 * agents + (scheme == "scheme1")


# ---------------------------------------------------------------------------------------------------------------------------
# slot relocation
# ---------------------------------------------------------------------------------------------------------------------------

def relocate_slots(dims, records, shift):
    """records uint32 [n][RW] (or one record) with slot s moved to slot s + shift: the dyn0 and dyn1 words move together, every
    agent's held byte and every dyn1 plate byte that names a slot is raised by `shift`, vacated slots are zero.  A shift keeps the
    slot order (the oracle wants static content in slot order).  The slots that would leave [0, D) must be dead: what a dead slot
    still holds of the object it was (class, cell) is dropped with it, as nothing reads a dead slot."""
    recs = np.array(records, dtype=np.uint32)
    single = recs.ndim == 1
    recs = recs.reshape(-1, recs.shape[-1])
    D, shift = dims.D, int(shift)
    assert recs.shape[1] == dims.RW, f"relocate_slots: records of {recs.shape[1]} words, the dims say {dims.RW}"
    assert 0 <= shift < D, f"relocate_slots: shift {shift} with D = {D}"
    d0, d1 = slice(dims.dyn0_word0, dims.dyn0_word0 + D), slice(dims.dyn1_word0, dims.dyn1_word0 + D)
    dyn0, dyn1 = recs[:, d0].copy(), recs[:, d1].copy()
    assert not ((dyn0[:, D - shift:] >> 24) & soa.DYN_ALIVE).any(), f"relocate_slots: a slot at or above {D - shift} is alive"
    assert not (dyn1[:, D - shift:] & 0xFF).any(), f"relocate_slots: a dead slot at or above {D - shift} carries a plate reference"
    agents = recs[:, soa.AGENT_WORD0:soa.AGENT_WORD0 + dims.A]
    held = agents >> 24
    assert (held <= D - shift).all(), "relocate_slots: an agent holds a slot that would leave the record"
    agents[held != 0] += np.uint32(shift << 24)
    plate = dyn1 & 0xFF
    assert (plate <= D - shift).all(), "relocate_slots: a plate reference would leave the record"
    dyn1[plate != 0] += np.uint32(shift)
    recs[:, d0], recs[:, d1] = 0, 0
    recs[:, dims.dyn0_word0 + shift:dims.dyn0_word0 + D] = dyn0[:, :D - shift]
    recs[:, dims.dyn1_word0 + shift:dims.dyn1_word0 + D] = dyn1[:, :D - shift]
    return recs[0] if single else recs


def relocate_layout(layout, shift, D):
    """a copy of `layout` whose slot table starts `shift` slots up: every class block at its base + shift, in the same order.  The
    device encodes an observation through the slot table of the record's layout (Layout.obs_descriptor), so records relocated by
    `shift` are the worlds of such a layout, not of the natural one.  A block that would pass D is cut there and a class behind it
    is left out (relocate_slots asserts that those slots are dead in the records): its features are the padding zeros."""
    import copy
    out = copy.copy(layout)
    out.dyn_classes, out.dyn_xy, out.slot_base, out.slot_cap, out.slots_used = [], [], {}, {}, 0
    first = 0
    for cls, n in layout.dyn_classes:
        base, cap = layout.slot_base[cls], min(layout.slot_cap[cls], D - int(shift) - layout.slot_base[cls])
        if cap > 0:
            keep = min(n, cap)
            out.dyn_classes.append((cls, keep))
            out.dyn_xy += layout.dyn_xy[first:first + keep]
            out.slot_base[cls], out.slot_cap[cls] = base + int(shift), cap
            out.slots_used = base + int(shift) + cap
        first += n
    assert out.slots_used <= D, f"relocate_layout: the slot table ends at {out.slots_used}, behind D = {D}"
    return out


def relocated_pool(tables, shift):
    """the layout pool of `tables` for records relocated by `shift` (0: the pool itself)"""
    return list(tables.layouts) if not shift else [relocate_layout(l, shift, tables.dims.D) for l in tables.layouts]


def alive_slots(dims, records):
    """bool [n][D]"""
    recs = np.asarray(records, dtype=np.uint32).reshape(-1, dims.RW)
    return ((recs[:, dims.dyn0_word0:dims.dyn0_word0 + dims.D] >> 24) & soa.DYN_ALIVE) != 0


def held_bytes(dims, records):
    """[n][A]: slot + 1 of what the agent holds, 0 for empty hands"""
    recs = np.asarray(records, dtype=np.uint32).reshape(-1, dims.RW)
    return (recs[:, soa.AGENT_WORD0:soa.AGENT_WORD0 + dims.A] >> 24).astype(np.int64)


def plate_bytes(dims, records):
    """[n][D]: slot + 1 of the plate an alive object lies in, 0 for none (and for every dead slot)"""
    recs = np.asarray(records, dtype=np.uint32).reshape(-1, dims.RW)
    return np.where(alive_slots(dims, recs), recs[:, dims.dyn1_word0:dims.dyn1_word0 + dims.D] & 0xFF, 0).astype(np.int64)


def top_shift(dims, records):
    """the shift that puts the batch's highest alive slot into slot D - 1"""
    alive = alive_slots(dims, records)
    assert alive.any(), "top_shift: no alive object in the batch"
    return dims.D - 1 - int(np.nonzero(alive.any(axis=0))[0].max())


# ---------------------------------------------------------------------------------------------------------------------------
# the cells' checkpoints
# ---------------------------------------------------------------------------------------------------------------------------

def cell_tables(agents, scheme, max_dyn=None, spawn=False):
    """device-free tables of the cell's world; max_dyn None: the level's own D = 6.  The layout pool does not depend on max_dyn."""
    return tables_of(N, LEVEL, META, agents, CROWDED4[:agents], scheme, max_steps=MAX_STEPS, num_layouts=LAYOUTS, max_dyn=max_dyn,
                     **(SPAWN if spawn else {}))


@functools.lru_cache(maxsize=None)
def natural_checkpoints(agents, scheme, spawn=False):
    """the oracle's records uint32 [points][N][RW] at natural D: POINTS evenly spaced steps of one trajectory under the state-aware
    policy, or - with despawn / respawn on - the one checkpoint at its end.  Computed once and shared: do not write to it."""
    from fuzz_policy import BumperActions
    tables = cell_tables(agents, scheme, None, spawn)
    assert (tables.dims.W, tables.dims.H, tables.dims.D) == (6, 5, 6), "crowded_6x5 changed"
    orc = oracle_for(tables)
    orc.reset()
    # (+ 51 with despawn / respawn on: with + 50 the two-agent scheme3 batch has nobody despawned at its checkpoint)
    pol = BumperActions(tables.dims, tables.scheme_class.CODE, np.random.default_rng(seed_of(agents, scheme) + (51 if spawn else 0)))
    at = {STEPS} if spawn else {STEPS * (k + 1) // POINTS for k in range(POINTS)}
    out = []
    for t in range(1, STEPS + 1):
        orc.step(pol.act(orc.records), want_obs=False)
        pol.observe_result(orc.records)
        if t in at:
            out.append(orc.records.copy())
    recs = np.stack(out)
    recs.setflags(write=False)
    return tables, recs


class Form:
    """one checkpoint as the device is shown it: `name`, the records at the cell's D, by how many slots they were relocated (0:
    widened only; the layout pool that goes with them is `relocated_pool(tables, shift)`), and whether despawn / respawn is on"""

    def __init__(self, name, records, shift, spawn):
        self.name, self.records, self.shift, self.spawn = name, records, int(shift), spawn
        self.records.setflags(write=False)


@functools.lru_cache(maxsize=None)
def cell_forms(inst, agents, scheme):
    """-> (tables at the cell's D, spawn tables at the cell's D or None, [(widened Form, relocated Form)] per checkpoint): four
    checkpoints of the plain trajectory and, for 2 or more agents, one with despawn / respawn on"""
    max_dyn = INSTANCES[inst][0]
    out = []
    padded = {}
    for spawn in ((False, True) if agents >= 2 else (False,)):
        tn, points = natural_checkpoints(agents, scheme, spawn)
        padded[spawn] = tp = cell_tables(agents, scheme, max_dyn, spawn)
        assert tp.dims.D == max_dyn
        for k, recs in enumerate(points):
            wide = widen(recs, tn.dims, tp.dims)
            name = f"{'spawn ' if spawn else ''}checkpoint {k}"
            shift = top_shift(tp.dims, wide)
            out.append((Form(f"{name} widened", wide, 0, spawn), Form(f"{name} relocated", relocate_slots(tp.dims, wide, shift), shift, spawn)))
    return padded[False], padded.get(True), out


class StepScript:
    """STEP_T steps of the oracle from the relocated form of checkpoint j of the cell (the oracle alone, at the cell's D): the
    actions of the state-aware policy, per step (observation, rewards, terminations, truncations, records), and on how many
    env-steps a word of the six top slots changed"""

    def __init__(self, inst, agents, scheme, j):
        from fuzz_policy import BumperActions
        tp, tps, forms = cell_forms(inst, agents, scheme)
        form = forms[j][1]
        tables = tps if form.spawn else tp
        d = tables.dims
        orc = oracle_for(tables)
        orc.update_layouts(0, relocated_pool(tables, form.shift))        # (an env that finishes restarts on the relocated layout)
        orc.records[:] = form.records
        pol = BumperActions(d, tables.scheme_class.CODE, np.random.default_rng(seed_of(agents, scheme) + 7 * j + 1))
        top = np.r_[d.dyn0_word0 + d.D - 6:d.dyn0_word0 + d.D, d.dyn1_word0 + d.D - 6:d.dyn1_word0 + d.D]
        self.form, self.start, self.spawn, self.acts, self.want, self.top_changed = form, form.records, form.spawn, [], [], 0
        self.restarts = 0                                                # env-steps on which an env began a new episode
        for _ in range(STEP_T):
            before = orc.records.copy()
            acts = np.ascontiguousarray(pol.act(orc.records), dtype=np.int32)
            obs, rew, term, trunc = orc.step(acts)
            pol.observe_result(orc.records)
            self.acts.append(acts)
            self.want.append((obs.copy(), rew.copy(), term.copy(), trunc.copy(), orc.records.copy()))
            self.top_changed += int((before[:, top] != orc.records[:, top]).any(axis=1).sum())
            self.restarts += int((before[:, soa.W_EPISODE] != orc.records[:, soa.W_EPISODE]).sum())


@functools.lru_cache(maxsize=None)
def step_script(inst, agents, scheme, j):
    return StepScript(inst, agents, scheme, j)


# ---------------------------------------------------------------------------------------------------------------------------
# what the host models say of one form
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sheet():
    s = random_sheet(SHEET_M, 26)
    s.setflags(write=False)
    return s


def nav_targets(dims, records, k):
    return draw_targets(dims, records, NAV_T, 31 * k + NAV_T)


def host_answers(tables, form, k, which=("nav", "partner", "effects", "render")):
    """the host models' answers for one form of checkpoint k: nav -> {flag: (actions, steps, field)} and the targets; partner ->
    (actions, targets, status); effects -> uint8 [n][A][n_actions]; render -> {P: frames}.  (The grid's is made by GridBufs.check.)"""
    dims, recs, out = tables.dims, form.records, {}
    if "nav" in which:
        out["targets"] = tg = nav_targets(dims, recs, k)
        out["nav"] = {wb: nav.host_navigate(dims, recs, tg, wb) for wb in (False, True)}
    if "partner" in which:
        out["partner"] = partner.host_partner(dims, tables.layouts, recs, book_of(tables))
    if "effects" in which:
        out["effects"] = effects_model(tables, recs)
    if "render" in which:
        out["render"] = {P: render.host_frame(dims, recs, P, sheet(), VIS) for P in TILES}
    return out


@functools.lru_cache(maxsize=None)
def cell_answers(inst, agents, scheme, j, relocated):
    """`host_answers` of one form of pair j of the cell, computed once and shared: do not write to it"""
    tp, tps, forms = cell_forms(inst, agents, scheme)
    form = forms[j][1 if relocated else 0]
    return host_answers(tps if form.spawn else tp, form, j)


def census(inst, agents, scheme):
    """what the relocated forms of one cell show, on the oracle's records and the host models' answers alone: records with an alive
    object in slot D - 1, agents that hold slot D - 1, objects in a plate whose slot is at least D - 6, the walk codes and partner
    statuses seen, the effects of the live rows, and the env-steps of the step scripts on which a top slot changed and on which an env
    began a new episode (on the relocated layout)"""
    tp, tps, forms = cell_forms(inst, agents, scheme)
    D = tp.dims.D
    out = dict(top_alive=0, top_held=0, top_plate=0, codes=set(), statuses=set(), effects=[], top_changed=0, restarts=0)
    for j, (_wide, top) in enumerate(forms):
        recs, ans = top.records, cell_answers(inst, agents, scheme, j, True)
        out["top_alive"] += int(alive_slots(tp.dims, recs)[:, D - 1].sum())
        out["top_held"] += int((held_bytes(tp.dims, recs) == D).sum())
        out["top_plate"] += int((plate_bytes(tp.dims, recs) >= D - 6 + 1).sum())
        for wb in (False, True):
            out["codes"] |= set(np.unique(ans["nav"][wb][0]).tolist())
        out["statuses"] |= set(np.unique(ans["partner"][2]).tolist())
        out["effects"].append((ans["effects"], live_rows(recs, agents)))
        out["top_changed"] += step_script(inst, agents, scheme, j).top_changed
        out["restarts"] += step_script(inst, agents, scheme, j).restarts
    return out


def descriptor_rows(tables, records, shift):
    """float64 rows [n][A][F] of `records` the way the device encodes them: the observation descriptor of the record's layout in
    `relocated_pool(tables, shift)`, walked on the host (host_common.eval_descriptor)"""
    from host_common import eval_descriptor
    desc = [l.obs_descriptor(tables.meta, tables.dims) for l in relocated_pool(tables, shift)]
    return np.stack([eval_descriptor(desc[int(r[soa.W_LAYOUT])], tables.dims, r) for r in records])


def oracle_rows(orc, records):
    """float64 rows [n][A][F] of `records` by Oracle.observe"""
    return np.stack([orc.oracle.observe(np.ascontiguousarray(r)) for r in records])


# ---------------------------------------------------------------------------------------------------------------------------
# exact comparisons (pytest rewrites asserts in test modules only: every assert here carries its own message)
# ---------------------------------------------------------------------------------------------------------------------------

def check_equal(ctx, got, want):
    """two arrays of one shape and dtype, element for element"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{ctx}: got {got.dtype}{got.shape}, want {want.dtype}{want.shape}"
    bad = np.argwhere(got != want)
    assert not len(bad), f"{ctx}: differs at {bad[:6].tolist()} ({len(bad)} elements): got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def check_obs_forms(ctx, got, want64, table, F):
    """got = (float64 rows as uint64, codes uint8 [n][A][codes_pitch], float32 rows as uint32) against the oracle's float64 rows"""
    obs, codes, r32 = got
    check_equal(f"{ctx}: float64 rows", obs, np.ascontiguousarray(want64).view(np.uint64))
    assert (codes[..., F:] == 255).all(), f"{ctx}: padding bytes of the codes"
    check_equal(f"{ctx}: codes", np.ascontiguousarray(table[codes[..., :F]]).view(np.uint64), np.ascontiguousarray(want64).view(np.uint64))
    check_equal(f"{ctx}: float32 rows", r32, want32(want64))


def check_records(ctx, got, want):
    """records word for word"""
    check_equal(f"{ctx}: records", np.asarray(got, dtype=np.uint32), np.asarray(want, dtype=np.uint32))


def check_step_outputs(ctx, got, want, rows32=None):
    """got = (float64 rows or None, rewards, terminations, truncations) of one step against the oracle's, bit for bit; rows32: the
    float32 rows as uint32 where the step wrote those"""
    obs, rew, term, trunc = got
    if obs is not None:
        check_equal(f"{ctx}: observation", np.ascontiguousarray(obs).view(np.uint64), np.ascontiguousarray(want[0]).view(np.uint64))
    if rows32 is not None:
        check_equal(f"{ctx}: float32 observation", rows32, want32(want[0]))
    check_equal(f"{ctx}: rewards", np.ascontiguousarray(rew).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))
    check_equal(f"{ctx}: terminations", term, want[2])
    check_equal(f"{ctx}: truncations", trunc, want[3])


def check_reset(ctx, got, before, chosen, want_chosen, dims, shift=0):
    """records after a reset_device over the pool relocated by `shift`: the chosen envs are the oracle's fresh worlds - the level's
    six slots from slot `shift` on (0: the natural slots), every other slot zero -, the others are what they were"""
    got, chosen = np.asarray(got), np.asarray(chosen, dtype=bool)
    check_equal(f"{ctx}: envs that were not chosen", got[~chosen], np.asarray(before)[~chosen])
    check_equal(f"{ctx}: chosen envs", got[chosen], np.asarray(want_chosen))
    outside = np.r_[0:shift, shift + 6:dims.D]
    rest = np.concatenate([got[chosen][:, dims.dyn0_word0 + outside], got[chosen][:, dims.dyn1_word0 + outside]], axis=1)
    assert not rest.any(), f"{ctx}: a slot outside the level's six is not zero after the reset"


# ---------------------------------------------------------------------------------------------------------------------------
# host-backed stand-ins: the *Bufs classes over plain arrays
# ---------------------------------------------------------------------------------------------------------------------------

class HostBuffer:
    """what `alloc` returns, on the host"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.data = np.zeros(self.shape, self.dtype)

    def from_host(self, arr):
        self.data[...] = np.asarray(arr, dtype=self.dtype).reshape(self.shape)

    def to_host(self):
        return self.data.copy()


class HostEnv:
    """the attributes of a CookingVecEnv the *Bufs classes read, over device-free tables"""

    def __init__(self, tables):
        self.tables, self.dims, self.num_agents, self.F = tables, tables.dims, tables.num_agents, tables.F
        self.num_actions = effects.num_actions(tables.scheme_class.CODE)

    def alloc(self, shape, dtype):
        return HostBuffer(shape, dtype)

    def frame_shape(self, P):
        return (self.dims.H * int(P), self.dims.W * int(P), 3)


def put(buf, body):
    """write `body` to the front of a guarded buffer, as a kernel would, and leave the guard behind it alone"""
    flat = np.ascontiguousarray(body).reshape(-1)
    buf.data[:flat.size] = flat.view(buf.dtype) if flat.dtype.itemsize == buf.dtype.itemsize else flat.astype(buf.dtype)
