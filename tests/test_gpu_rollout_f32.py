"""GPU: float32 trajectories from the fused rollouts - cz_rollout_f32 (k_step<..., ROLLOUT_F32>, mode 7: the on-device action stream)
and cz_rollout_actions_f32 (k_step<..., ROLLOUT_ACTIONS_F32>, mode 8: the caller's actions) - against the oracle.

Rules of every comparison here: the expected values are the oracle's float64 trajectory; the float32 trajectory compares as uint32
with np.float32 of it, rewards as uint64, flags as bytes, the records after a launch (cz_get_state) word for word.  Every buffer is
filled with a sentinel before each launch (float32 rows: a quiet NaN no table entry equals; rewards: a NaN pattern; flags: 0xA5)
and has one more row than the launch writes: that row is the guard region behind the last row and must come back untouched.

Levels: grids whose width and height are powers of two make every quotient a float32 already, so every level here has another
grid (6 x 5, 7 x 7, 8 x 31, 20 x 20) and every test asserts on the EXPECTED rows that at least 5 % of the compared elements are
inexact in float32.  The matrix needs more than the shipped levels give it in two respects: a pool with at least four layouts whose
descriptor rows differ (crowded_6x5 and limit_8x31 have two or three, huge_20x20 one: their static objects never move), and four
agents on the middle and the huge instance (their meta files stop at three).  `movable_levels` therefore writes, next to the
test's temporary files, a copy of each level in which two static objects draw their cell from a short list, with a fourth agent
entry, and a copy of its meta file with "Agent": 4; everything else is the shipped file.

Shapes: 35 envs (the last workgroup is partly empty at 8 and at 4 envs per workgroup), T = 5 with max_steps = 3, so that an episode
end, the reset pass behind it and a move to another layout fall inside one launch - the descriptor re-fetch of the kernel."""
import json
import os

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from oracle_binding import VecOracle
from host_common import register_fixture_recipes
from vec_common import (CROWDED4, HUGE3, MIN_INEXACT, SENTINEL, TWO, CallerStream, Sensitivity, instance, last_mode, make_env as make, strip,
                        want32)

pytestmark = pytest.mark.gpu

ROLLOUT_F32, ROLLOUT_ACTIONS_F32 = 7, 8                         # StepMode, cz_kernels.h
N, T, MAX_STEPS = 35, 5, 3
NAN64 = 0xFFF8A5A5A5A5A5A5                                      # the rewards' sentinel: a NaN no reward equals
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cooking_zoo_amd", "utils")
# level -> (meta file, instance, {(static class, k-th entry of it): (x candidates, y candidates)}, the fourth agent's spawn area)
MOVABLE = {
    "crowded_6x5": ("crowded_6x5", 0, {("Cutboard", 0): ([0], [2, 3]), ("Blender", 0): ([5], [1, 2])}, None),
    "limit_8x31": ("limits", 1, {("Cutboard", 0): ([0], [2, 5, 9]), ("Blender", 0): ([3, 5], [30])},
                   {"MAX_COUNT": 1, "X_POSITION": [1, 2, 3, 4, 5, 6], "Y_POSITION": list(range(1, 30))}),
    "huge_20x20": ("huge_20x20", 2, {("Cutboard", 0): ([3, 7, 11], [4]), ("Blender", 0): ([0], [8, 12])},
                   {"MAX_COUNT": 1, "X_POSITION": list(range(2, 18)), "Y_POSITION": [6, 7, 11, 12]}),
}


@pytest.fixture(scope="module")
def movable_levels(tmp_path_factory):
    """-> {level: (level file, meta file, instance)}: the copies described in the module's docstring"""
    d, out = tmp_path_factory.mktemp("movable"), {}
    for level, (meta, inst, moves, fourth) in MOVABLE.items():
        lv = json.load(open(os.path.join(PKG, "level", level + ".json")))
        seen = {}
        for entry in lv["STATIC_OBJECTS"]:
            (name, spec), = entry.items()
            k = seen.get(name, 0)
            seen[name] = k + 1
            if (name, k) in moves:
                spec["X_POSITION"], spec["Y_POSITION"] = moves[(name, k)]
        if fourth:
            lv["AGENTS"].append(fourth)
        mt = json.load(open(os.path.join(PKG, "meta_files", meta + ".json")))
        for entry in mt:
            if "Agent" in entry:
                entry["Agent"] = 4
        lp, mp = str(d / (level + "_movable.json")), str(d / (meta + "_4agents.json"))
        json.dump(lv, open(lp, "w"))
        json.dump(mt, open(mp, "w"))
        out[level] = (lp, mp, inst)
    return out


class Traj:
    """the buffers of one fused float32 launch of T steps, each with a guard row behind row T - 1 (None for those in `skip`):
    rows uint32 [T + 1][n][A][F], rew uint64 [T + 1][n][A], term / trunc uint8 [T + 1][n][A], act int32 [T][n][A]"""

    def __init__(self, env, T, skip=(), sharded=False):
        n, A, F = env.num_envs, env.num_agents, env.F
        self.T, self.fillers = T, dict(rows=((A, F), np.uint32, SENTINEL), rew=((A,), np.uint64, NAN64), term=((A,), np.uint8, 0xA5),
                                       trunc=((A,), np.uint8, 0xA5))
        alloc = (lambda per, t, lead: env.alloc(per, t, leading=(lead,))) if sharded else (lambda per, t, lead: env.alloc((lead, n) + per, t))
        self.buf = {k: None if k in skip else alloc(per, t, T + 1) for k, (per, t, _) in self.fillers.items()}
        self.shape = {k: (T + 1, n) + per for k, (per, _, _) in self.fillers.items()}
        self.act = alloc((A,), np.int32, T)

    def fill(self):
        for k, b in self.buf.items():
            if b is not None:
                b.from_host(np.full(self.shape[k], self.fillers[k][2], self.fillers[k][1]))

    def get(self):
        """-> (rows, rewards, terminations, truncations), each [T][n]... or None; asserts every guard row"""
        out = []
        for k in ("rows", "rew", "term", "trunc"):
            if self.buf[k] is None:
                out.append(None)
                continue
            got = self.buf[k].to_host()
            assert (got[self.T] == self.fillers[k][2]).all(), f"{k}: a store went past the last row of the trajectory"
            out.append(got[:self.T])
        return tuple(out)

    def rollout(self, env, seed, step0):
        self.fill()
        b = self.buf
        env.rollout_f32(self.T, seed, step0, b["rows"], b["rew"], b["term"], b["trunc"])
        env.sync()
        return self.get()

    def rollout_actions(self, env, acts):
        self.fill()
        self.act.from_host(acts)
        b = self.buf
        env.rollout_actions_f32(self.act, self.T, b["rows"], b["rew"], b["term"], b["trunc"])
        env.sync()
        return self.get()


def expected(orc, T, seed=None, step0=0, acts=None, sens=None):
    """the oracle walks T steps - over the on-device stream of (seed, step0), or over `acts` - -> (actions [T][n][A], per step
    (observation, rewards, terminations, truncations, records))"""
    if acts is None:
        err, _, _, _, _, acts = orc.oracle.rollout(orc.records.copy(), T, seed, step0, want_obs=False, want_actions=True)
        assert err == 0
    wants = []
    for t in range(T):
        wants.append(tuple(x.copy() for x in orc.step(acts[t])) + (orc.records.copy(),))
        if sens is not None:
            sens.add(wants[-1][0])
    return np.ascontiguousarray(acts, dtype=np.int32), wants


def check(ctx, got, wants):
    rows, rew, term, trunc = got
    for t, want in enumerate(wants):
        bad = np.argwhere(rows[t] != want32(want[0]))
        assert not len(bad), f"{ctx} step {t}: float32 rows differ at (env, agent, feature) {bad[:6].tolist()}" \
                             f"{' - sentinel left' if (rows[t] == SENTINEL).any() else ''}"
        if rew is not None:
            assert np.array_equal(rew[t], want[1].view(np.uint64)), f"{ctx} step {t}: rewards"
        if term is not None:
            assert np.array_equal(term[t], want[2]), f"{ctx} step {t}: terminations"
        if trunc is not None:
            assert np.array_equal(trunc[t], want[3]), f"{ctx} step {t}: truncations"


def start(env, orc):
    env.reset(return_obs=False)
    orc.reset()
    assert np.array_equal(strip(env.get_state()), orc.records), "records after reset"


def random_actions(env, T, seed):
    return np.random.default_rng(seed).integers(0, env.n_actions, size=(T, env.num_envs, env.num_agents), dtype=np.int32)


def both_modes(ctx, env, orc, tr, seed, sens=None, step0=0):
    """one launch of each mode on the same handle, one behind the other, each against the oracle (trajectory, rewards, flags, records)"""
    _, wants = expected(orc, tr.T, seed, step0, sens=sens)
    got = tr.rollout(env, seed, step0)
    assert last_mode(env) == ROLLOUT_F32
    check(f"{ctx} cz_rollout_f32", got, wants)
    assert np.array_equal(strip(env.get_state()), wants[-1][4]), f"{ctx} cz_rollout_f32: records"
    acts, wants2 = expected(orc, tr.T, acts=random_actions(env, tr.T, seed + 1), sens=sens)
    got = tr.rollout_actions(env, acts)
    assert last_mode(env) == ROLLOUT_ACTIONS_F32
    check(f"{ctx} cz_rollout_actions_f32", got, wants2)
    assert np.array_equal(strip(env.get_state()), wants2[-1][4]), f"{ctx} cz_rollout_actions_f32: records"
    return wants + wants2


# ---------------------------------------------------------------------------------------------------------------------------
# the matrix: every (instance, agents, scheme) cell, both modes
# ---------------------------------------------------------------------------------------------------------------------------

CELLS = [(level, agents, scheme) for level in MOVABLE for agents in (1, 2, 3, 4) for scheme in ("scheme1", "scheme3")]


@pytest.mark.parametrize("level,agents,scheme", CELLS, ids=[f"{l}-{a}agents-{s}" for l, a, s in CELLS])
def test_every_cell_both_modes(movable_levels, level, agents, scheme):
    lp, mp, inst = movable_levels[level]
    env = make(N, lp, mp, agents, CROWDED4[:agents], scheme, max_steps=MAX_STEPS, num_layouts=16)
    try:
        assert instance(env) == inst and last_mode(env) == -1
        desc = np.stack([l.obs_descriptor(env.meta, env.dims) for l in env.layouts])
        assert len({row.tobytes() for row in desc}) >= 4, "the pool needs at least four layouts whose descriptors differ"
        orc = VecOracle.from_vec_env(env)
        start(env, orc)
        sens = Sensitivity()
        first = orc.records[:, soa.W_LAYOUT].copy()
        wants = both_modes(f"{level} {agents} agents {scheme}", env, orc, Traj(env, T), 300 + agents, sens)
        # inside each launch envs finished an episode, took the reset pass and came out on a layout with another descriptor row
        for k, launch in enumerate((wants[:T], wants[T:])):
            before = first if k == 0 else wants[T - 1][4][:, soa.W_LAYOUT]
            moved = 0
            for want in launch:
                after = want[4][:, soa.W_LAYOUT]
                moved += int((desc[after] != desc[before]).any(axis=1).sum())
                before = after
            assert moved >= 5, f"launch {k}: only {moved} envs moved to a layout with another descriptor row"
        assert int(orc.records[:, soa.W_EPISODE].min()) >= 2
        sens.check(level)
    finally:
        env.close()


def test_the_chosen_levels_are_sensitive_to_the_rounding(movable_levels):
    """(the oracle alone) every level the cases below use has at least 5 % of its features inexact in float32"""
    from cooking_zoo_amd.vec_env import BatchTables
    cases = [(lp, mp, 3, CROWDED4[:3], "scheme1") for lp, mp, _ in movable_levels.values()]
    cases += [("coop_test", "example_odd", 2, TWO, "scheme3"), ("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1"),
              ("crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1")]
    for level, meta, agents, recipes, scheme in cases:
        tables = BatchTables(N, level, meta, agents, MAX_STEPS, recipes, action_scheme=scheme, num_layouts=8)
        orc = VecOracle.from_vec_env(tables)
        sens = Sensitivity()
        sens.add(orc.reset())
        expected(orc, T, 1, 0, sens=sens)
        assert sens.inexact >= MIN_INEXACT * sens.total, (level, sens.inexact, sens.total)


# ---------------------------------------------------------------------------------------------------------------------------
# T edges
# ---------------------------------------------------------------------------------------------------------------------------

def crowded(n=N, **kw):
    args = dict(max_steps=MAX_STEPS)
    args.update(kw)
    return make(n, "crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1", **args)


def test_one_step_launches():
    env = crowded()
    orc = VecOracle.from_vec_env(env)
    start(env, orc)
    tr, sens = Traj(env, 1), Sensitivity()
    for k in range(4):                                            # (the fourth step of each mode is a reset pass)
        both_modes(f"T = 1, launch {k}", env, orc, tr, 40, sens, step0=k)
    sens.check("T = 1")
    env.close()


@pytest.mark.parametrize("mode", [ROLLOUT_F32, ROLLOUT_ACTIONS_F32])
def test_three_then_four_steps_equal_seven(mode):
    """T = 3 followed by T = 4 with step0 advanced == T = 7 in one launch: trajectory, state and statistics; and both the oracle's"""
    split, whole = crowded(), crowded()
    orc = VecOracle.from_vec_env(split)
    start(split, orc)
    whole.reset(return_obs=False)
    sens = Sensitivity()
    seed = 77
    if mode == ROLLOUT_F32:
        acts, wants = expected(orc, 7, seed, 0, sens=sens)
    else:
        acts, wants = expected(orc, 7, acts=random_actions(split, 7, seed), sens=sens)
    t3, t4, t7 = Traj(split, 3), Traj(split, 4), Traj(whole, 7)
    if mode == ROLLOUT_F32:
        a, b, c = t3.rollout(split, seed, 0), t4.rollout(split, seed, 3), t7.rollout(whole, seed, 0)
    else:
        a, b, c = t3.rollout_actions(split, acts[:3]), t4.rollout_actions(split, acts[3:]), t7.rollout_actions(whole, acts)
    assert last_mode(split) == mode == last_mode(whole)
    check("T = 7", c, wants)
    for x, y, z, what in zip(a, b, c, ("rows", "rewards", "terminations", "truncations")):
        assert np.array_equal(np.concatenate([x, y]), z), f"3 + 4 steps against 7: {what}"
    assert np.array_equal(split.get_state(), whole.get_state()), "3 + 4 steps against 7: records"
    assert np.array_equal(strip(whole.get_state()), wants[-1][4])
    assert split.stats() == whole.stats() and whole.stats()["episodes"] >= N
    sens.check("T = 7")
    split.close()
    whole.close()


# ---------------------------------------------------------------------------------------------------------------------------
# against the one-step kernel, and the state left behind
# ---------------------------------------------------------------------------------------------------------------------------

def test_rollout_actions_f32_is_t_calls_of_step_device_f32():
    fused, single = crowded(), crowded()
    orc = VecOracle.from_vec_env(fused)
    start(fused, orc)
    single.reset(return_obs=False)
    T_ = 9
    sens = Sensitivity()
    acts, wants = expected(orc, T_, acts=random_actions(fused, T_, 5), sens=sens)
    tr = Traj(fused, T_)
    got = tr.rollout_actions(fused, acts)
    check("cz_rollout_actions_f32", got, wants)
    one = Traj(single, 1)
    d_act = single.alloc((N, 4), np.int32)
    for t in range(T_):
        one.fill()
        d_act.from_host(acts[t])
        b = one.buf
        single.step_device_f32(d_act, b["rows"], b["rew"], b["term"], b["trunc"])
        single.sync()
        for x, y, what in zip(one.get(), got, ("rows", "rewards", "terminations", "truncations")):
            assert np.array_equal(x[0], y[t]), f"row {t}: {what} of cz_step_device_f32 differ from the fused launch's"
    assert np.array_equal(single.get_state(), fused.get_state()) and single.stats() == fused.stats()
    sens.check("cz_rollout_actions_f32")
    fused.close()
    single.close()


def test_state_and_statistics_are_those_of_cz_rollout():
    env, twin = crowded(), crowded()
    orc = VecOracle.from_vec_env(env)
    start(env, orc)
    twin.reset(return_obs=False)
    T_, seed, step0 = 11, 9, 4
    _, wants = expected(orc, T_, seed, step0)
    tr = Traj(env, T_)
    got = tr.rollout(env, seed, step0)
    check("cz_rollout_f32", got, wants)
    spec = [((T_, N, 4, env.F), np.float64), ((T_, N, 4), np.uint64), ((T_, N, 4), np.uint8), ((T_, N, 4), np.uint8)]
    d = [twin.alloc(s, t) for s, t in spec]
    twin.rollout(T_, seed, step0, *d)
    twin.sync()
    assert last_mode(twin) == 1 and last_mode(env) == ROLLOUT_F32
    assert np.array_equal(env.get_state(), twin.get_state()), "records (running returns included)"
    assert env.stats() == twin.stats() and env.stats()["episodes"] >= 2 * N
    assert np.array_equal(got[0], want32(d[0].to_host()))
    for x, y in zip(got[1:], d[1:]):
        assert np.array_equal(x, y.to_host())
    env.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# row tails and rounds, store flavours
# ---------------------------------------------------------------------------------------------------------------------------

TAILS = [("coop_test", "example_odd", 2, TWO, "scheme3", 283, 0)] + \
        [("coop_test", f"example_f{F}", 2, TWO, "scheme3", F, 0) for F in (384, 385, 512, 513, 515)] + \
        [("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", 639, 2)]


def tails_case(case, wt=None):
    level, meta, agents, recipes, scheme, F, inst = case
    n, layouts = 20, 3
    if wt is not None:
        os.environ["CZ_WT"] = str(wt)
    try:
        env = make(n, level, meta, agents, recipes, scheme, max_steps=4, num_layouts=layouts)
    finally:
        os.environ.pop("CZ_WT", None)
    assert env.F == F and instance(env) == inst
    orc = VecOracle.from_vec_env(env)
    start(env, orc)
    sens = Sensitivity()
    wants = both_modes(f"F = {F} wt = {wt}", env, orc, Traj(env, 6), 3 * F, sens)
    lay = np.stack([w[4][:, soa.W_LAYOUT] for w in wants])
    # envs sat on the first and on the last layout of the pool at compared steps: the descriptor row whose b128 tail reads into the
    # next layout's row, and the one whose tail reads past the table (out of the load's range: zeros, and every such store dropped)
    assert int(lay.max()) == layouts - 1 and (lay == 0).any()
    sens.check(f"F = {F}")
    env.close()


@pytest.mark.parametrize("case", TAILS, ids=[f"F{c[5]}" for c in TAILS])
def test_row_tails_and_rounds(case):
    tails_case(case)


@pytest.mark.parametrize("wt", [0, 1, 2])
def test_store_flavours(wt):
    tails_case(TAILS[0], wt)


# ---------------------------------------------------------------------------------------------------------------------------
# null outputs
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [(), ("rew",), ("term",), ("trunc",), ("rew", "term"), ("rew", "trunc"), ("term", "trunc"), ("rew", "term", "trunc")],
                         ids=lambda s: "no-" + "-".join(s) if s else "all")
def test_null_outputs(skip):
    env = crowded()
    orc = VecOracle.from_vec_env(env)
    start(env, orc)
    tr = Traj(env, T, skip=skip)
    assert all((tr.buf[k] is None) == (k in skip) for k in ("rew", "term", "trunc"))
    both_modes(f"without {skip}", env, orc, tr, 60 + len(skip))
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# wide recipe tables with despawn / respawn, one cell per instance
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_dyn,inst,agents,scheme", [(None, 0, 4, "scheme3"), (65, 1, 3, "scheme1"), (129, 2, 4, "scheme1")])
def test_wide_books_and_spawning(max_dyn, inst, agents, scheme):
    from cooking_zoo_amd.cooking_book import recipe_drawer as rd
    assert not rd.RECIPE_STORE
    register_fixture_recipes()
    try:
        env = make(N, "crowded_6x5", "crowded_6x5", agents, ["FruitFeast", "PickyBanana", "BreadSnack", "FruitFeast"][:agents], scheme,
                   max_steps=9, max_dyn=max_dyn, agent_despawn_rate=0.1, agent_respawn_rate=0.3, grace_period=2, spawn_seed=5)
        assert instance(env) == inst and env.recipe_nodes == 16
        orc = VecOracle.from_vec_env(env)
        start(env, orc)
        sens = Sensitivity()
        before = orc.records.copy()
        wants = both_modes(f"wide, spawning, instance {inst}", env, orc, Traj(env, 12), 500 + inst, sens)
        despawns = respawns = 0
        for want in wants:
            after = want[4]
            same = after[:, soa.W_EPISODE] == before[:, soa.W_EPISODE]
            gone0, gone1 = (before[:, soa.W_STATUS] >> 8) & 0xF, (after[:, soa.W_STATUS] >> 8) & 0xF
            despawns += int(np.count_nonzero((gone1 & ~gone0)[same]))
            respawns += int(np.count_nonzero((gone0 & ~gone1)[same]))
            before = after
        assert despawns >= 1 and respawns >= 1, (despawns, respawns)
        sens.check("wide")
        env.close()
    finally:
        rd.RECIPE_STORE.clear()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_step_nothing():
    env = crowded()
    orc = VecOracle.from_vec_env(env)
    start(env, orc)
    tr = Traj(env, T)
    tr.fill()
    b, A = tr.buf, env.num_agents
    state = env.get_state()
    limit = 0xFFFFFFFF // (N * A * 8)                           # begin_device_call: T * num_envs * num_agents * 8 must stay below 4 GiB
    assert limit + 1 < 2 ** 31
    calls = [
        ("float32 trajectory pointer", lambda: env.rollout_f32(T, 1, 0, None, b["rew"], b["term"], b["trunc"])),
        ("float32 trajectory", lambda: env.rollout_actions_f32(tr.act, T, None, b["rew"], b["term"], b["trunc"])),
        ("T must be >= 1", lambda: env.rollout_f32(0, 1, 0, b["rows"], b["rew"], b["term"], b["trunc"])),
        ("T must be >= 1", lambda: env.rollout_f32(-3, 1, 0, b["rows"], b["rew"], b["term"], b["trunc"])),
        ("T must be >= 1", lambda: env.rollout_actions_f32(tr.act, 0, b["rows"], b["rew"], b["term"], b["trunc"])),
        (f"T <= {limit} here", lambda: env.rollout_f32(limit + 1, 1, 0, b["rows"], b["rew"], b["term"], b["trunc"])),
        (f"T <= {limit} here", lambda: env.rollout_actions_f32(tr.act, limit + 1, b["rows"], b["rew"], b["term"], b["trunc"])),
    ]
    for message, call in calls:
        with pytest.raises(_native.NativeError, match=message):
            call()
        env.sync()
        assert np.array_equal(env.get_state(), state), f"a refused call ({message}) stepped something"
        for got, (k, (_, _, filler)) in zip(tr.get(), tr.fillers.items()):
            assert (got == filler).all(), f"a refused call ({message}) wrote {k}"
    both_modes("after the refusals", env, orc, tr, 8)            # the next valid calls work
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# inside a capture of the caller
# ---------------------------------------------------------------------------------------------------------------------------

def test_both_launches_captured_into_a_callers_graph():
    env, ref = crowded(), crowded()
    orc = VecOracle.from_vec_env(env)
    start(env, orc)
    ref.reset(return_obs=False)
    seed = 31
    _, wants_a = expected(orc, T, seed, 0)
    acts, wants_b = expected(orc, T, acts=random_actions(env, T, 32))
    ta, tb, ra, rb = Traj(env, T), Traj(env, T), Traj(ref, T), Traj(ref, T)
    for x in (ta, tb):
        x.fill()
    tb.act.from_host(acts)
    cs = CallerStream(env)
    with cs.capture():
        env.rollout_f32(T, seed, 0, ta.buf["rows"], ta.buf["rew"], ta.buf["term"], ta.buf["trunc"])
        env.rollout_actions_f32(tb.act, T, tb.buf["rows"], tb.buf["rew"], tb.buf["term"], tb.buf["trunc"])
    assert (env.get_state()[:, soa.W_T] == 0).all(), "capturing must not have stepped anything"
    cs.replay()
    cs.sync()
    eager_a, eager_b = ra.rollout(ref, seed, 0), rb.rollout_actions(ref, acts)
    got_a, got_b = ta.get(), tb.get()
    check("captured cz_rollout_f32", got_a, wants_a)
    check("captured cz_rollout_actions_f32", got_b, wants_b)
    for got, eager in ((got_a, eager_a), (got_b, eager_b)):
        for x, y in zip(got, eager):
            assert np.array_equal(x, y), "the replayed launch differs from the eager one"
    assert np.array_equal(env.get_state(), ref.get_state()) and env.stats() == ref.stats()
    cs.close()
    env.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# shards of unequal size
# ---------------------------------------------------------------------------------------------------------------------------

def test_three_unequal_shards_equal_one_handle():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n, A = 13, 4
    one = crowded(n)
    three = ShardedVecEnv(n, "crowded_6x5", "crowded_6x5", A, MAX_STEPS, CROWDED4, device_ids=[0, 0, 0], action_scheme="scheme1", num_layouts=8,
                          auto_reset=True)
    assert [s.num_envs for s in three.shards] == [5, 4, 4]
    orc = VecOracle.from_vec_env(one)
    start(one, orc)
    three.reset(return_obs=False)
    sens = Sensitivity()
    to, ts = Traj(one, T), Traj(three, T, sharded=True)
    seed = 19
    _, wants = expected(orc, T, seed, 0, sens=sens)
    acts, wants2 = expected(orc, T, acts=random_actions(one, T, 20), sens=sens)
    for tr, env in ((to, one), (ts, three)):
        check("cz_rollout_f32", tr.rollout(env, seed, 0), wants)
        check("cz_rollout_actions_f32", tr.rollout_actions(env, acts), wants2)
    assert np.array_equal(three.get_state(), one.get_state()) and np.array_equal(strip(one.get_state()), wants2[-1][4])
    sens.check("shards")
    one.close()
    three.close()
