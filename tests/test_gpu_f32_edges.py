"""GPU: the float32 observation rows (k_step<..., STEP_F32>, k_observe_f32) where tests/test_gpu_f32_obs.py does not reach them:
  a. all three store flavours of the 16-byte row stores (CZ_WT = 0 plain, 1 write-through, 2 streaming; a batch picks 0 or 2 only
     above 10 240 envs), on rows that start 4-byte aligned (F = 283, 639), with one, three and five rounds of 256 features;
  b. batches that do not fill their last workgroup (8 envs per workgroup, 4 on the huge instance): the waves past N stage the
     float32 table and leave after the barrier; and one-env windows of cz_observe_device_f32 at either end of the batch;
  c. row tails on the small instance: F = 384 | 385 | 512 | 513 | 515 (F mod 4 = 0, 1, 3; a row that ends exactly on a round, a last
     round of one and of three features), with one layout - the b128 descriptor load of a row's last lanes runs off the table - and
     with envs on the first and the last layout of a pool of three; the same F through the compact form, whose padding arithmetic
     has the same residues;
  d. every kernel instance at its capacity edge (coop_test padded to D = 64 | 65 | 128 | 129 | 255; dense_8x8 with 1-4 agents);
  e. deep states: 200 steps under the state-aware policy, with the transitions counted from the oracle's records;
  f. null reward / flag pointers (the handle's scratch row);
  g. three shards of unequal size.
Every comparison of rows is uint32 == uint32 against np.float32 of the oracle's float64 rows; rewards as uint64, flags and records
as bytes.  Every float32 buffer is filled with a NaN sentinel before each launch and carries a guard region behind its last row
(test_gpu_f32_obs.GuardedRows): a feature left unwritten, or a store past a row, shows.

Sensitivity: a float32 row can only tell round-to-nearest-even from another conversion where the float64 feature is not a float32
already.  a, b, c and e therefore assert on the EXPECTED rows that at least 5 % of the compared elements are inexact in float32
(coop_test: 27 %, crowded_6x5: 34 %, huge_20x20: 51 % - the normalised positions k / (W - 1), k / (H - 1) of these grids; on
edge_8x8 and large_16x16 every feature is a multiple of 1 / 8 or 1 / 16 and the share is zero)."""
import functools
import os

import numpy as np
import pytest

from cooking_zoo_amd import soa
from fuzz_policy import BumperActions, EventCounter
from oracle_binding import VecOracle
from vec_common import (CROWDED4, DENSE_RECIPES, HUGE3, PADDED, SENTINEL, TWO, GuardedRows, Sensitivity, bits, instance, junk, make_env,
                        one_world_trajectory, policy, run_compact, strip, want32, widen)

pytestmark = pytest.mark.gpu

make = functools.partial(make_env, max_steps=40)
CORE_EVENTS = ["pick_up", "put_down", "chop", "plate_add", "static_accepts", "delivery", "marks_changed", "truncation"]


class Outs32:
    """the buffers of cz_step_device_f32 (None for those in `skip`); step() fills all of them with sentinel / 0xFF bytes first"""

    def __init__(self, env, skip=()):
        n, A = env.num_envs, env.num_agents
        spec = dict(rew=((n, A), np.float64), term=((n, A), np.uint8), trunc=((n, A), np.uint8))
        self.act, self.rows = env.alloc((n, A), np.int32), GuardedRows(env)
        self.buf = {k: None if k in skip else env.alloc(s, t) for k, (s, t) in spec.items()}
        self.junk = {k: junk(s, t) for k, (s, t) in spec.items()}

    def step(self, env, acts):
        self.rows.fill()
        for k, b in self.buf.items():
            if b is not None:
                b.from_host(self.junk[k])
        self.act.from_host(acts)
        b = self.buf
        env.step_device_f32(self.act, self.rows, b["rew"], b["term"], b["trunc"])
        env.sync()
        return (self.rows.rows(),) + tuple(None if b[k] is None else b[k].to_host() for k in ("rew", "term", "trunc"))


def check32(ctx, got, want):
    """got: (uint32 rows, rewards, terminations, truncations), None where not asked for; want: the oracle's float64 forms"""
    rows, rew, term, trunc = got
    bad = np.argwhere(rows != want32(want[0]))
    assert not len(bad), f"{ctx}: float32 rows differ at (env, agent, feature) {bad[:6].tolist()}" \
                         f"{' - sentinel left' if (rows == SENTINEL).any() else ''}"
    if rew is not None:
        assert np.array_equal(bits(rew), bits(want[1])), f"{ctx}: rewards"
    if term is not None:
        assert np.array_equal(term, want[2]), f"{ctx}: terminations"
    if trunc is not None:
        assert np.array_equal(trunc, want[3]), f"{ctx}: truncations"


def first_observation(env, orc, sens=None):
    """reset both; the first observation through cz_observe_device_f32 is the oracle's"""
    env.reset(return_obs=False)
    first = orc.reset()
    rows = GuardedRows(env)
    env.observe_device(d_obs32=rows)
    env.sync()
    assert np.array_equal(rows.rows(), want32(first)), "first observation"
    assert np.array_equal(strip(env.get_state()), orc.records), "records after reset"
    if sens is not None:
        sens.add(first)
    rows.buf.free()


# ---------------------------------------------------------------------------------------------------------------------------
# a. store flavours
# ---------------------------------------------------------------------------------------------------------------------------

FLAVOUR_LEVELS = [
    # level, meta, agents, recipes, scheme, F, instance, sensitive
    ("coop_test", "example_odd", 2, TWO, "scheme3", 283, 0, True),          # every second row starts 4-byte aligned; two rounds
    ("crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1", None, 0, True),   # one round
    ("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", 639, 2, True),         # odd, three rounds, 4 envs per workgroup
    # (dense_16x16 is here for the large instance and its five rounds.  It is exempt from the sensitivity condition: none of its
    # expected elements is inexact in float32 - the three levels above carry the rounding)
    ("dense_16x16", "dense_16x16", 2, TWO, "scheme3", None, 1, False),
]


@pytest.mark.parametrize("wt", [0, 1, 2])
@pytest.mark.parametrize("level,meta,agents,recipes,scheme,F,inst,sensitive", FLAVOUR_LEVELS, ids=[c[0] for c in FLAVOUR_LEVELS])
def test_store_flavours(wt, level, meta, agents, recipes, scheme, F, inst, sensitive):
    n, T = 77, 30
    os.environ["CZ_WT"] = str(wt)
    try:
        env = make(n, level, meta, agents, recipes, scheme, max_steps=20, num_layouts=6)
    finally:
        del os.environ["CZ_WT"]
    assert instance(env) == inst and (F is None or env.F == F)
    if level == "crowded_6x5":
        assert env.F <= 256
    if level == "dense_16x16":
        assert 1024 < env.F <= 1280
    orc = VecOracle.from_vec_env(env)
    sens = Sensitivity()
    first_observation(env, orc, sens)
    o = Outs32(env)
    rng = np.random.default_rng(23 + wt)
    for t in range(T):
        acts = rng.integers(0, env.n_actions, size=(n, agents), dtype=np.int32)
        got = o.step(env, acts)
        want = orc.step(acts)
        sens.add(want[0])
        check32(f"wt={wt} {level} step {t}", got, want)
    assert np.array_equal(strip(env.get_state()), orc.records)
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 1              # reset passes were encoded
    if sensitive:
        sens.check(level)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# b. partial last workgroup, one-env windows
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level,meta,agents,recipes,scheme,n", [
    ("coop_test", "example", 2, TWO, "scheme3", 1), ("coop_test", "example", 2, TWO, "scheme3", 7),
    ("coop_test", "example", 2, TWO, "scheme3", 9), ("coop_test", "example", 2, TWO, "scheme3", 13),
    ("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", 1), ("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", 5),
    ("crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1", 3),
])
def test_partial_workgroups_and_one_env_windows(level, meta, agents, recipes, scheme, n):
    T = 25
    env = make(n, level, meta, agents, recipes, scheme, max_steps=10)
    orc = VecOracle.from_vec_env(env)
    sens = Sensitivity()
    first_observation(env, orc, sens)
    o = Outs32(env)
    rng = np.random.default_rng(100 + n)
    for t in range(T):
        acts = rng.integers(0, env.n_actions, size=(n, agents), dtype=np.int32)
        got = o.step(env, acts)
        want = orc.step(acts)
        sens.add(want[0])
        check32(f"{level} n={n} step {t}", got, want)
    assert np.array_equal(strip(env.get_state()), orc.records)
    one = GuardedRows(env, 1)
    for begin in (n - 1, 0):
        one.fill()
        env.observe_device(env_begin=begin, env_count=1, d_obs32=one)
        env.sync()
        assert np.array_equal(one.rows(), want32(want[0][begin:begin + 1])), f"{level} n={n}: window ({begin}, 1)"
    sens.check(level)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# c. row tails on the small instance
# ---------------------------------------------------------------------------------------------------------------------------

TAIL_F = [384, 385, 512, 513, 515]


@pytest.mark.parametrize("num_layouts", [1, 3])
@pytest.mark.parametrize("F", TAIL_F)
def test_row_tails(F, num_layouts):
    n, T = 20, 30
    env = make(n, meta=f"example_f{F}", max_steps=12, num_layouts=num_layouts)
    assert env.F == F and instance(env) == 0
    orc = VecOracle.from_vec_env(env)
    sens = Sensitivity()
    first_observation(env, orc, sens)
    pol = policy(env, 3 * F + num_layouts)
    o = Outs32(env)
    on_first = on_last = 0
    for t in range(T):
        acts = pol.act(orc.records)
        got = o.step(env, acts)
        want = orc.step(acts)
        pol.observe_result(orc.records)
        sens.add(want[0])
        check32(f"F={F} L={num_layouts} step {t}", got, want)
        lay = orc.records[:, soa.W_LAYOUT]
        assert int(lay.max()) < num_layouts
        on_first += int((lay == 0).sum())
        on_last += int((lay == num_layouts - 1).sum())
    assert np.array_equal(strip(env.get_state()), orc.records)
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 1
    # envs sat on the first and on the last layout of the pool at compared steps: the descriptor row whose b128 tail reads into the
    # next layout's row, and the one whose tail reads past the table (out of the load's range: zeros, and every such store dropped)
    assert on_first > 0 and on_last > 0
    sens.check(f"F={F}")
    env.close()


@pytest.mark.parametrize("F", TAIL_F)
def test_row_tails_compact(F):
    """the same feature counts through cz_step_device_compact: padding bytes 255, the decoded rows the oracle's"""
    n, T = 20, 30
    env = make(n, meta=f"example_f{F}", max_steps=12, num_layouts=3)
    assert env.F == F and instance(env) == 0 and env.codes_pitch == (F + 15) // 16 * 16
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    orc.reset()
    pol = policy(env, 5 * F)
    acts, want = [], []
    for t in range(T):
        acts.append(pol.act(orc.records))
        want.append(tuple(x.copy() for x in orc.step(acts[-1])) + (strip(orc.records),))
        pol.observe_result(orc.records)
    run_compact(env, np.stack(acts), want, env.dims)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# d. the kernel instances at their capacity edges (exempt from the sensitivity condition: what d asks is which instance ran and
# that its rows are the natural-D ones; coop_test and dense_8x8 both carry inexact features, but nothing here depends on it)
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def padded_trajectory():
    return one_world_trajectory("scheme3", 32, 120)


@pytest.mark.parametrize("max_dyn,inst", PADDED)
def test_one_world_on_every_instance_f32(max_dyn, inst):
    n = 32
    dn, obs0, rec0, acts, want, episodes = padded_trajectory()
    assert episodes >= 2
    env = make(n, scheme="scheme3", max_dyn=max_dyn)
    assert env.dims.D == (max_dyn or 12) and instance(env) == inst
    env.reset(return_obs=False)
    rows = GuardedRows(env)
    env.observe_device(d_obs32=rows)
    env.sync()
    assert np.array_equal(rows.rows(), want32(obs0)), f"D={max_dyn}: reset observation"
    assert np.array_equal(strip(env.get_state()), widen(rec0, dn, env.dims)), f"D={max_dyn}: reset records"
    o = Outs32(env)
    for t, a in enumerate(acts):
        ctx = f"D={env.dims.D} cz_step_device_f32 step {t}"
        check32(ctx, o.step(env, a), want[t])
        assert np.array_equal(strip(env.get_state()), widen(want[t][4], dn, env.dims)), f"{ctx}: records"
    assert instance(env) == inst
    env.close()


@pytest.mark.parametrize("scheme", ["scheme3", "scheme1"])
@pytest.mark.parametrize("agents", [1, 2, 3, 4])
def test_dense_8x8_f32(agents, scheme):
    n, T = 32, 150
    env = make(n, "dense_8x8", "dense_8x8", agents, DENSE_RECIPES[:agents], scheme, max_steps=70)
    assert (env.dims.W * env.dims.H, env.dims.D, env.F) == (64, 64, 466) and instance(env) == 0
    orc = VecOracle.from_vec_env(env)
    first_observation(env, orc)
    pol = policy(env, 60 + 2 * agents + (scheme == "scheme1"))
    o = Outs32(env)
    for t in range(T):
        acts = pol.act(orc.records)
        got = o.step(env, acts)
        check32(f"step {t}", got, orc.step(acts))
        pol.observe_result(orc.records)
        assert np.array_equal(strip(env.get_state()), orc.records), f"step {t}: records"
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 2
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# e. deep states
# ---------------------------------------------------------------------------------------------------------------------------

DEEP_N, DEEP_T, DEEP_MAX_STEPS = 96, 200, 70
DEEP_CASES = {
    "coop_test": (("coop_test", "example", 2, TWO, "scheme3"), 11),
    "crowded_6x5": (("crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1"), 12),
}


def deep_tables(name):
    """the host half of a deep case (no device)"""
    from cooking_zoo_amd.vec_env import BatchTables
    (level, meta, agents, recipes, scheme), seed = DEEP_CASES[name]
    return BatchTables(DEEP_N, level, meta, agents, DEEP_MAX_STEPS, recipes, action_scheme=scheme, num_layouts=8), seed


@functools.lru_cache(maxsize=None)
def deep_actions(name):
    """host only: the policy's actions [T][n][A] over the oracle, and the transitions they reach"""
    tables, seed = deep_tables(name)
    orc = VecOracle.from_vec_env(tables)
    orc.reset()
    pol = BumperActions(tables.dims, tables.scheme_class.CODE, np.random.default_rng(seed))
    ev = EventCounter(tables.dims)
    acts = np.empty((DEEP_T, DEEP_N, tables.num_agents), np.int32)
    for t in range(DEEP_T):
        before = orc.records.copy()
        acts[t] = pol.act(before)
        _, _, term, trunc = orc.step(acts[t], want_obs=False)
        pol.observe_result(orc.records)
        ev.update(before, orc.records, term, trunc)
    return acts, dict(ev.counts)


def test_deep_cases_reach_the_core_events():
    """(host only, but it belongs to the GPU cases below) the two trajectories together plate, deliver, complete and truncate"""
    total = {k: sum(deep_actions(name)[1][k] for name in DEEP_CASES) for k in CORE_EVENTS}
    assert all(v > 0 for v in total.values()), total


@pytest.mark.parametrize("name", list(DEEP_CASES))
def test_deep_states(name):
    acts, _ = deep_actions(name)
    total = {k: sum(deep_actions(c)[1][k] for c in DEEP_CASES) for k in CORE_EVENTS}
    assert all(v > 0 for v in total.values()), total
    (level, meta, agents, recipes, scheme), _ = DEEP_CASES[name]
    env = make(DEEP_N, level, meta, agents, recipes, scheme, max_steps=DEEP_MAX_STEPS)
    orc = VecOracle.from_vec_env(env)
    sens = Sensitivity()
    first_observation(env, orc, sens)
    o = Outs32(env)
    ev = EventCounter(env.dims)
    for t in range(DEEP_T):
        before = orc.records.copy()
        got = o.step(env, acts[t])
        want = orc.step(acts[t])
        ev.update(before, orc.records, want[2], want[3])
        sens.add(want[0])
        check32(f"{name} step {t}", got, want)
        assert np.array_equal(strip(env.get_state()), orc.records), f"{name} step {t}: records"
    assert dict(ev.counts) == deep_actions(name)[1]                   # the run compared is the run that was counted
    sens.check(name)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# f. null outputs
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [("rew", "term", "trunc"), ("rew",), ("term",), ("trunc",)])
def test_null_outputs(skip):
    """null rewards / terminations / truncations with a float32 launch: those stores go to the handle's scratch row; the rows, what
    was asked for, and the records are the oracle's"""
    n, T = 48, 40
    env = make(n, max_steps=25)
    orc = VecOracle.from_vec_env(env)
    first_observation(env, orc)
    pol = policy(env, 9 + len(skip[0]) + len(skip))
    o = Outs32(env, skip=skip)
    for t in range(T):
        acts = pol.act(orc.records)
        got = o.step(env, acts)
        assert all(got[1 + k] is None for k, name in enumerate(("rew", "term", "trunc")) if name in skip)
        check32(f"null {skip} step {t}", got, orc.step(acts))
        pol.observe_result(orc.records)
        assert np.array_equal(strip(env.get_state()), orc.records), f"step {t}: records"
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 1
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# g. shards of unequal size
# ---------------------------------------------------------------------------------------------------------------------------

def test_three_unequal_shards_equal_one_handle():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n, A, T = 13, 2, 30
    one = make(n, max_steps=12)
    three = ShardedVecEnv(n, "coop_test", "example", A, 12, TWO, device_ids=[0, 0, 0], action_scheme="scheme3", num_layouts=8,
                          auto_reset=True)
    sizes = [s.num_envs for s in three.shards]
    assert sum(sizes) == n and len(set(sizes)) > 1, sizes
    orc = VecOracle.from_vec_env(one)
    F = one.F
    fill = np.full((n, A, F), SENTINEL, np.uint32)
    o_act, o_rows = one.alloc((n, A), np.int32), GuardedRows(one)
    o_out = [one.alloc((n, A), np.float64), one.alloc((n, A), np.uint8), one.alloc((n, A), np.uint8)]
    s_act, s_rows = three.alloc((A,), np.int32), three.alloc((A, F), np.uint32)
    s_out = [three.alloc((A,), np.float64), three.alloc((A,), np.uint8), three.alloc((A,), np.uint8)]
    one.reset(return_obs=False)
    three.reset(return_obs=False)
    first = orc.reset()
    s_rows.from_host(fill)
    one.observe_device(d_obs32=o_rows)
    three.observe_device(d_obs32=s_rows)
    one.sync()
    three.sync()
    assert np.array_equal(o_rows.rows(), want32(first)) and np.array_equal(s_rows.to_host(), want32(first))
    rng = np.random.default_rng(16)
    for t in range(T):
        acts = rng.integers(0, 5, size=(n, A), dtype=np.int32)
        o_act.from_host(acts)
        s_act.from_host(acts)
        o_rows.fill()
        s_rows.from_host(fill)
        if t < T // 2:
            one.step_device_f32(o_act, o_rows, *o_out)
            three.step_device_f32(s_act, s_rows, *s_out)
        else:                                            # the second half through the handle setting
            if t == T // 2:
                one.set_f32_output(o_rows)
                three.set_f32_output(s_rows)
            one.step_device(o_act, None, *o_out)
            three.step_device(s_act, None, *s_out)
        one.sync()
        three.sync()
        oo, ro, to, uo = orc.step(acts)
        assert np.array_equal(o_rows.rows(), want32(oo)) and np.array_equal(s_rows.to_host(), want32(oo)), t
        for got, single, want in zip(s_out, o_out, (ro, to, uo)):
            g, s = got.to_host(), single.to_host()
            assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), t
            assert np.array_equal(bits(g), bits(want)) if g.dtype == np.float64 else np.array_equal(g, want), t
    assert np.array_equal(strip(three.get_state()), orc.records) and np.array_equal(strip(one.get_state()), orc.records)
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 1
    one.close()
    three.close()
