"""GPU: the observation as float32 rows (cz_step_device_f32 / cz_set_f32_output / cz_observe_device_f32): float [N][A][F], dense,
every element np.float32 of the reference's float64 feature (cooking_env.py:352-373; round to nearest even) - compared bit for bit
as uint32 against the oracle's rows on every level family / kernel instance / scheme / agent count, with a sentinel pattern under
the rows and a guard region behind them (a 16-byte store that ran past its row would show), on despawning mixed-level batches and
a wide user book, through ring runs (graph replay and direct launches), with fused ring runs switched on, as the first observation
after reset / set_state, over two shards, and inside a stream capture of the caller."""
import ctypes as C

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from host_common import register_fixture_recipes
from vec_common import GUARD, OBS_CASES as CASES, SENTINEL, CallerStream, GuardedRows, bits, make_env as make, strip, want32

pytestmark = pytest.mark.gpu

def test_the_cases_are_the_thirteen_of_the_compact_test():
    assert len(CASES) == 13 and any(c[4] == "example_odd" for c in CASES)


@pytest.mark.parametrize("scheme,level,agents,recipes,meta", CASES)
def test_float32_rows_are_the_rounded_oracle_observation(scheme, level, agents, recipes, meta):
    from oracle_binding import VecOracle
    n, T = 48, 70
    env, twin = make(n, level, meta, agents, recipes, scheme), make(n, level, meta, agents, recipes, scheme)
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    twin.reset(return_obs=False)
    orc.reset()
    A, F = agents, env.F
    if meta == "example_odd":
        assert F == 283
    t32 = env.obs_table_f32()
    assert t32.dtype == np.float32 and np.array_equal(t32.view(np.uint32), env.obs_table().astype(np.float32).view(np.uint32))
    d_act, rows = env.alloc((n, A), np.int32), GuardedRows(env)
    d_rew, d_t, d_u = env.alloc((n, A), np.float64), env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)
    w_act, w_obs = twin.alloc((n, A), np.int32), twin.alloc((n, A, F), np.float64)
    rng = np.random.default_rng(5)
    for t in range(T):
        acts = rng.integers(0, env.n_actions, size=(n, A), dtype=np.int32)
        d_act.from_host(acts)
        rows.fill()
        env.step_device_f32(d_act, rows, d_rew, d_t, d_u)
        env.sync()
        oo, ro, to, uo = orc.step(acts)
        got = rows.rows()
        assert np.array_equal(got, want32(oo)), f"float32 observation at step {t}"
        assert np.array_equal(bits(d_rew.to_host()), bits(ro)), f"rewards at step {t}"
        assert np.array_equal(d_t.to_host(), to) and np.array_equal(d_u.to_host(), uo), f"flags at step {t}"
        # the twin walks the same trajectory; every third step through float64 rows, checked against the oracle too
        w_act.from_host(acts)
        twin.step_device(w_act, w_obs if t % 3 == 0 else None, None, None, None)
        if t % 3 == 0:
            twin.sync()
            assert np.array_equal(bits(w_obs.to_host()), bits(oo)), f"float64 observation of the twin at step {t}"
            assert np.array_equal(strip(twin.get_state()), orc.records) and np.array_equal(strip(env.get_state()), orc.records), t
    assert np.array_equal(strip(env.get_state()), orc.records)
    assert int(env.get_state()[:, soa.W_EPISODE].min()) >= 1          # reset passes were encoded too
    env.close()
    twin.close()


def test_despawn_respawn_on_a_mixed_level_batch():
    from cooking_zoo_amd.vec_env import CookingVecEnv
    from oracle_binding import VecOracle
    n, A = 96, 2
    kw = dict(action_scheme="scheme3", num_layouts=6, auto_reset=True, agent_despawn_rate=0.12, agent_respawn_rate=0.3, grace_period=3, spawn_seed=21)
    env = CookingVecEnv(n, ["coop_test", "switch_test"], "example", A, 35, ["TomatoSalad", "TomatoSalad"], env_id_base=500, **kw)
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    orc.reset()
    d_act, rows = env.alloc((n, A), np.int32), GuardedRows(env)
    d_rew, d_t, d_u = env.alloc((n, A), np.float64), env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)
    rng = np.random.default_rng(8)
    gone_seen = 0
    for t in range(80):
        acts = rng.integers(0, env.n_actions, size=(n, A), dtype=np.int32)
        d_act.from_host(acts)
        env.step_device_f32(d_act, rows, d_rew, d_t, d_u)
        env.sync()
        oo, ro, to, uo = orc.step(acts)
        assert np.array_equal(rows.rows(), want32(oo)), t
        assert np.array_equal(bits(d_rew.to_host()), bits(ro)) and np.array_equal(d_t.to_host(), to) and np.array_equal(d_u.to_host(), uo), t
        gone_seen += int((((orc.records[:, soa.W_STATUS] >> 8) & 0xF) != 0).sum())
    assert np.array_equal(strip(env.get_state()), orc.records) and gone_seen > 100
    env.close()


def test_wide_user_book():
    """graphs of more than 8 nodes (custom_wide_* recipes: wide tables, marks in record words 1 and 7)"""
    from cooking_zoo_amd.cooking_book import recipe_drawer as rd
    from oracle_binding import VecOracle
    assert not rd.RECIPE_STORE
    register_fixture_recipes()
    try:
        n, A = 64, 2
        env = make(n, "coop_test", "example", A, ["FruitFeast", "PickyBanana"], "scheme3")
        assert env.recipe_nodes == 16
        orc = VecOracle.from_vec_env(env)
        env.reset(return_obs=False)
        orc.reset()
        d_act, rows = env.alloc((n, A), np.int32), GuardedRows(env)
        d_rew, d_t, d_u = env.alloc((n, A), np.float64), env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)
        rng = np.random.default_rng(4)
        for t in range(70):
            acts = rng.integers(0, env.n_actions, size=(n, A), dtype=np.int32)
            d_act.from_host(acts)
            env.step_device_f32(d_act, rows, d_rew, d_t, d_u)
            env.sync()
            oo, ro, to, uo = orc.step(acts)
            assert np.array_equal(rows.rows(), want32(oo)), t
            assert np.array_equal(bits(d_rew.to_host()), bits(ro)) and np.array_equal(d_t.to_host(), to) and np.array_equal(d_u.to_host(), uo), t
        assert np.array_equal(strip(env.get_state()), orc.records)
        env.close()
    finally:
        rd.RECIPE_STORE.clear()


@pytest.mark.parametrize("K,graph", [(60, True), (20, False)])
def test_ring_runs_with_the_float32_output_set_on_the_handle(K, graph):
    """cz_set_f32_output: ring runs - K >= 48: graph replay, K < 48: direct launches - write the float32 rows; switching it off
    restores the float64 kernels, and the graphs captured before a switch are not replayed with a stale pointer"""
    from oracle_binding import VecOracle
    n, A, period = 192, 2, 64
    env = make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=25)
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    orc.reset()
    ring_host = np.random.default_rng(9).integers(0, 5, size=(period, n, A), dtype=np.int32)
    d_ring = env.alloc((period, n, A), np.int32)
    d_ring.from_host(ring_host)
    d_obs, rows, other = env.alloc((n, A, env.F), np.float64), GuardedRows(env), GuardedRows(env)
    outs = [env.alloc((n, A), np.float64), env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)]
    L, h = _native.lib(), env._h
    gk, dk = C.c_int64(), C.c_int64()
    step = 0
    for phase, (f32, obs) in enumerate([(None, d_obs), (rows, None), (other, None), (None, d_obs), (rows, None)]):
        env.set_f32_output(f32)
        rows.fill()
        other.fill()
        _native.check(h, L.cz_launch_counts(h, None, None, 1))
        env.step_device_ring(K, d_ring, n * A, period, 0, obs, *outs)
        env.sync()
        _native.check(h, L.cz_launch_counts(h, C.byref(gk), C.byref(dk), 0))
        assert (gk.value > 0) == graph and gk.value + dk.value == K, (gk.value, dk.value)
        for k in range(K):
            oo, ro, to, uo = orc.step(ring_host[k % period], k == K - 1)
        step += K
        if obs is not None:
            assert np.array_equal(bits(d_obs.to_host()), bits(oo)), phase
            assert (rows.rows() == SENTINEL).all() and (other.rows() == SENTINEL).all(), phase
        else:
            assert np.array_equal(f32.rows(), want32(oo)), phase
            assert ((other if f32 is rows else rows).rows() == SENTINEL).all(), phase
        assert np.array_equal(bits(outs[0].to_host()), bits(ro)) and np.array_equal(outs[2].to_host(), uo), phase
        assert np.array_equal(strip(env.get_state()), orc.records), phase
    env.close()


def test_fused_ring_runs_fall_back_to_one_step_launches():
    """cz_set_ring_fused with the float32 output set: the run goes out as one-step launches - identical results, no fused steps"""
    n, A, period, K = 160, 2, 16, 16
    a, b = (make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=25) for _ in range(2))
    ring_host = np.random.default_rng(3).integers(0, 5, size=(period, n, A), dtype=np.int32)
    res = []
    for env, fused in ((a, True), (b, False)):
        env.reset(return_obs=False)
        d_ring = env.alloc((period, n, A), np.int32)
        d_ring.from_host(ring_host)
        rows = GuardedRows(env)
        outs = [env.alloc((n, A), np.float64), env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)]
        env.set_ring_fused(fused)
        env.set_f32_output(rows)
        for _ in range(3):
            env.step_device_ring(K, d_ring, n * A, period, 0, None, *outs)
        env.sync()
        assert env.ring_fused_steps() == 0
        res.append((rows.rows(), [o.to_host() for o in outs], strip(env.get_state())))
        # ... and with the setting off the same call is fused again
        env.set_f32_output(None)
        env.step_device_ring(K, d_ring, n * A, period, 0, None, *outs)
        env.sync()
        assert env.ring_fused_steps() == (K if fused else 0)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][2], res[1][2])
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(res[0][1], res[1][1]))
    a.close()
    b.close()


@pytest.mark.parametrize("scheme,level,agents,recipes,meta", [CASES[0], CASES[1], CASES[4], CASES[6], CASES[-1]])
def test_first_observation_as_float32_after_reset_and_set_state(scheme, level, agents, recipes, meta):
    from oracle_binding import VecOracle
    n = 96
    env = make(n, level, meta, agents, recipes, scheme)
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    first = orc.reset()
    rows = GuardedRows(env)
    env.observe_device(d_obs32=rows)
    env.sync()
    assert np.array_equal(rows.rows(), want32(first))
    rng = np.random.default_rng(1)
    for _ in range(12):
        acts = rng.integers(0, env.n_actions, size=(n, agents), dtype=np.int32)
        oo, *_ = orc.step(acts)
    env.set_state(orc.records)
    part = GuardedRows(env, 40)
    d_obs = env.alloc((40, agents, env.F), np.float64)
    env.observe_device(d_obs, None, env_begin=17, env_count=40, d_obs32=part)       # both forms in one call
    env.sync()
    assert np.array_equal(part.rows(), want32(oo[17:57])) and np.array_equal(bits(d_obs.to_host()), bits(oo[17:57]))
    env.close()


def test_argument_errors():
    env = make(8, "coop_test", "example", 2, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3")
    env.reset(return_obs=False)
    L, h = _native.lib(), env._h
    d_act, d_obs = env.alloc((8, 2), np.int32), env.alloc((8, 2, env.F), np.float64)
    rows, d_codes = GuardedRows(env), env.alloc((8, 2, env.codes_pitch), np.uint8)
    assert L.cz_step_device_f32(h, d_act.ptr, None, None, None, None) != 0 and b"float32" in L.cz_last_error(h)
    assert L.cz_observe_device_f32(h, 0, 8, None) != 0 and b"null" in L.cz_last_error(h)
    assert L.cz_obs_table_f32(h, None) != 0
    # both outputs set, in either order, and per call
    env.set_f32_output(rows)
    with pytest.raises(_native.NativeError, match="float32 output is set"):
        env.set_compact_output(d_codes)
    with pytest.raises(_native.NativeError, match="both set"):
        env.step_device_compact(d_act, d_codes, None, None, None)
    # a float64 buffer with the setting on
    with pytest.raises(_native.NativeError, match="d_obs = NULL"):
        env.step_device(d_act, d_obs, None, None, None)
    with pytest.raises(_native.NativeError, match="d_obs = NULL"):
        env.step(np.zeros((8, 2), np.int32))
    env.set_f32_output(None)
    env.set_compact_output(d_codes)
    with pytest.raises(_native.NativeError, match="compact output is set"):
        env.set_f32_output(rows)
    with pytest.raises(_native.NativeError, match="both set"):
        env.step_device_f32(d_act, rows, None, None, None)
    env.set_compact_output(None)
    # nothing of the above stepped the batch or wrote a row, and everything works afterwards
    assert (env.get_state()[:, soa.W_T] == 0).all() and (rows.rows() == SENTINEL).all()
    env.step_device_f32(d_act, rows, None, None, None)
    env.step_device(d_act, d_obs, None, None, None)
    env.sync()
    assert (env.get_state()[:, soa.W_T] == 2).all()
    env.close()


def test_host_step_with_the_float32_output_set():
    """cz_step with return_obs=False and the setting on: the launch it issues writes the float32 rows"""
    from oracle_binding import VecOracle
    n, A = 64, 2
    env = make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3")
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    orc.reset()
    rows = GuardedRows(env)
    env.set_f32_output(rows)
    rng = np.random.default_rng(2)
    for t in range(10):
        acts = rng.integers(0, 5, size=(n, A), dtype=np.int32)
        _, rg, tg, ug = env.step(acts, return_obs=False)
        oo, ro, to, uo = orc.step(acts)
        assert np.array_equal(rows.rows(), want32(oo)) and np.array_equal(bits(rg), bits(ro)) and np.array_equal(ug, uo), t
    env.close()


def test_two_shards_on_one_device_equal_one_handle():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n, A, T = 128, 2, 40
    args = ("coop_test", "example", A, 25, ["TomatoLettuceSalad", "CarrotBanana"])
    kw = dict(action_scheme="scheme3", num_layouts=8, auto_reset=True)
    one = make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=25)
    two = ShardedVecEnv(n, *args, device_ids=[0, 0], **kw)
    one.reset(return_obs=False)
    two.reset(return_obs=False)
    assert np.array_equal(two.obs_table_f32().view(np.uint32), one.obs_table_f32().view(np.uint32))
    F = one.F
    o_act, o_rows = one.alloc((n, A), np.int32), one.alloc((n, A, F), np.float32)
    o_out = [one.alloc((n, A), np.float64), one.alloc((n, A), np.uint8), one.alloc((n, A), np.uint8)]
    s_act, s_rows = two.alloc((A,), np.int32), two.alloc((A, F), np.float32)
    s_out = [two.alloc((A,), np.float64), two.alloc((A,), np.uint8), two.alloc((A,), np.uint8)]
    one.observe_device(d_obs32=o_rows)
    two.observe_device(d_obs32=s_rows)
    one.sync()
    two.sync()
    assert np.array_equal(s_rows.to_host().view(np.uint32), o_rows.to_host().view(np.uint32))
    rng = np.random.default_rng(6)
    for t in range(T):
        acts = rng.integers(0, 5, size=(n, A), dtype=np.int32)
        o_act.from_host(acts)
        s_act.from_host(acts)
        if t < T // 2:
            one.step_device_f32(o_act, o_rows, *o_out)
            two.step_device_f32(s_act, s_rows, *s_out)
        else:                                            # the second half through the handle setting
            if t == T // 2:
                one.set_f32_output(o_rows)
                two.set_f32_output(s_rows)
            one.step_device(o_act, None, *o_out)
            two.step_device(s_act, None, *s_out)
        one.sync()
        two.sync()
        assert np.array_equal(s_rows.to_host().view(np.uint32), o_rows.to_host().view(np.uint32)), t
        for a, b in zip(s_out, o_out):
            assert np.array_equal(a.to_host().view(np.uint8), b.to_host().view(np.uint8)), t
    assert np.array_equal(strip(two.get_state()), strip(one.get_state()))
    one.close()
    two.close()


def test_step_device_f32_captured_into_a_callers_graph_replays_bit_exact():
    """[a host-prepared action ring -> cz_step_device_f32] x K captured with hipStreamBeginCapture on the caller's stream: replays do
    what the same launches do eagerly on the twin, and capturing steps nothing"""
    n, A, K, R = 512, 2, 8, 25
    env, ref = (make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=25) for _ in range(2))
    ring_host = np.random.default_rng(12).integers(0, 5, size=(K, n, A), dtype=np.int32)
    bufs = []
    for e in (env, ref):
        e.reset(return_obs=False)
        ring = e.alloc((K, n, A), np.int32)
        ring.from_host(ring_host)
        bufs.append(dict(ring=ring, rows=GuardedRows(e), rew=e.alloc((n, A), np.float64), term=e.alloc((n, A), np.uint8),
                         trunc=e.alloc((n, A), np.uint8)))
    be, br = bufs
    cs = CallerStream(env)
    slot = lambda b, k: b["ring"].ptr + k * n * A * 4
    with cs.capture():
        for k in range(K):
            env.step_device_f32(slot(be, k), be["rows"], be["rew"], be["term"], be["trunc"])
        env.observe_device(d_obs32=be["rows"])                     # (a pure launch as well; rewrites the rows it finds)
    assert env._steps == 0 and env.captured_steps == K
    assert (env.get_state()[:, soa.W_T] == 0).all(), "capturing must not have stepped anything"
    cs.replay(R)
    cs.sync()
    for _ in range(R):
        for k in range(K):
            ref.step_device_f32(slot(br, k), br["rows"], br["rew"], br["term"], br["trunc"])
    ref.sync()
    assert np.array_equal(env.get_state(), ref.get_state())
    assert np.array_equal(be["rows"].rows(), br["rows"].rows()) and not (be["rows"].rows() == SENTINEL).any()
    for k in ("rew", "term", "trunc"):
        assert np.array_equal(be[k].to_host().view(np.uint8), br[k].to_host().view(np.uint8)), k
    assert env.stats() == ref.stats() and env.stats()["episodes"] > n
    cs.close()
    env.close()
    ref.close()


BOTH_SET = ("a float32 output (cz_set_f32_output / cz_step_device_f32) and a compact output (cz_set_compact_output / "
            "cz_step_device_compact) are both set: switch one of them off")
PASS_NULL = ("float32 observation rows are switched on (cz_set_f32_output): pass d_obs = NULL, or switch them off "
             "with cz_set_f32_output(h, NULL) to get float64 rows")


class Guarded:
    """a device array of `shape` with a sentinel in every element and GUARD more elements of it behind the last one"""
    SENTINELS = {1: 0xA5, 4: SENTINEL, 8: 0x7FF8BEEF0BADF00D}

    def __init__(self, env, shape, itemsize):
        self.shape, self.words = shape, int(np.prod(shape))
        self.dtype = {1: np.uint8, 4: np.uint32, 8: np.uint64}[itemsize]
        self.sentinel = self.SENTINELS[itemsize]
        self.buf = env.alloc((self.words + GUARD,), self.dtype)
        self.ptr = self.buf.ptr
        self.fill()

    def fill(self):
        self.buf.from_host(np.full(self.words + GUARD, self.sentinel, dtype=self.dtype))

    def get(self):
        got = self.buf.to_host()
        assert (got[self.words:] == self.sentinel).all(), "a store went past the array's end"
        return got[:self.words].reshape(self.shape)

    def untouched(self):
        return bool((self.buf.to_host() == self.sentinel).all())


def test_every_call_writes_the_outputs_it_names_and_no_others():
    """One handle, 9 envs (one full workgroup of 8 waves and a partial one) of the 7x7 two-agent level.  Every call form in turn -
    cz_step_device_f32, cz_step_device_compact, cz_step + cz_last_marks, cz_step_compact, cz_step_device, a 3-step
    cz_step_device_ring - first with no output set on the handle, then with cz_set_compact_output, then with cz_set_f32_output:
    what a call names (its own buffers, and the handle's buffer where the form includes it) equals the oracle bit for bit, every
    other buffer - the handle's one under a one-call form that excludes it, the one-call buffers under every later call - keeps its
    sentinel, and the refused combinations fail with their messages, step nothing and leave the next call working."""
    from oracle_binding import VecOracle
    n, A, K = 9, 2, 3
    env = make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=20)
    assert (env.dims.W, env.dims.H) == (7, 7)
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    orc.reset()
    F, Fp, table = env.F, env.codes_pitch, env.obs_table()
    B = dict(call32=Guarded(env, (n, A, F), 4), set32=Guarded(env, (n, A, F), 4), call_codes=Guarded(env, (n, A, Fp), 1),
             set_codes=Guarded(env, (n, A, Fp), 1), obs=Guarded(env, (n, A, F), 8), rew=Guarded(env, (n, A), 8),
             term=Guarded(env, (n, A), 1), trunc=Guarded(env, (n, A), 1))
    outs = (B["rew"], B["term"], B["trunc"])
    d_act, d_ring = env.alloc((n, A), np.int32), env.alloc((K, n, A), np.int32)
    rng = np.random.default_rng(31)
    state = {"steps": 0}

    def codes_ok(codes, oo):
        return np.array_equal(bits(table[codes[..., :F]]), bits(oo)) and (codes[..., F:] == 255).all()

    def expect(what, oracle, named, host=None):
        """`named`: the device buffers the call wrote (all of rew / term / trunc with "outs"); `host`: what a host step returned"""
        oo, ro, to, uo = oracle
        for key in named:
            if key in ("call32", "set32"):
                assert np.array_equal(B[key].get(), want32(oo)), (what, key)
            elif key in ("call_codes", "set_codes"):
                assert codes_ok(B[key].get(), oo), (what, key)
            elif key == "obs":
                assert np.array_equal(B[key].get(), bits(oo)), (what, key)
            else:
                assert key == "outs"
                assert np.array_equal(B["rew"].get(), bits(ro)) and np.array_equal(B["term"].get(), to) and np.array_equal(B["trunc"].get(), uo), what
        written = set(named) - {"outs"} | ({"rew", "term", "trunc"} if "outs" in named else set())
        for key, buf in B.items():
            if key not in written:
                assert buf.untouched(), (what, "wrote", key)
            buf.fill()
        if host is not None:
            og, cg, rg, tg, ug = host
            assert og is None or np.array_equal(bits(og), bits(oo)), what
            assert cg is None or codes_ok(cg, oo), what
            assert np.array_equal(bits(rg), bits(ro)) and np.array_equal(tg, to) and np.array_equal(ug, uo), what
        state["steps"] += 1
        assert np.array_equal(strip(env.get_state()), orc.records), what

    def refused(what, message, call):
        with pytest.raises(_native.NativeError) as err:
            call()
        assert message in str(err.value), what
        env.sync()
        assert all(buf.untouched() for buf in B.values()), what
        assert np.array_equal(strip(env.get_state()), orc.records), what

    def fresh():
        acts = rng.integers(0, 5, size=(n, A), dtype=np.int32)
        d_act.from_host(acts)
        return acts

    for setting in (None, "codes", "f32"):
        env.set_compact_output(B["set_codes"] if setting == "codes" else None)
        env.set_f32_output(B["set32"] if setting == "f32" else None)
        durable = [] if setting is None else ["set_codes" if setting == "codes" else "set32"]
        rows = None if setting == "f32" else B["obs"]           # the float64 buffer of the device calls: NULL under cz_set_f32_output
        named_rows = [] if setting == "f32" else ["obs"]
        for cycle in range(3):
            what = (setting, cycle)
            # cz_step_device_f32: its own rows and nothing else; refused beside a compact output of the handle
            acts = fresh()
            if setting == "codes":
                refused(what, BOTH_SET, lambda: env.step_device_f32(d_act, B["call32"], *outs))
            else:
                env.step_device_f32(d_act, B["call32"], *outs)
                env.sync()
                expect((what, "f32"), orc.step(acts), ["call32", "outs"])
            # cz_step_device_compact: its own codes (every other cycle with float64 rows beside them), not the handle's
            acts = fresh()
            beside = B["obs"] if cycle % 2 else None
            if setting == "f32":
                refused(what, BOTH_SET, lambda: env.step_device_compact(d_act, B["call_codes"], *outs, d_obs=beside))
            else:
                env.step_device_compact(d_act, B["call_codes"], *outs, d_obs=beside)
                env.sync()
                expect((what, "compact"), orc.step(acts), ["call_codes", "outs"] + (["obs"] if beside is not None else []))
            # cz_step: host arrays, cz_last_marks, and the handle's output
            acts = fresh()
            if setting == "f32":
                refused(what, PASS_NULL, lambda: env.step(acts))
            og, rg, tg, ug = env.step(acts, return_obs=setting != "f32")
            expect((what, "host"), orc.step(acts), durable, host=(og, None, rg, tg, ug))
            marks = orc.records[:, soa.W_MARKS].astype(np.uint64) | (orc.records[:, soa.W_MARKS_HI].astype(np.uint64) << np.uint64(32))
            assert np.array_equal(env.last_marks(), marks), what
            # cz_step_compact: host codes, not the handle's
            acts = fresh()
            if setting == "f32":
                refused(what, BOTH_SET, lambda: env.step_compact(acts))
            else:
                cg, rg, tg, ug = env.step_compact(acts)
                expect((what, "host compact"), orc.step(acts), [], host=(None, cg, rg, tg, ug))
            # cz_step_device: float64 rows (NULL, and refused otherwise, under cz_set_f32_output) and the handle's output
            acts = fresh()
            if setting == "f32":
                refused(what, PASS_NULL, lambda: env.step_device(d_act, B["obs"], *outs))
            env.step_device(d_act, rows, *outs)
            env.sync()
            expect((what, "device"), orc.step(acts), named_rows + durable + ["outs"])
            # cz_step_device_ring, 3 steps: the last step's outputs
            ring = rng.integers(0, 5, size=(K, n, A), dtype=np.int32)
            d_ring.from_host(ring)
            env.step_device_ring(K, d_ring, n * A, K, 0, rows, *outs)
            env.sync()
            for k in range(K - 1):
                orc.step(ring[k], False)
            expect((what, "ring"), orc.step(ring[K - 1]), named_rows + durable + ["outs"])
    assert int(env.get_state()[:, soa.W_EPISODE].min()) >= 2 and state["steps"] >= 40         # reset passes were among the steps
    env.close()
