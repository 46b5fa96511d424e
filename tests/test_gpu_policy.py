"""GPU: the MLP policy on the device - cz_load_policy_device (k_policy_pack), cz_policy_device (k_policy) and cz_rollout_policy
(k_step<..., ROLLOUT_POLICY>, mode 9) - against the oracle and the numpy model of cooking_zoo_amd/policy.py.

Every rollout comparison has two halves (policy_common.verify_rollout): the oracle replays the device's own actions - rows, rewards,
flags and records must be exact - and the device's actions and logits equal policy.host_actions / host_logits on the row before
each step: the oracle's first observation as float32, then the trajectory's own rows, which the first half has proved.  Agents
without a weight set must have played the oracle's action stream and have their logits untouched.

Conventions of test_gpu_rollout_f32.py: a sentinel in every buffer before every launch, one guard row behind each buffer that
must come back untouched, float32 compared as uint32, 35 envs (the last workgroup is partial at 8 and at 4 envs per workgroup), T = 5
with max_steps = 3 (an episode end, the reset pass and a layout change fall inside a launch), levels whose quotients are inexact in
float32.  Weights are N(0, 0.3^2), the output layer N(0, 0.03^2) so that sampling has a choice: nothing near NaN, infinities or subnormals, which the definition does not pin."""
import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from oracle_binding import VecOracle
from policy_common import (ACT_SENT, MOVABLE, ROLLOUT_POLICY, PolicyTraj, check_policy, current_obs, expected_policy, sets_for, start,
                           stream_actions, verify_rollout, weights, write_movable_levels)
from vec_common import CROWDED4, HUGE3, SENTINEL, TWO, CallerStream, instance, last_mode, make_env as make, strip, want32

pytestmark = pytest.mark.gpu

N, T, MAX_STEPS = 35, 5, 3


@pytest.fixture(scope="module")
def movable_levels(tmp_path_factory):
    return write_movable_levels(tmp_path_factory.mktemp("movable_policy"))


def crowded(n=N, **kw):
    args = dict(max_steps=MAX_STEPS)
    args.update(kw)
    return make(n, "crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1", **args)


def loaded(env, n_sets=2, seed=0):
    W = weights(env.F, env.num_actions, n_sets, seed, scale2=0.03)
    env.load_policy(*W)
    assert env.policy_sets == n_sets
    return W


# ---------------------------------------------------------------------------------------------------------------------------
# the matrix: every (instance, agents, scheme) cell, greedy and sample
# ---------------------------------------------------------------------------------------------------------------------------

CELLS = [(level, agents, scheme) for level in MOVABLE for agents in (1, 2, 3, 4) for scheme in ("scheme1", "scheme3")]


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("level,agents,scheme", CELLS, ids=[f"{l}-{a}agents-{s}" for l, a, s in CELLS])
def test_every_cell(movable_levels, level, agents, scheme, mode):
    lp, mp, inst = movable_levels[level]
    env = make(N, lp, mp, agents, CROWDED4[:agents], scheme, max_steps=MAX_STEPS, num_layouts=16)
    try:
        assert instance(env) == inst
        W = loaded(env, 2, agents)
        orc = VecOracle.from_vec_env(env)
        obs0 = start(env, orc)
        sets = sets_for(agents)
        got = PolicyTraj(env, T).rollout(env, sets, mode, 700 + agents, step0=2)
        assert last_mode(env) == ROLLOUT_POLICY
        recs = verify_rollout(f"{level} {agents} agents {scheme} {mode}", orc, obs0, got, W, sets, mode, 700 + agents, step0=2)
        assert np.array_equal(strip(env.get_state()), recs[-1]), "records after the launch"
        assert int(recs[-1][:, soa.W_EPISODE].min()) >= 1, "every env finished an episode and took the reset pass inside the launch"
        assert len(np.unique(got["logits"][:, :, 0])) >= 10, "the policy agent's logits barely vary: the case shows nothing"
        if mode == "sample":
            assert len(np.unique(got["act"][:, :, 0])) >= 2, "the sampling agent played one action only: the case shows nothing"
            assert (got["act"][:, :, 0] != got["logits"].view(np.float32)[:, :, 0].argmax(-1)).any(), "every draw fell on the largest logit"
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# row tails: F = 283, 384, 385, 513 and, on the huge instance, 639.  What this shows: the float32 rows the step kernels write at those
# F and their staging for the policy, on observation rows.  What it does not: the weights of a row's tail - observation rows are 0.0 in
# about half their features, the last 16 and more included (test_policy_host.py states it), so the columns of W1 there never reach a
# logit here.  test_gpu_policy_dense.py covers them, with dense rows through cz_policy_device at the same F.
# ---------------------------------------------------------------------------------------------------------------------------

TAILS = [("coop_test", "example_odd", 2, TWO, "scheme3", 283, 0)] + \
        [("coop_test", f"example_f{F}", 2, TWO, "scheme3", F, 0) for F in (384, 385, 513)] + \
        [("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", 639, 2)]


@pytest.mark.parametrize("case", TAILS, ids=[f"F{c[5]}" for c in TAILS])
def test_row_tails(case):
    level, meta, agents, recipes, scheme, F, inst = case
    env = make(20, level, meta, agents, recipes, scheme, max_steps=4, num_layouts=3)
    try:
        assert env.F == F and instance(env) == inst
        W = loaded(env, 2, F)
        orc = VecOracle.from_vec_env(env)
        obs0 = start(env, orc)
        sets = (0, 1) if agents == 2 else (0, 1, None)
        for mode, step0 in (("sample", 0), ("greedy", 6)):
            got = PolicyTraj(env, 6).rollout(env, sets, mode, 3 * F, step0)
            verify_rollout(f"F = {F} {mode}", orc, obs0, got, W, sets, mode, 3 * F, step0)
            obs0 = current_obs(orc)
        assert np.array_equal(strip(env.get_state()), orc.records)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# ties, T edges
# ---------------------------------------------------------------------------------------------------------------------------

def test_ties_go_to_the_first_action():
    env = crowded()
    W = [w.copy() for w in weights(env.F, env.num_actions, 1, 5)]
    W[2][0, 2] = W[2][0, 1]                                       # two identical rows of W2 and entries of b2, and far above the rest
    W[3][0, 1] = W[3][0, 2] = 50.0
    env.load_policy(*W)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    sets = (0, 0, 0, 0)
    got = PolicyTraj(env, T).rollout(env, sets, "greedy", 3)
    verify_rollout("ties", orc, obs0, got, W, sets, "greedy", 3)
    assert (got["act"] == 1).all(), "the first of two equal largest logits wins everywhere"
    assert np.array_equal(got["logits"][..., 1], got["logits"][..., 2]) and (got["logits"][..., 1] != SENTINEL).all()
    env.close()


def test_one_step_launches():
    env = crowded()
    W = loaded(env)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    tr, sets = PolicyTraj(env, 1), sets_for(4)
    for k in range(5):                                            # (the fourth step is a reset pass: the fifth reads its row)
        got = tr.rollout(env, sets, "sample", 40, step0=k)
        verify_rollout(f"T = 1, launch {k}", orc, obs0, got, W, sets, "sample", 40, step0=k)
        obs0 = current_obs(orc)
    assert np.array_equal(strip(env.get_state()), orc.records)
    env.close()


def test_three_then_four_steps_equal_seven():
    split, whole = crowded(), crowded()
    W = loaded(split)
    whole.load_policy(*W)
    orc = VecOracle.from_vec_env(split)
    obs0 = start(split, orc)
    whole.reset(return_obs=False)
    sets, seed = sets_for(4), 77
    a = PolicyTraj(split, 3).rollout(split, sets, "sample", seed, 0)
    b = PolicyTraj(split, 4).rollout(split, sets, "sample", seed, 3)
    c = PolicyTraj(whole, 7).rollout(whole, sets, "sample", seed, 0)
    verify_rollout("T = 7", orc, obs0, c, W, sets, "sample", seed, 0)
    for k in c:
        assert np.array_equal(np.concatenate([a[k], b[k]]), c[k]), f"3 + 4 steps against 7: {k}"
    assert np.array_equal(split.get_state(), whole.get_state()), "3 + 4 steps against 7: records"
    assert np.array_equal(strip(whole.get_state()), orc.records)
    assert split.stats() == whole.stats() and whole.stats()["episodes"] >= N
    split.close()
    whole.close()


# ---------------------------------------------------------------------------------------------------------------------------
# against the launches it fuses
# ---------------------------------------------------------------------------------------------------------------------------

def test_rollout_policy_is_t_times_policy_device_and_step_device_f32():
    fused, twin = crowded(), crowded()
    W = loaded(fused)
    twin.load_policy(*W)
    orc = VecOracle.from_vec_env(fused)
    obs0 = start(fused, orc)
    twin.reset(return_obs=False)
    sets, seed, step0, T_ = sets_for(4), 11, 4, 7
    stream = stream_actions(orc, T_, seed, step0)
    got = PolicyTraj(fused, T_).rollout(fused, sets, "sample", seed, step0)
    verify_rollout("fused", orc, obs0, got, W, sets, "sample", seed, step0)
    A, F, Cn = 4, twin.F, twin.num_actions
    rows = [twin.alloc((N, A, F), np.uint32) for _ in range(2)]
    d_act, d_lg = twin.alloc((N, A), np.int32), twin.alloc((N, A, Cn), np.uint32)
    d_rew, d_term, d_trunc = twin.alloc((N, A), np.uint64), twin.alloc((N, A), np.uint8), twin.alloc((N, A), np.uint8)
    twin.observe_device(d_obs32=rows[0])
    assert np.array_equal(rows[0].to_host(), want32(obs0)), "row 0 comes from observe_device"
    for t in range(T_):
        d_act.from_host(stream[t])                                # the stream agents' entries
        d_lg.from_host(np.full((N, A, Cn), SENTINEL, np.uint32))
        twin.policy_device(rows[t & 1], d_act, d_lg, sets=sets, mode="sample", seed=seed, step=step0 + t)
        twin.step_device_f32(d_act, rows[(t + 1) & 1], d_rew, d_term, d_trunc)
        twin.sync()
        for name, buf in (("act", d_act), ("logits", d_lg), ("rows", rows[(t + 1) & 1]), ("rew", d_rew), ("term", d_term), ("trunc", d_trunc)):
            assert np.array_equal(buf.to_host(), got[name][t]), f"step {t}: {name} of the two launches differ from the fused launch's"
    assert np.array_equal(twin.get_state(), fused.get_state()) and twin.stats() == fused.stats()
    fused.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# cz_policy_device: untouched entries, output subsets, ranges
# ---------------------------------------------------------------------------------------------------------------------------

def policy_rows(env, seed=0):
    """float32 rows [n][A][F] of table values (the oracle's reset observation)"""
    orc = VecOracle.from_vec_env(env)
    return want32(orc.reset())


@pytest.mark.parametrize("outputs", [("act", "logits"), ("act",), ("logits",)], ids="-".join)
def test_policy_device_output_subsets_ranges_and_untouched_entries(outputs):
    env = crowded()
    W = loaded(env)
    A, F, Cn = 4, env.F, env.num_actions
    x = policy_rows(env)
    sets = (1, None, 0, None)
    for begin, count in ((0, N), (3, 9), (N - 1, 1), (8, 16)):
        d_x = env.alloc((count + 1, A, F), np.uint32)
        d_x.from_host(np.concatenate([x[begin:begin + count], np.full((1, A, F), SENTINEL, np.uint32)]))
        d_act, d_lg = env.alloc((count + 1, A), np.int32), env.alloc((count + 1, A, Cn), np.uint32)
        d_act.from_host(np.full((count + 1, A), ACT_SENT, np.int32))
        d_lg.from_host(np.full((count + 1, A, Cn), SENTINEL, np.uint32))
        env.policy_device(d_x, d_act if "act" in outputs else None, d_lg if "logits" in outputs else None, sets=sets, mode="sample", seed=9,
                          step=17, env_begin=begin, env_count=count)
        env.sync()
        act, lg = d_act.to_host(), d_lg.to_host()
        assert (act[count] == ACT_SENT).all() and (lg[count] == SENTINEL).all(), "guard rows"
        want_a, want_l, mask = expected_policy(x[None, begin:begin + count], W, sets, "sample", 9, 17, np.full((1, count, A), ACT_SENT, np.int32),
                                               env_id_base=begin)
        got = dict(act=act[None, :count] if "act" in outputs else None, logits=lg[None, :count] if "logits" in outputs else None)
        check_policy(f"envs [{begin}, {begin + count}) {outputs}", got, want_a, want_l, mask)
        if "act" not in outputs:
            assert (act == ACT_SENT).all(), "the actions were not asked for"
        if "logits" not in outputs:
            assert (lg == SENTINEL).all(), "the logits were not asked for"
    env.close()


@pytest.mark.parametrize("skip", [(), ("act",), ("logits",), ("rew", "term", "trunc"), ("act", "logits", "rew", "term", "trunc"), ("logits", "term")],
                         ids=lambda s: "no-" + "-".join(s) if s else "all")
def test_rollout_output_subsets(skip):
    env, ref = crowded(), crowded()
    W = loaded(env)
    ref.load_policy(*W)
    orc = VecOracle.from_vec_env(ref)
    obs0 = start(ref, orc)
    env.reset(return_obs=False)
    sets = sets_for(4)
    full = PolicyTraj(ref, T).rollout(ref, sets, "sample", 21)
    verify_rollout("all outputs", orc, obs0, full, W, sets, "sample", 21)
    tr = PolicyTraj(env, T, skip=skip)
    got = tr.rollout(env, sets, "sample", 21)
    for k, v in got.items():
        assert (v is None) == (k in skip)
        if v is not None:
            assert np.array_equal(v, full[k]), f"without {skip}: {k}"
    assert np.array_equal(env.get_state(), ref.get_state()) and env.stats() == ref.stats()
    env.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# reload, refusals, capture
# ---------------------------------------------------------------------------------------------------------------------------

def test_reload_behind_a_launch_changes_the_next_launch_only():
    env = crowded()
    W1, W2 = weights(env.F, env.num_actions, 2, 1), weights(env.F, env.num_actions, 2, 2)
    dev = [[env.alloc(w.shape, np.float32) for w in W] for W in (W1, W2)]
    for bufs, W in zip(dev, (W1, W2)):
        for b, w in zip(bufs, W):
            b.from_host(w)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    sets = sets_for(4)
    ta, tb = PolicyTraj(env, T), PolicyTraj(env, T)
    ta.fill()
    tb.fill()
    env.load_policy(*dev[0])                                       # four stream-ordered calls, no wait in between
    ta.launch(env, sets, "greedy", 5, 0)
    env.load_policy(*dev[1])
    tb.launch(env, sets, "greedy", 5, T)
    env.sync()
    verify_rollout("first weights", orc, obs0, ta.get(), W1, sets, "greedy", 5, 0)
    verify_rollout("second weights", orc, current_obs(orc), tb.get(), W2, sets, "greedy", 5, T)
    env.close()


def test_refusals_step_nothing_and_write_nothing():
    env = crowded()
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    tr = PolicyTraj(env, T)
    tr.fill()
    b = tr.buf
    state = env.get_state()
    W = weights(env.F, env.num_actions, 2, 0)
    run = lambda **kw: env.rollout_policy(kw.pop("T", T), kw.pop("rows", b["rows"]), b["act"], b["logits"], b["rew"], b["term"], b["trunc"], **kw)
    pol = lambda **kw: env.policy_device(kw.pop("rows", b["rows"]), kw.pop("act", b["act"]), kw.pop("lg", b["logits"]), **kw)

    def refused(message, call):
        with pytest.raises(_native.NativeError, match=message):
            call()
        env.sync()
        assert np.array_equal(env.get_state(), state), f"a refused call ({message}) stepped something"
        for k, v in tr.get().items():
            assert (v == tr.fillers[k][2]).all(), f"a refused call ({message}) wrote {k}"

    refused("no weight table loaded", lambda: run())
    refused("no weight table loaded", lambda: pol())
    lib = _native.lib()
    dW = [env.alloc(w.shape, np.float32) for w in W]
    for n_sets in (0, 5, -1):
        with pytest.raises(_native.NativeError, match="n_sets"):
            _native.check(env._h, lib.cz_load_policy_device(env._h, n_sets, dW[0].ptr, dW[1].ptr, dW[2].ptr, dW[3].ptr))
    for k in range(4):
        ptrs = [None if j == k else d.ptr for j, d in enumerate(dW)]
        with pytest.raises(_native.NativeError, match="pointer is null"):
            _native.check(env._h, lib.cz_load_policy_device(env._h, 2, *ptrs))
    assert env.policy_sets == 0
    env.load_policy(*W)
    limit = 0xFFFFFFFF // (N * 4 * 8)
    refused("T must be >= 1", lambda: run(T=0))
    refused("float32 trajectory pointer", lambda: run(rows=None))
    refused(f"T <= {limit} here", lambda: run(T=limit + 1))
    refused("every agent's set is 0xFF", lambda: run(sets=(None, None, None, None)))
    refused("weight set 2, but 2 are loaded", lambda: run(sets=(0, 2, 0, 0)))
    refused("weight set 3, but 2 are loaded", lambda: pol(sets=(3, 0, 0, 0)))
    refused("both output pointers are null", lambda: pol(act=None, lg=None))
    refused("rows pointer is null", lambda: pol(rows=None))
    refused("range|outside|env", lambda: pol(env_begin=N - 2, env_count=5))
    with pytest.raises(KeyError):
        run(mode="argmax")
    sets = sets_for(4)
    verify_rollout("after the refusals", orc, obs0, tr.rollout(env, sets, "greedy", 8), W, sets, "greedy", 8)
    env.close()


def test_reload_and_rollout_captured_into_a_callers_graph():
    env, ref = crowded(), crowded()
    Wa, Wb = weights(env.F, env.num_actions, 2, 3), weights(env.F, env.num_actions, 2, 4)
    dev = [env.alloc(w.shape, np.float32) for w in Wa]
    for d, w in zip(dev, Wa):
        d.from_host(w)
    env.load_policy(*dev)                                          # the handle's first load allocates: outside the capture
    env.reset(return_obs=False)
    orc = VecOracle.from_vec_env(ref)
    obs0 = start(ref, orc)
    sets = sets_for(4)
    tr, rr = PolicyTraj(env, T), PolicyTraj(ref, T)
    tr.fill()
    for d, w in zip(dev, Wb):
        d.from_host(w)
    env.sync()
    cs = CallerStream(env)
    with cs.capture():
        env.load_policy(*dev)
        tr.launch(env, sets, "sample", 13, 0)
    assert (env.get_state()[:, soa.W_T] == 0).all(), "capturing must not have stepped anything"
    ref.load_policy(*Wb)
    for k in range(2):                                             # replayed twice: the second replay goes on from the first one's state
        tr.fill()
        cs.replay()
        cs.sync()
        got = tr.get()
        eager = rr.rollout(ref, sets, "sample", 13, 0)
        verify_rollout(f"replay {k}", orc, obs0, got, Wb, sets, "sample", 13, 0)
        obs0 = current_obs(orc)
        for name in got:
            assert np.array_equal(got[name], eager[name]), f"replay {k}: {name} differs from the eager launch"
    assert np.array_equal(env.get_state(), ref.get_state()) and env.stats() == ref.stats()
    cs.close()
    env.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# shards of unequal size, despawn / respawn
# ---------------------------------------------------------------------------------------------------------------------------

def test_three_unequal_shards_equal_one_handle():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n, A = 13, 4
    one = crowded(n)
    three = ShardedVecEnv(n, "crowded_6x5", "crowded_6x5", A, MAX_STEPS, CROWDED4, device_ids=[0, 0, 0], action_scheme="scheme1", num_layouts=8,
                          auto_reset=True)
    assert [s.num_envs for s in three.shards] == [5, 4, 4]
    W = loaded(one)
    three.load_policy(*W)
    assert three.policy_sets == 2
    orc = VecOracle.from_vec_env(one)
    obs0 = start(one, orc)
    three.reset(return_obs=False)
    sets = sets_for(A)
    got = PolicyTraj(one, T).rollout(one, sets, "sample", 19)
    sharded = PolicyTraj(three, T, sharded=True).rollout(three, sets, "sample", 19)
    verify_rollout("one handle", orc, obs0, got, W, sets, "sample", 19)
    for k in got:
        assert np.array_equal(got[k], sharded[k]), f"shards: {k}"
    assert np.array_equal(three.get_state(), one.get_state())
    # ... and cz_policy_device over the shards' slices of one array
    d1, d3 = one.alloc((n, A), np.int32), three.alloc((A,), np.int32)
    x1, x3 = one.alloc((n, A, one.F), np.uint32), three.alloc((A, one.F), np.uint32)
    for d in (d1, d3):
        d.from_host(np.full((n, A), ACT_SENT, np.int32))
    for x in (x1, x3):
        x.from_host(got["rows"][-1])
    one.policy_device(x1, d1, sets=sets, mode="sample", seed=4, step=3)
    three.policy_device(x3, d3, sets=sets, mode="sample", seed=4, step=3)
    one.sync()
    three.sync()
    want, _, _ = expected_policy(got["rows"][-1][None], W, sets, "sample", 4, 3, np.full((1, n, A), ACT_SENT, np.int32))
    assert np.array_equal(d1.to_host(), want[0]) and np.array_equal(d3.to_host(), want[0])
    one.close()
    three.close()


def test_despawn_and_respawn():
    """an absent agent's action is computed and ignored: the rows, which the oracle makes from the device's actions, say so"""
    env = make(N, "crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme3", max_steps=9, agent_despawn_rate=0.1, agent_respawn_rate=0.3,
               grace_period=2, spawn_seed=5)
    W = loaded(env)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    sets = (1, 0, 0, 0)
    got = PolicyTraj(env, 12).rollout(env, sets, "sample", 6)
    recs = verify_rollout("despawn", orc, obs0, got, W, sets, "sample", 6)
    assert np.array_equal(strip(env.get_state()), recs[-1])
    gone = np.stack([(r[:, soa.W_STATUS] >> 8) & 0xF for r in recs])
    assert (gone != 0).any(), "nobody was despawned: the case shows nothing"
    env.close()
