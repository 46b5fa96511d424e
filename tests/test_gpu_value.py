"""GPU: the critic on the device - cz_load_value_device (k_value_pack), cz_value_device (k_value) and cz_rollout_policy_value
(k_step<..., ROLLOUT_POLICY_VALUE>, mode 10) - against the oracle and the numpy model of cooking_zoo_amd/policy.py (host_value).

A rollout with values is compared in three parts: policy_common.verify_rollout on everything cz_rollout_policy writes (the oracle
replays the device's actions; actions and logits follow the model on the row before each step), then values rows 0 .. T against
host_value on [the oracle's first observation as float32, rows 0 .. T - 1] - the rows the first part has proved.  Agents without a
value set must have their entries untouched.

Conventions of test_gpu_policy.py: a sentinel in every buffer before every launch, one guard row behind each buffer (for the values
behind row T + 1) that must come back untouched, float32 compared as uint32, 35 envs, T = 5 with max_steps = 3, weights N(0, 0.3^2).
Nothing near NaN, infinities or subnormals, which the definition does not pin."""
import itertools

import numpy as np
import pytest

from cooking_zoo_amd import _native, policy, soa, targets
from oracle_binding import VecOracle
from policy_common import (MOVABLE, PolicyTraj, current_obs, dense_rows, sets_for, start, verify_rollout, weights,
                           write_movable_levels)
from targets_common import F32_SENT, GAMMA, LAM, bits32
from value_common import (ROLLOUT_POLICY_VALUE, ValueTraj, check_values, expected_values, matrix_product_value, split_values,
                          value_as_logit_set, value_weights)
from vec_common import CROWDED4, HUGE3, SENTINEL, TWO, CallerStream, instance, last_mode, make_env as make, strip, want32

pytestmark = pytest.mark.gpu

N, T, MAX_STEPS = 35, 5, 3


@pytest.fixture(scope="module")
def movable_levels(tmp_path_factory):
    return write_movable_levels(tmp_path_factory.mktemp("movable_value"))


def crowded(n=N, **kw):
    args = dict(max_steps=MAX_STEPS)
    args.update(kw)
    return make(n, "crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1", **args)


def loaded(env, n_sets=2, seed=0):
    W, V = weights(env.F, env.num_actions, n_sets, seed, scale2=0.03), value_weights(n_sets, seed)
    env.load_policy(*W)
    assert env.value_sets == 0
    env.load_value(*V)
    assert env.policy_sets == n_sets and env.value_sets == n_sets
    return W, V


def vsets_for(A, flip):
    """beside sets_for(A) = (1, 0, ..., None): agent 0's value set equals its policy set, agent 1's differs (a second hidden pass),
    agent 2's is equal again; with one policy agent only (A <= 2) `flip` chooses between equal and different.  The agent without a
    policy has a value under the action stream when `flip`, none otherwise"""
    if A == 1:
        return (0 if flip else 1,)
    v = [1, 1, 0][:A - 1] if A >= 3 else [0 if flip else 1]
    return tuple(v) + (0 if flip else None,)


def verify_values(ctx, obs0, got, W, V, vsets):
    """values rows 0 .. T against host_value on [obs0 as float32, rows 0 .. T - 1]"""
    before = np.concatenate([want32(obs0)[None], got["rows"]])
    want, mask = expected_values(before, W, V, vsets)
    assert mask.sum() == sum(s is not None for s in vsets)
    check_values(ctx, got["values"], want, mask)
    return want


def verify(ctx, orc, obs0, got, W, V, sets, vsets, mode, seed, step0=0):
    rest, _ = split_values(got)
    recs = verify_rollout(ctx, orc, obs0, rest, W, sets, mode, seed, step0)
    verify_values(ctx, obs0, got, W, V, vsets)
    return recs


# ---------------------------------------------------------------------------------------------------------------------------
# cz_value_device on dense rows, at every row tail, with one to four agents
# ---------------------------------------------------------------------------------------------------------------------------

DENSE = [("crowded_6x5", "crowded_6x5", a, CROWDED4[:a], "scheme1", None) for a in (1, 2, 3, 4)] + \
        [("coop_test", meta, 2, TWO, "scheme3", F) for meta, F in (("example_odd", 283), ("example_f384", 384), ("example_f385", 385),
                                                                    ("example_f513", 513))]
ROW_COUNTS = (1, 63, 64, 65, 5 * N)


@pytest.mark.parametrize("case", DENSE, ids=[f"{c[1]}-{c[2]}agents" for c in DENSE])
def test_value_device_on_dense_rows(case):
    level, meta, A, recipes, scheme, F = case
    env = make(4, level, meta, A, recipes, scheme, max_steps=4, num_layouts=3)
    try:
        assert F is None or env.F == F
        F, Cn, R = env.F, env.num_actions, max(ROW_COUNTS)
        ctx = f"{level} / {meta}, {A} agents, F = {F}"
        W, V = weights(F, Cn, 4, F + A), value_weights(4, F + A)
        x = dense_rows(R, A, F, F + A)
        # the model, once: per value set the values of every row; and what makes the comparison able to fail
        per_set = [policy.host_value(x, W[0][s], W[1][s], V[0][s], V[1][s]) for s in range(4)]
        flat = x.reshape(-1, F)
        differ = sum(int((matrix_product_value(flat, W[0][s], W[1][s], V[0][s], V[1][s]).view(np.uint32) != per_set[s].reshape(-1).view(np.uint32)).sum())
                     for s in range(4))
        share = differ / (4 * len(flat))
        print(f"{ctx}: {share:.1%} of the expected values differ from the matrix-product form")
        assert share >= 0.25, f"{ctx}: only {share:.1%} of the values differ from the matrix-product form: the case shows nothing"
        for s, t in itertools.combinations(range(4), 2):
            assert (per_set[s].view(np.uint32) != per_set[t].view(np.uint32)).all(), f"{ctx}: sets {s} and {t} give one value somewhere"
        env.load_policy(*W)
        env.load_value(*V)
        assert env.value_sets == 4
        d_x = env.alloc((R + 1, A, F), np.uint32)
        d_x.from_host(np.concatenate([x.view(np.uint32), np.full((1, A, F), SENTINEL, np.uint32)]))     # (NaN directly behind the last row)
        d_v = env.alloc((R + 1, A), np.uint32)
        fill = np.full((R + 1, A), SENTINEL, np.uint32)
        subsets = [m for m in range(1, 1 << A)]
        for k, rows in enumerate(ROW_COUNTS):
            for m in subsets:
                vsets = tuple((a + k + m) % 4 if m >> a & 1 else None for a in range(A))
                d_v.from_host(fill)
                env.value_device(d_x, d_v, vsets=vsets, rows=rows)
                env.sync()
                got = d_v.to_host()
                assert (got[rows:] == SENTINEL).all(), f"{ctx}, {rows} rows, vsets {vsets}: a store went past the last row"
                for a in range(A):
                    if vsets[a] is None:
                        assert (got[:rows, a] == SENTINEL).all(), f"{ctx}, {rows} rows, vsets {vsets}: agent {a} has no value set and was written"
                    else:
                        bad = np.argwhere(got[:rows, a] != per_set[vsets[a]][:rows, a].view(np.uint32))
                        assert not len(bad), f"{ctx}, {rows} rows, vsets {vsets}: agent {a}'s values differ in bits at rows {bad[:6, 0].tolist()}"
        # ... and the value is the logit policy_device gives for a set whose W2 row c is wv and whose b2[c] is bv
        vsets = tuple(range(A))
        d_v.from_host(fill)
        env.value_device(d_x, d_v, vsets=vsets, rows=R)
        as_logits = [value_as_logit_set(W[0][s], W[1][s], V[0][s], V[1][s], Cn, s % Cn) for s in range(4)]
        env.load_policy(*(np.stack(p) for p in zip(*as_logits)))
        d_lg = env.alloc((4, A, Cn), np.uint32)
        d_lg.from_host(np.full((4, A, Cn), SENTINEL, np.uint32))
        env.policy_device(d_x, None, d_lg, sets=vsets, env_count=4)
        env.sync()
        lg, val = d_lg.to_host(), d_v.to_host()
        for a in range(A):
            assert np.array_equal(lg[:, a, a % Cn], val[:4, a]) and (val[:4, a] != SENTINEL).all(), f"{ctx}: agent {a}'s value is not the logit of the same weights"
    finally:
        env.close()


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
        W, V = loaded(env, 2, agents)
        orc = VecOracle.from_vec_env(env)
        obs0 = start(env, orc)
        sets, vsets = sets_for(agents), vsets_for(agents, (agents + (scheme == "scheme3")) % 2 == 1)
        got = ValueTraj(env, T).rollout(env, sets, mode, 700 + agents, step0=2, vsets=vsets)
        assert last_mode(env) == ROLLOUT_POLICY_VALUE
        ctx = f"{level} {agents} agents {scheme} {mode}, vsets {vsets}"
        recs = verify(ctx, orc, obs0, got, W, V, sets, vsets, mode, 700 + agents, step0=2)
        assert np.array_equal(strip(env.get_state()), recs[-1]), "records after the launch"
        assert int(recs[-1][:, soa.W_EPISODE].min()) >= 1, "every env finished an episode and took the reset pass inside the launch"
        assert len(np.unique(got["values"][:, :, 0])) >= 10, "the first agent's values barely vary: the case shows nothing"
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the same launch with and without values; chains of launches
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_the_launch_with_values_leaves_what_the_launch_without_them_leaves(mode):
    env = crowded()
    W, V = loaded(env)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    archive = env.alloc((N, env.dims.RW), np.uint32)
    env.save_device(archive)
    sets = sets_for(4)
    plain = PolicyTraj(env, T).rollout(env, sets, mode, 31, step0=1)
    state_plain, stats_plain = env.get_state(), env.stats()
    verify_rollout("without values", orc, obs0, plain, W, sets, mode, 31, step0=1)
    for vsets in ((1, 0, 0, None), (0, 1, None, 1), (None, None, None, 0)):
        env.restore_device(archive)
        got = ValueTraj(env, T).rollout(env, sets, mode, 31, step0=1, vsets=vsets)
        assert last_mode(env) == ROLLOUT_POLICY_VALUE
        rest, _ = split_values(got)
        for k in plain:
            assert rest[k].tobytes() == plain[k].tobytes(), f"vsets {vsets}: {k} differs from the launch without values"
        assert np.array_equal(env.get_state(), state_plain), f"vsets {vsets}: records differ from the launch without values"
        verify_values(f"vsets {vsets}", obs0, got, W, V, vsets)
    assert env.stats()["episodes"] >= stats_plain["episodes"] >= N
    env.close()


def test_chained_launches_and_three_then_four_steps_equal_seven():
    split, whole = crowded(), crowded()
    W, V = loaded(split)
    whole.load_policy(*W)
    whole.load_value(*V)
    orc = VecOracle.from_vec_env(split)
    obs0 = start(split, orc)
    whole.reset(return_obs=False)
    sets, vsets, seed = sets_for(4), (1, 1, None, 0), 77
    a = ValueTraj(split, 3).rollout(split, sets, "sample", seed, 0, vsets=vsets)
    b = ValueTraj(split, 4).rollout(split, sets, "sample", seed, 3, vsets=vsets)
    c = ValueTraj(whole, 7).rollout(whole, sets, "sample", seed, 0, vsets=vsets)
    verify("T = 7", orc, obs0, c, W, V, sets, vsets, "sample", seed, 0)
    assert np.array_equal(a["values"][3], b["values"][0]), "row T of a launch is row 0 of the next one"
    for k in c:
        joined = np.concatenate([a[k][:3], b[k]]) if k == "values" else np.concatenate([a[k], b[k]])
        assert np.array_equal(joined, c[k]), f"3 + 4 steps against 7: {k}"
    assert np.array_equal(split.get_state(), whole.get_state()), "3 + 4 steps against 7: records"
    assert split.stats() == whole.stats() and whole.stats()["episodes"] >= N
    # ... and a chain of one-step launches: row 1 of launch k is row 0 of launch k + 1 (the fourth step is a reset pass)
    one = ValueTraj(whole, 1)
    obs0, prev = current_obs(orc), None
    for k in range(5):
        got = one.rollout(whole, sets, "greedy", 5, step0=k, vsets=vsets)
        verify(f"T = 1, launch {k}", orc, obs0, got, W, V, sets, vsets, "greedy", 5, step0=k)
        assert prev is None or np.array_equal(prev, got["values"][0]), f"launch {k}: row 0 is not the row T of the launch before"
        obs0, prev = current_obs(orc), got["values"][1]
    split.close()
    whole.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the huge instance at F = 639, frozen envs, despawn / respawn
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_huge_instance_at_f_639():
    env = make(20, "huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", max_steps=4, num_layouts=3)
    try:
        assert env.F == 639 and instance(env) == 2
        W, V = loaded(env, 2, 639)
        orc = VecOracle.from_vec_env(env)
        obs0 = start(env, orc)
        sets = (0, 1, None)
        for mode, step0, vsets in (("sample", 0, (0, 0, 1)), ("greedy", 6, (None, 1, None))):
            got = ValueTraj(env, 6).rollout(env, sets, mode, 1917, step0, vsets=vsets)
            verify(f"F = 639 {mode}", orc, obs0, got, W, V, sets, vsets, mode, 1917, step0)
            obs0 = current_obs(orc)
        assert np.array_equal(strip(env.get_state()), orc.records)
    finally:
        env.close()


def test_frozen_envs_without_auto_reset():
    """a finished env stays as it is: in the second launch every env is frozen, and its row, and so its value, repeats"""
    env, twin = crowded(auto_reset=False), crowded(auto_reset=False)
    W, V = loaded(env)
    twin.load_policy(*W)
    env.reset(return_obs=False)
    twin.reset(return_obs=False)
    rows0 = env.alloc((N, 4, env.F), np.uint32)
    env.observe_device(d_obs32=rows0)
    env.sync()
    x0 = rows0.to_host()
    sets, vsets = sets_for(4), (1, 0, None, 1)
    for k in range(2):
        got = ValueTraj(env, T).rollout(env, sets, "sample", 3, step0=k * T, vsets=vsets)
        plain = PolicyTraj(twin, T).rollout(twin, sets, "sample", 3, step0=k * T)
        rest, values = split_values(got)
        for name in plain:
            assert np.array_equal(rest[name], plain[name]), f"launch {k}: {name} differs from the launch without values"
        assert np.array_equal(env.get_state(), twin.get_state())
        want, mask = expected_values(np.concatenate([x0[None], got["rows"]]), W, V, vsets)
        check_values(f"launch {k}", values, want, mask)
        if k == 0:
            assert ((got["term"] | got["trunc"]) != 0).any(axis=(0, 2)).all(), "every env ends inside the first launch (max_steps = 3 < T)"
        else:
            assert np.array_equal(got["rows"][0], got["rows"][-1]) and np.array_equal(values[0], values[T]), "a frozen env's row and value repeat"
        x0 = got["rows"][-1]
    assert (env.get_state()[:, soa.W_EPISODE] == 0).all(), "nobody was reset"
    env.close()
    twin.close()


def test_despawn_and_respawn():
    env = make(N, "crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme3", max_steps=9, agent_despawn_rate=0.1, agent_respawn_rate=0.3,
               grace_period=2, spawn_seed=5)
    W, V = loaded(env)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    sets, vsets = (1, 0, 0, 0), (1, 1, None, 0)
    got = ValueTraj(env, 12).rollout(env, sets, "sample", 6, vsets=vsets)
    recs = verify("despawn", orc, obs0, got, W, V, sets, vsets, "sample", 6)
    assert np.array_equal(strip(env.get_state()), recs[-1])
    gone = np.stack([(r[:, soa.W_STATUS] >> 8) & 0xF for r in recs])
    assert (gone != 0).any(), "nobody was despawned: the case shows nothing"
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# reload, refusals, capture, shards
# ---------------------------------------------------------------------------------------------------------------------------

def test_a_reload_of_value_heads_behind_a_launch_changes_the_next_launch_only():
    env = crowded()
    W = weights(env.F, env.num_actions, 2, 1, scale2=0.03)
    Va, Vb = value_weights(2, 1), value_weights(2, 2)
    dev = [[env.alloc(v.shape, np.float32) for v in V] for V in (Va, Vb)]
    for bufs, V in zip(dev, (Va, Vb)):
        for b, v in zip(bufs, V):
            b.from_host(v)
    env.load_policy(*W)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    sets, vsets = sets_for(4), (1, 1, 0, 0)
    ta, tb = ValueTraj(env, T), ValueTraj(env, T)
    ta.vsets = tb.vsets = vsets
    ta.fill()
    tb.fill()
    env.load_value(*dev[0])                                        # four stream-ordered calls, no wait in between
    ta.launch(env, sets, "greedy", 5, 0)
    env.load_value(*dev[1])
    tb.launch(env, sets, "greedy", 5, T)
    env.sync()
    ga, gb = ta.get(), tb.get()
    verify("first heads", orc, obs0, ga, W, Va, sets, vsets, "greedy", 5, 0)
    verify("second heads", orc, current_obs(orc), gb, W, Vb, sets, vsets, "greedy", 5, T)
    assert not np.array_equal(ga["values"][T], gb["values"][0]), "the two loads give one value: the case shows nothing"
    env.close()


def test_refusals_step_nothing_and_write_nothing():
    env = crowded()
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    tr = ValueTraj(env, T)
    tr.fill()
    b = tr.buf
    state = env.get_state()
    W, V = weights(env.F, env.num_actions, 3, 0, scale2=0.03), value_weights(2, 0)
    run = lambda **kw: env.rollout_policy_value(kw.pop("T", T), kw.pop("rows", b["rows"]), kw.pop("values", tr.values), b["act"], b["logits"], b["rew"],
                                                b["term"], b["trunc"], **kw)
    val = lambda **kw: env.value_device(kw.pop("x", b["rows"]), kw.pop("values", tr.values), **kw)

    def refused(message, call):
        with pytest.raises(_native.NativeError, match=message):
            call()
        env.sync()
        assert np.array_equal(env.get_state(), state), f"a refused call ({message}) stepped something"
        for k, v in tr.get().items():
            sent = SENTINEL if k == "values" else tr.fillers[k][2]
            assert (v == sent).all(), f"a refused call ({message}) wrote {k}"

    lib = _native.lib()
    dV = [env.alloc(v.shape, np.float32) for v in V]
    refused("cz_load_policy_device allocates it", lambda: env.load_value(*V))
    refused("no weight table loaded", lambda: run())
    refused("no weight table loaded", lambda: val())
    assert env.value_sets == 0
    env.load_policy(*W)
    refused("value head of set 0, but 3 sets and 0 value heads", lambda: run())
    refused("value head of set 0, but 3 sets and 0 value heads", lambda: val())
    for n_sets in (0, 5, -1):
        with pytest.raises(_native.NativeError, match="n_sets"):
            _native.check(env._h, lib.cz_load_value_device(env._h, n_sets, dV[0].ptr, dV[1].ptr))
    for ptrs in ((None, dV[1].ptr), (dV[0].ptr, None)):
        with pytest.raises(_native.NativeError, match="pointer is null"):
            _native.check(env._h, lib.cz_load_value_device(env._h, 2, *ptrs))
    assert env.value_sets == 0
    env.load_value(*V)
    assert env.value_sets == 2 and env.policy_sets == 3
    limit = 0xFFFFFFFF // (N * 4 * 8)
    refused("T must be >= 1", lambda: run(T=0))
    refused("trajectory and values pointers non-null", lambda: run(rows=None))
    refused("trajectory and values pointers non-null", lambda: run(values=None))
    refused(f"T <= {limit} here", lambda: run(T=limit + 1))
    refused("0xFF in both sets and vsets", lambda: run(sets=(None,) * 4, vsets=(None,) * 4))
    refused("weight set 3, but 3 are loaded", lambda: run(sets=(0, 3, 0, 0), vsets=(0, 0, 0, 0)))
    refused("value head of set 2, but 3 sets and 2 value heads", lambda: run(sets=(0, 0, 0, 0), vsets=(0, 2, 0, 0)))
    refused("value head of set 2, but 3 sets and 2 value heads", lambda: run(sets=(2, 0, 0, 0)))                 # vsets=None: as sets
    refused("value head of set 3, but 3 sets and 2 value heads", lambda: val(vsets=(None, None, 3, None)))
    refused("every agent's byte of vsets is 0xFF", lambda: val(vsets=(None,) * 4))
    refused("rows or values pointer is null", lambda: val(x=None))
    refused("rows or values pointer is null", lambda: val(values=None))
    refused("rows is 0", lambda: val(rows=0))
    env.load_policy(*(w[:1] for w in W))                           # fewer policy sets than value heads: the smaller count holds
    refused("value head of set 1, but 1 sets and 2 value heads", lambda: val(vsets=(1, 0, 0, 0)))
    env.load_policy(*W)
    with pytest.raises(KeyError):
        run(mode="argmax")
    # values under the action stream are no refusal; and everything still works
    sets, vsets = (None,) * 4, (0, None, 1, None)
    got = tr.rollout(env, sets, "greedy", 8, vsets=vsets)
    recs = verify_rollout("stream only", orc, obs0, split_values(got)[0], W, sets, "greedy", 8)
    verify_values("stream only", obs0, got, W, V, vsets)
    assert (got["logits"] == SENTINEL).all() and np.array_equal(strip(env.get_state()), recs[-1])
    env.close()


def test_the_collection_phase_captured_into_a_callers_graph():
    """reload, rollout with values, logprob_device and gae_device in one graph of the caller: equal to the eager run, and the
    advantages are targets.host_gae on the device's own values"""
    env, ref = crowded(), crowded()
    Wa, Va = weights(env.F, env.num_actions, 2, 3, scale2=0.03), value_weights(2, 3)
    Wb, Vb = weights(env.F, env.num_actions, 2, 4, scale2=0.03), value_weights(2, 4)
    dev = [env.alloc(w.shape, np.float32) for w in Wa + Va]
    for d, w in zip(dev, Wa + Va):
        d.from_host(w)
    env.load_policy(*dev[:4])                                      # the handle's first load allocates: outside the capture
    env.load_value(*dev[4:])
    env.reset(return_obs=False)
    orc = VecOracle.from_vec_env(ref)
    obs0 = start(ref, orc)
    sets = vsets = (1, 0, 0, 0)
    tr, rr = ValueTraj(env, T), ValueTraj(ref, T)
    outs = {e: {k: e.alloc((T + 1, N, 4), np.uint32) for k in ("adv", "ret", "lp", "en")} for e in (env, ref)}
    sent = np.full((T + 1, N, 4), F32_SENT, np.uint32)

    def fill(e, t):
        t.fill()
        for o in outs[e].values():
            o.from_host(sent)

    def calls(e, t):
        t.vsets = vsets
        t.launch(e, sets, "sample", 13, 0)
        e.logprob_device(t.buf["logits"], t.buf["act"], outs[e]["lp"], outs[e]["en"], sets=sets, rows=T * N)
        e.gae_device(T, t.buf["rew"], t.buf["term"], t.buf["trunc"], t.values, outs[e]["adv"], outs[e]["ret"], gamma=GAMMA, lam=LAM)

    def fetch(e, t):
        got = t.get()
        for k, o in outs[e].items():
            h = o.to_host()
            assert (h[T] == F32_SENT).all(), f"{k}: a store went past the last row"
            got[k] = h[:T]
        return got

    fill(env, tr)
    for d, w in zip(dev, Wb + Vb):
        d.from_host(w)
    env.sync()
    cs = CallerStream(env)
    with cs.capture():
        env.load_policy(*dev[:4])
        env.load_value(*dev[4:])
        calls(env, tr)
    assert (env.get_state()[:, soa.W_T] == 0).all(), "capturing must not have stepped anything"
    ref.load_policy(*Wb)
    ref.load_value(*Vb)
    for k in range(2):                                             # replayed twice: the second replay goes on from the first one's state
        fill(env, tr)
        cs.replay()
        cs.sync()
        got = fetch(env, tr)
        fill(ref, rr)
        calls(ref, rr)
        ref.sync()
        eager = fetch(ref, rr)
        verify(f"replay {k}", orc, obs0, {n: got[n] for n in list(tr.buf) + ["values"]}, Wb, Vb, sets, vsets, "sample", 13, 0)
        obs0 = current_obs(orc)
        for name in got:
            assert np.array_equal(got[name], eager[name]), f"replay {k}: {name} differs from the eager launch"
        want_adv, want_ret = targets.host_gae(got["rew"].view(np.float64), got["term"], got["trunc"], got["values"].view(np.float32), GAMMA, LAM)
        assert np.array_equal(got["adv"], bits32(want_adv)) and np.array_equal(got["ret"], bits32(want_ret)), f"replay {k}: host_gae on the device's values"
        want_lp, want_en = targets.host_logprob(got["logits"].view(np.float32), got["act"])
        assert np.array_equal(got["lp"], bits32(want_lp)) and np.array_equal(got["en"], bits32(want_en)), f"replay {k}: host_logprob"
    assert np.array_equal(env.get_state(), ref.get_state()) and env.stats() == ref.stats()
    cs.close()
    env.close()
    ref.close()


def test_three_unequal_shards_equal_one_handle(monkeypatch):
    from cooking_zoo_amd import sharded
    n, A = 70, 4
    monkeypatch.setattr(sharded, "plan_shards", lambda num_envs, world_size, k: [(0, 37), (37, 30), (67, 3)])
    one = crowded(n)
    three = sharded.ShardedVecEnv(n, "crowded_6x5", "crowded_6x5", A, MAX_STEPS, CROWDED4, device_ids=[0, 0, 0], action_scheme="scheme1",
                                  num_layouts=8, auto_reset=True)
    try:
        assert [s.num_envs for s in three.shards] == [37, 30, 3]
        W, V = loaded(one)
        three.load_policy(*W)
        three.load_value(*V)
        assert three.value_sets == 2
        orc = VecOracle.from_vec_env(one)
        obs0 = start(one, orc)
        three.reset(return_obs=False)
        sets, vsets = sets_for(A), (1, 1, None, 0)
        got = ValueTraj(one, T).rollout(one, sets, "sample", 19, vsets=vsets)
        parts = ValueTraj(three, T, sharded=True).rollout(three, sets, "sample", 19, vsets=vsets)
        verify("one handle", orc, obs0, got, W, V, sets, vsets, "sample", 19)
        for k in got:
            assert np.array_equal(got[k], parts[k]), f"shards: {k}"
        assert np.array_equal(three.get_state(), one.get_state())
        # ... and cz_value_device over the shards' slices of the whole trajectory, [T + 1] * N rows in one call
        traj = np.concatenate([want32(obs0)[None], got["rows"]])
        x1, x3 = one.alloc((T + 1, n, A, one.F), np.uint32), three.alloc((A, one.F), np.uint32, leading=(T + 1,))
        v1, v3 = one.alloc((T + 1, n, A), np.uint32), three.alloc((A,), np.uint32, leading=(T + 1,))
        for x, v in ((x1, v1), (x3, v3)):
            x.from_host(traj)
            v.from_host(np.full((T + 1, n, A), SENTINEL, np.uint32))
        one.value_device(x1, v1, vsets=vsets, rows=(T + 1) * n)
        three.value_device(x3, v3, vsets=vsets)
        one.sync()
        three.sync()
        assert np.array_equal(v1.to_host(), got["values"]), "value_device on the trajectory gives the rollout's values"
        assert np.array_equal(v3.to_host(), got["values"]), "... over the shards as well"
        with pytest.raises(ValueError):
            three.value_device(x3, v3, vsets=vsets, rows=(T + 1) * n + 1)
    finally:
        one.close()
        three.close()
