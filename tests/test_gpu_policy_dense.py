"""GPU: the device policy where test_gpu_policy.py's inputs leave it unobserved - dense rows at every row tail (every column of W1
reaches a logit; observation rows are zero in about half their features and in the whole last quad of most tails), all four weight
sets and a shrinking and growing `n_sets`, the fused rollout on sets 2 and 3, chosen logits (all equal, tied, beyond the clamp,
overwhelming, a dead hidden layer) with cz_logprob_device on what the device wrote, and global env ids beyond 32 bits.

Every comparison is bit for bit against policy.host_logits / host_actions and targets.host_logprob.  Conventions of
test_gpu_policy.py: a sentinel in every output before every launch, a guard row behind each buffer, float32 compared as uint32.
Every condition that makes a case able to fail is computed on the model and asserted BEFORE the launch it protects.  Every input is
finite and of ordinary scale."""
import numpy as np
import pytest

from cooking_zoo_amd import _native, policy, targets
from oracle_binding import VecOracle
from policy_common import (ACT_SENT, PolicyTraj, check_policy, dense_conditions, dense_rows, exact_logit_weights, expected_policy, logit_cases,
                           logits_per_set, stack_sets, start, stream_actions, verify_rollout, weights)
from targets_common import F32_SENT, bits32
from vec_common import CROWDED4, HUGE3, SENTINEL, TWO, instance, make_env as make, strip, want32

pytestmark = pytest.mark.gpu

N, T, MAX_STEPS = 35, 5, 3
BIG_BASE = 2 ** 33 + 7


def crowded(n=N, scheme="scheme1", **kw):
    args = dict(max_steps=MAX_STEPS)
    args.update(kw)
    return make(n, "crowded_6x5", "crowded_6x5", 4, CROWDED4, scheme, **args)


def loaded(env, n_sets=4, seed=0):
    W = weights(env.F, env.num_actions, n_sets, seed, scale2=0.03)
    env.load_policy(*W)
    assert env.policy_sets == n_sets
    return W


class PolicyCall:
    """cz_policy_device on rows of the caller: the rows with a guard row of the NaN sentinel directly behind the last one (the
    features behind F of the last agent's row are NaN in memory), sentinel-filled outputs with a guard row each"""

    def __init__(self, env, x):
        self.env, self.n, self.A = env, len(x), env.num_agents
        Cn = env.num_actions
        self.d_x = env.alloc((self.n + 1,) + x.shape[1:], np.uint32)
        self.d_x.from_host(np.concatenate([np.ascontiguousarray(x).view(np.uint32), np.full((1,) + x.shape[1:], SENTINEL, np.uint32)]))
        self.d_act, self.d_lg = env.alloc((self.n + 1, self.A), np.int32), env.alloc((self.n + 1, self.A, Cn), np.uint32)
        self.fills = (np.full((self.n + 1, self.A), ACT_SENT, np.int32), np.full((self.n + 1, self.A, Cn), SENTINEL, np.uint32))

    def fill(self):
        self.d_act.from_host(self.fills[0])
        self.d_lg.from_host(self.fills[1])

    def launch(self, **kw):
        self.env.policy_device(self.d_x, self.d_act, self.d_lg, env_count=self.n, **kw)

    def get(self, ctx):
        """-> {"act": [1][n][A], "logits": [1][n][A][C]} for check_policy; asserts the guard rows"""
        act, lg = self.d_act.to_host(), self.d_lg.to_host()
        assert (act[self.n] == ACT_SENT).all() and (lg[self.n] == SENTINEL).all(), f"{ctx}: a store went past the last row"
        return dict(act=act[None, :self.n], logits=lg[None, :self.n])

    def run(self, ctx, **kw):
        self.fill()
        self.launch(**kw)
        self.env.sync()
        return self.get(ctx)

    def free(self):
        for b in (self.d_x, self.d_act, self.d_lg):
            b.free()


# ---------------------------------------------------------------------------------------------------------------------------
# A. dense rows through cz_policy_device, at every row tail, on all four sets
# ---------------------------------------------------------------------------------------------------------------------------

DENSE = [("crowded_6x5", "crowded_6x5", a, CROWDED4[:a], "scheme1", None, 8, 0) for a in (1, 2, 3, 4)] + \
        [("coop_test", meta, 2, TWO, "scheme3", F, 5, 0) for meta, F in (("example", 278), ("example_odd", 283), ("example_f384", 384),
                                                                          ("example_f385", 385), ("example_f513", 513))] + \
        [("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", 639, 8, 2)]
DENSE_ENVS = 9                                                  # k_policy runs one wavefront per env


@pytest.mark.parametrize("case", DENSE, ids=[f"{c[0]}-{c[1]}-{c[2]}agents" for c in DENSE])
def test_dense_rows_on_every_set_at_every_tail(case):
    level, meta, A, recipes, scheme, F, Cn, inst = case
    n = DENSE_ENVS
    env = make(n, level, meta, A, recipes, scheme, max_steps=4, num_layouts=3)
    try:
        assert (F is None or env.F == F) and env.num_actions == Cn and instance(env) == inst
        assert A < 4 or env.F == 128, "crowded_6x5 with four agents has no row tail"
        F = env.F
        ctx = f"{level} / {meta}, {A} agents, F = {F}"
        W = weights(F, Cn, 4, F + A, scale2=0.03)
        x = dense_rows(n, A, F, F + A)
        per_set = logits_per_set(x[None], W)                   # [4] of [1][n][A][C]: the model, once for every launch below
        share = dense_conditions(ctx, x, W, per_set)
        print(f"{ctx}: {share:.1%} of the expected logits differ from the matrix-product form")
        env.load_policy(*W)
        assert env.policy_sets == 4
        whole = PolicyCall(env, x)
        none = np.full((1, n, A), ACT_SENT, np.int32)

        def check(call, what, sets, mode, seed, step, begin, count):
            got = call.run(f"{ctx}, {what}", sets=sets, mode=mode, seed=seed, step=step, env_begin=begin)
            want_a, want_l, mask = expected_policy(x[None, begin:begin + count], W, sets, mode, seed, step, none[:, :count], env_id_base=begin,
                                                   per_set=[p[:, begin:begin + count] for p in per_set])
            assert mask.sum() == sum(s is not None for s in sets)
            check_policy(f"{ctx}, {what}", got, want_a, want_l, mask)      # (an agent without a set: the "stream" is the sentinel)

        for r in range(4):                                      # every agent position uses every set
            sets = tuple((a + r) % 4 for a in range(A))
            for mode in ("greedy", "sample"):
                check(whole, f"sets {sets} {mode}", sets, mode, 9 + r, 17 + r, 0, n)
            holed = tuple(None if a == r % A else s for a, s in enumerate(sets))
            check(whole, f"sets {holed}", holed, "sample", 19 + r, 3 * r, 0, n)
        whole.free()
        for k, (begin, count) in enumerate(((n - 1, 1), (2, 5), (n - 3, 3))):
            part = PolicyCall(env, x[begin:begin + count])
            sets = tuple((a + 3 - k) % 4 for a in range(A))
            check(part, f"envs [{begin}, {begin + count})", sets, "sample", 31, 5, begin, count)
            part.free()
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# B. the life of n_sets: 4, then 1, then 3
# ---------------------------------------------------------------------------------------------------------------------------

def loads_of(env):
    """three loads of 4, 1 and 3 sets whose logits on the dense rows differ from each other's in every row and set: nothing of an
    earlier load can pass for a later one's"""
    x = dense_rows(DENSE_ENVS, 4, env.F, 77)
    Ws = [weights(env.F, env.num_actions, k, 40 + k, scale2=0.03) for k in (4, 1, 3)]
    models = [logits_per_set(x[None], W) for W in Ws]
    flat = [bits32(p).reshape(-1, env.num_actions) for m in models for p in m]
    for i in range(len(flat)):
        for j in range(i):
            assert (flat[i] != flat[j]).any(axis=-1).all(), f"sets {j} and {i} of the three loads give a row the same logits: the case shows nothing"
    return x, Ws, models


def test_n_sets_shrinks_and_grows():
    env = crowded(DENSE_ENVS)
    x, (W4, W1, W3), (m4, m1, m3) = loads_of(env)
    call = PolicyCall(env, x)
    none = np.full((1, DENSE_ENVS, 4), ACT_SENT, np.int32)

    def gives(what, W, model, sets):
        for mode in ("greedy", "sample"):
            got = call.run(what, sets=sets, mode=mode, seed=3, step=8)
            check_policy(f"{what}, sets {sets} {mode}", got, *expected_policy(x[None], W, sets, mode, 3, 8, none, per_set=model))

    def refused(message, sets):
        call.fill()
        with pytest.raises(_native.NativeError, match=message):
            call.launch(sets=sets)
        env.sync()
        got = call.get(message)
        assert (got["act"] == ACT_SENT).all() and (got["logits"] == SENTINEL).all(), f"a refused call ({message}) wrote something"

    env.load_policy(*W4)
    assert env.policy_sets == 4
    gives("4 sets loaded", W4, m4, (3, 2, 1, 0))
    env.load_policy(*W1)
    assert env.policy_sets == 1
    refused("weight set 1, but 1 are loaded", (0, 1, 0, 0))
    refused("weight set 3, but 1 are loaded", (0, 0, 0, 3))
    gives("1 set loaded behind 4", W1, m1, (0, 0, None, 0))
    env.load_policy(*W3)
    assert env.policy_sets == 3
    refused("weight set 3, but 3 are loaded", (0, 1, 2, 3))
    gives("3 sets loaded behind 1", W3, m3, (2, 1, 0, 2))
    gives("3 sets loaded behind 1", W3, m3, (0, 2, None, 1))
    env.close()


def test_n_sets_shrinks_and_grows_behind_launches_without_a_wait():
    env = crowded(DENSE_ENVS)
    x, Ws, models = loads_of(env)
    dev = [[env.alloc(w.shape, np.float32) for w in W] for W in Ws]
    for bufs, W in zip(dev, Ws):
        for b, w in zip(bufs, W):
            b.from_host(w)
    calls = [PolicyCall(env, x) for _ in Ws]
    for c in calls:
        c.fill()
    plans = [(3, 2, 1, 0), (0, 0, 0, 0), (2, 1, 0, 2)]
    for k, (c, sets) in enumerate(zip(calls, plans)):              # six stream-ordered calls, no wait in between
        env.load_policy(*dev[k])
        c.launch(sets=sets, mode="sample", seed=6, step=k)
    assert env.policy_sets == 3
    env.sync()
    none = np.full((1, DENSE_ENVS, 4), ACT_SENT, np.int32)
    for k, (c, sets) in enumerate(zip(calls, plans)):
        check_policy(f"load {k} of {len(Ws[k][0])} sets, sets {sets}", c.get(f"load {k}"),
                     *expected_policy(x[None], Ws[k], sets, "sample", 6, k, none, per_set=models[k]))
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# C. the fused rollout on sets 2 and 3
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("sets", [(3, 2, 1, 0), (2, None, 3, 2)], ids=lambda s: "-".join(str(v) for v in s))
def test_rollout_on_sets_two_and_three(sets, mode):
    env = crowded()
    W = loaded(env, 4, 8)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    got = PolicyTraj(env, T).rollout(env, sets, mode, 23, step0=1)
    recs = verify_rollout(f"sets {sets} {mode}", orc, obs0, got, W, sets, mode, 23, step0=1)
    assert np.array_equal(strip(env.get_state()), recs[-1]), "records after the launch"
    env.close()


def test_rollout_on_sets_two_and_three_huge_instance():
    env = make(N, "huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", max_steps=MAX_STEPS, num_layouts=3)
    assert env.F == 639 and instance(env) == 2
    W = loaded(env, 4, 9)
    orc = VecOracle.from_vec_env(env)
    obs0 = start(env, orc)
    sets = (3, None, 2)
    got = PolicyTraj(env, T).rollout(env, sets, "sample", 29)
    recs = verify_rollout(f"huge_20x20, sets {sets}", orc, obs0, got, W, sets, "sample", 29)
    assert np.array_equal(strip(env.get_state()), recs[-1]), "records after the launch"
    env.close()


def test_rollout_on_four_sets_is_t_times_policy_device_and_step_device_f32():
    fused, twin = crowded(), crowded()
    W = loaded(fused, 4, 10)
    twin.load_policy(*W)
    orc = VecOracle.from_vec_env(fused)
    obs0 = start(fused, orc)
    twin.reset(return_obs=False)
    sets, seed, step0, T_ = (3, 2, 1, 0), 11, 4, T
    got = PolicyTraj(fused, T_).rollout(fused, sets, "sample", seed, step0)
    verify_rollout("fused", orc, obs0, got, W, sets, "sample", seed, step0)
    A, F, Cn = 4, twin.F, twin.num_actions
    rows = [twin.alloc((N, A, F), np.uint32) for _ in range(2)]
    d_act, d_lg = twin.alloc((N, A), np.int32), twin.alloc((N, A, Cn), np.uint32)
    d_rew, d_term, d_trunc = twin.alloc((N, A), np.uint64), twin.alloc((N, A), np.uint8), twin.alloc((N, A), np.uint8)
    twin.observe_device(d_obs32=rows[0])
    assert np.array_equal(rows[0].to_host(), want32(obs0)), "row 0 comes from observe_device"
    for t in range(T_):
        d_act.from_host(np.full((N, A), ACT_SENT, np.int32))      # every agent has a set: every entry is written
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
# D. chosen logits on the device, and cz_logprob_device on what the device wrote
# ---------------------------------------------------------------------------------------------------------------------------

STEPS = (0, 17, 4_000_000_000)


def case_conditions(name, L, acts, logp):
    """`acts` int32 [steps][n][A], `logp` float32 like it: the model's sampled actions and their log-probabilities on logits `L`"""
    Cn, top = len(L), np.flatnonzero(L == L.max())
    counts = np.bincount(acts.ravel(), minlength=Cn)
    if name == "flat":
        assert (np.bincount(acts[1].ravel(), minlength=Cn) > 0).all(), "flat: an action never occurs among the draws of one step: the case shows nothing"
    if name == "dead":
        assert (counts > 0).all(), "dead: an action never occurs among the draws: the case shows nothing"
    if name == "tie3":
        assert len(top) == 3 and top[-1] == Cn - 1 and (counts[top] > 0).all(), "tie3: a tied action never occurs: the case shows nothing"
        assert counts.sum() > counts[top].sum(), "tie3: no draw falls beyond the tied actions: the case shows nothing"
    if name == "clamp":
        z = np.sort(L.astype(np.float64) - float(L.max()))
        assert z[0] <= -1000.0 and -1000.0 < z[1] <= -64.0, "clamp: not one logit 70 and one 1000 below the maximum"
        assert len(np.unique(acts)) >= 3, "clamp: the draws barely vary: the case shows nothing"
    if name == "one":
        assert (acts == int(top[0])).all() and top[0] not in (0, Cn - 1), "one: a draw misses the overwhelming action"
        assert (bits32(logp) == 0).all(), "one: the log-probability of the overwhelming action is not 0.0 with all bits zero"
    else:
        assert (logp < 0).all(), f"{name}: a log-probability is not negative"


@pytest.mark.parametrize("Cn,scheme", [(5, "scheme3"), (8, "scheme1")], ids=["C5", "C8"])
def test_chosen_logits_sampling_and_logprob_of_the_devices_own_outputs(Cn, scheme):
    env = crowded(scheme=scheme)
    assert env.num_actions == Cn
    A, F = 4, env.F
    cases = logit_cases(Cn)
    x = dense_rows(N, A, F, Cn)
    call = PolicyCall(env, x)
    lp, en = env.alloc((N + 1, A), np.uint32), env.alloc((N + 1, A), np.uint32)
    env_ids = np.arange(N, dtype=np.uint64)[None, :, None]
    steps = np.array(STEPS, np.uint64)[:, None, None]
    agents = np.arange(A)[None, None, :]
    names = list(cases)
    for first in range(0, len(names), policy.MAX_SETS):             # up to four cases per load, one set each
        chunk = names[first:first + policy.MAX_SETS]
        W = stack_sets([exact_logit_weights(F, *cases[name]) for name in chunk])
        model = logits_per_set(x[None], W)
        want = {}
        for si, name in enumerate(chunk):                           # every condition before the first launch
            L = cases[name][0]
            assert (bits32(model[si]) == bits32(L)).all(), f"{name}: the model's logits are not L in bits"
            acts = policy.host_actions(np.broadcast_to(L, (len(STEPS), N, A, Cn)), "sample", 9, env_ids, steps, agents)
            logp, ent = targets.host_logprob(np.broadcast_to(L, (len(STEPS), N, A, Cn)), acts)
            case_conditions(name, L, acts, logp)
            want[name] = (acts, logp, ent)
        env.load_policy(*W)
        assert env.policy_sets == len(chunk)
        for si, name in enumerate(chunk):
            L, sets = cases[name][0], (si,) * A
            greedy = call.run(f"{name} greedy", sets=sets, mode="greedy", seed=9, step=17)
            assert (greedy["logits"] == bits32(L)).all(), f"{name}: the device's logits are not L in bits"
            assert (greedy["act"] == int(L.argmax())).all(), f"{name}: greedy does not take the first of the largest logits"
            for k, step in enumerate(STEPS):
                ctx = f"C = {Cn}, {name}, step {step}"
                got = call.run(ctx, sets=sets, mode="sample", seed=9, step=step)
                assert (got["logits"] == bits32(L)).all(), f"{ctx}: the device's logits are not L in bits"
                bad = np.argwhere(got["act"][0] != want[name][0][k])
                assert not len(bad), f"{ctx}: actions differ from host_actions at (env, agent) {bad[:6].tolist()}"
                for out in (lp, en):
                    out.from_host(np.full((N + 1, A), F32_SENT, np.uint32))
                env.logprob_device(call.d_lg, call.d_act, lp, en, sets=sets, rows=N)      # the device's own logits and actions
                env.sync()
                for out, w, what in ((lp, want[name][1][k], "logp"), (en, want[name][2][k], "entropy")):
                    g = out.to_host()
                    assert (g[N] == F32_SENT).all(), f"{ctx}: a store went past the last row of {what}"
                    bad = np.argwhere(g[:N] != bits32(w))
                    assert not len(bad), f"{ctx}: {what} of the device's own outputs differs in bits at (env, agent) {bad[:6].tolist()}"
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# E. global env ids beyond 32 bits
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_draw_is_keyed_by_all_64_bits_of_the_global_env_id():
    env = crowded(env_id_base=BIG_BASE)
    A, F, Cn = 4, env.F, env.num_actions
    flat = stack_sets([exact_logit_weights(F, logit_cases(Cn)["flat"][0])])
    x = dense_rows(N, A, F, 5)
    none = np.full((1, N, A), ACT_SENT, np.int32)
    model = logits_per_set(x[None], flat)
    sets = (0, 0, 0, 0)
    want = expected_policy(x[None], flat, sets, "sample", 9, 17, none, env_id_base=BIG_BASE, per_set=model)
    low = expected_policy(x[None], flat, sets, "sample", 9, 17, none, env_id_base=BIG_BASE & 0xFFFFFFFF, per_set=model)
    other = int((want[0] != low[0]).sum())
    assert 4 * other >= N * A, f"only {other} of {N * A} draws differ from those of the id's low 32 bits: the case shows nothing"
    env.load_policy(*flat)
    call = PolicyCall(env, x)
    check_policy("flat logits, whole range", call.run("whole range", sets=sets, mode="sample", seed=9, step=17), *want)
    call.free()
    begin, count = N - 4, 4                                        # ... and with an env_begin on top of the base
    part = PolicyCall(env, x[begin:])
    want = expected_policy(x[None, begin:], flat, sets, "sample", 9, 17, none[:, :count], env_id_base=BIG_BASE + begin,
                           per_set=[p[:, begin:] for p in model])
    check_policy("flat logits, the last four envs", part.run("last four", sets=sets, mode="sample", seed=9, step=17, env_begin=begin), *want)
    part.free()
    # the fused rollout: the oracle's layout rotation and action stream, the device's, and the draws, all at such ids
    W = loaded(env, 2, 12)
    orc = VecOracle.from_vec_env(env)
    assert orc.env_id_base == BIG_BASE
    obs0 = start(env, orc)
    rsets = (1, 0, None, 0)
    low = VecOracle.from_vec_env(env, env_id_base=BIG_BASE & 0xFFFFFFFF)
    low.reset()
    assert (stream_actions(orc, 3, 41, 0) != stream_actions(low, 3, 41, 0)).any(), \
        "the action stream at the id's low 32 bits is the same: the stream agent shows nothing"
    got = PolicyTraj(env, 3).rollout(env, rsets, "sample", 41)
    recs = verify_rollout("rollout at ids beyond 2^33", orc, obs0, got, W, rsets, "sample", 41)
    assert np.array_equal(strip(env.get_state()), recs[-1]), "records after the launch"
    env.close()
