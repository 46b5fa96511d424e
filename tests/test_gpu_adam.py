"""GPU: cz_adam_reserve and cz_adam_step_device (k_adam_norm, k_adam_finish, k_adam_update) against the numpy model of
cooking_zoo_amd/adam.py, as bits (zeros of either sign equal), on dense synthetic tensors.

The smallest shapes that can go wrong: F = 26 .. 128 with 8 actions (w1 segments of two to eight whole chunks), F = 283-like rows with
F % 4 == 3 and 5 actions (a remainder chunk, a last quad of the table with one padding entry, W2 rows past C never touched) and F = 639
(40 chunks a set); one to four loaded sets; masks of one set, all sets and a hole.  Conventions of the other device tests: GUARD
sentinel elements before and behind P, M, V and the state; every input finite and of ordinary scale unless the test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from cooking_zoo_amd import _native, adam, policy, ppo, targets
from adam_common import AdamCall, TableProbe, View, gradients, mid_state, same, tensors
from ppo_common import GUARD, canon, trajectory
from targets_common import GAMMA, LAM
from vec_common import CROWDED4, HUGE3, TWO, CallerStream, make_env as make

pytestmark = pytest.mark.gpu

HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.01, max_norm=0.5)
COEF = dict(clip=0.2, c_value=0.5, c_entropy=0.01)


def model_kw(hyper, lr=None):
    """CookingVecEnv.adam_step_device's keywords as host_adam_step's"""
    kw = {k: v for k, v in hyper.items() if k not in ("betas", "d_lr", "sets", "keep_table")}
    kw["beta1"], kw["beta2"] = hyper.get("betas", (0.9, 0.999))
    if lr is not None:
        kw["lr"] = lr
    return kw


def crowded(A=2, n=8):
    return make(n, "crowded_6x5", "crowded_6x5", A, CROWDED4[:A], "scheme1", max_steps=4, num_layouts=3)


def views(call, value=True):
    """the call's parameter buffers as load_policy / load_value take them"""
    return [View(call.P[i].ptr + 4 * GUARD, call.shapes[i]) for i in range(6 if value else 4)]


def load(env, call, value=True):
    v = views(call, value)
    env.load_policy(*v[:4])
    if value:
        env.load_value(*v[4:])


def mask_of(sets):
    return sum(1 << k for k in sets)


# (level, meta, agents, recipes, scheme, actions, loaded sets, the sets that take part, value tensors, max_norm, weight_decay, d_lr)
CASES = [("crowded_6x5", "crowded_6x5", 1, CROWDED4[:1], "scheme1", 8, 1, (0,), True, 0.5, 0.01, False),
         ("crowded_6x5", "crowded_6x5", 2, CROWDED4[:2], "scheme1", 8, 2, (0, 1), True, 0.0, 0.0, True),
         ("crowded_6x5", "crowded_6x5", 3, CROWDED4[:3], "scheme1", 8, 3, (0, 2), True, 0.5, 0.0, True),
         ("crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1", 8, 4, (2,), False, 0.0, 0.01, False),
         ("coop_test", "example_odd", 2, TWO, "scheme3", 5, 3, (0, 1, 2), True, 0.5, 0.01, True),
         ("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", 8, 2, (1,), True, 0.5, 0.0, False)]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[2]}agents-{c[6]}sets-mask{mask_of(c[7]):04b}" for c in CASES])
def test_three_steps_on_every_handle(case):
    """three consecutive calls with the state carried on the device: P, M, V and the state are the model's in bits after every call, the
    sets outside the mask byte for byte what they were, the table's logits and values the model's under the new parameters - and what an
    explicit load_policy + load_value of the updated buffers then gives"""
    level, meta, A, recipes, scheme, Cn, n, sets, value, max_norm, wd, by_pointer = case
    env = make(8, level, meta, A, recipes, scheme, max_steps=4, num_layouts=3)
    try:
        F = env.F
        assert env.num_actions == Cn and (A < 4 or F == 128) and (level != "coop_test" or F % 4 == 3) and (level != "huge_20x20" or F == 639)
        P, M, V = tensors(F, Cn, n, F + n, value)
        state = adam.fresh_state()
        state[7] = 12345.0                                         # never written
        call = AdamCall(env, P, gradients(F, Cn, n, 0, value), M, V, state)
        probe = TableProbe(env, F)
        load(env, call, value)
        env.adam_reserve()
        env.adam_reserve()                                         # idempotent
        before = probe.check("before", P, value)
        hyper = dict(HYPER, max_norm=max_norm, weight_decay=wd)
        want = (P, M, V, state)
        for k in range(3):
            G = gradients(F, Cn, n, 10 * F + k, value)
            lr = 3e-3 * (k + 1)
            call.set_grads(G)
            if by_pointer:
                call.set_lr(lr)
                call.launch(sets=sets, d_lr=call.lr, **dict(hyper, lr=99.0))
            else:
                call.launch(sets=sets, **dict(hyper, lr=lr))
            env.sync()
            want = adam.host_adam_step(want[0], G, want[1], want[2], want[3], mask_of(sets), **model_kw(hyper, lr))
            ctx = f"{level}, {A} agents, F = {F}, {n} sets, sets {sets}, step {k}"
            same(ctx, call.get(ctx), want)
            assert want[3][0] == k + 1 and want[3][6] == lr and want[3][7] == 12345.0 and (max_norm == 0) == (want[3][4] == 1.0)
            after = probe.check(ctx, want[0], value)
            for s in range(n):
                assert (s in sets) != np.array_equal(after[0][s], before[0][s]), f"{ctx}: set {s}'s logits moved or stayed against the mask"
        load(env, call, value)
        probe.check("after an explicit reload", want[0], value)
        if not value:                                              # no value tensors: the heads the table holds were not touched
            with pytest.raises(_native.NativeError, match="value head"):
                env.value_device(probe.d_x, probe.d_v, vsets=(0,) * A, rows=probe.R)
        probe.free()
        call.free()
    finally:
        env.close()


def test_every_mask_of_three_sets_and_a_kept_table():
    env = crowded(2)
    try:
        F, Cn, n = env.F, env.num_actions, 3
        P, M, V = tensors(F, Cn, n, 1)
        G = gradients(F, Cn, n, 1)
        probe = TableProbe(env, 2)
        env.adam_reserve()
        for mask in range(1, 8):
            sets = [k for k in range(3) if (mask >> k) & 1]
            call = AdamCall(env, P, G, M, V, mid_state())
            load(env, call)
            call.launch(sets=sets, **HYPER)
            env.sync()
            want = adam.host_adam_step(P, G, M, V, mid_state(), mask, **model_kw(HYPER))
            same(f"mask {mask:03b}", call.get(f"mask {mask:03b}"), want)
            probe.check(f"mask {mask:03b}", want[0])
            call.free()
        # keep_table: the arrays move, the table stays the old weights'
        call = AdamCall(env, P, G, M, V, mid_state())
        load(env, call)
        call.launch(keep_table=True, **HYPER)                      # sets=None: every loaded set
        env.sync()
        want = adam.host_adam_step(P, G, M, V, mid_state(), 7, **model_kw(HYPER))
        same("keep_table", call.get("keep_table"), want)
        probe.check("keep_table", P)
        load(env, call)
        probe.check("keep_table, then a reload", want[0])
        call.free()
        probe.free()
    finally:
        env.close()


def test_a_gradient_that_is_not_finite_skips_the_call_and_the_next_proceeds():
    env = crowded(2)
    try:
        F, Cn, n = env.F, env.num_actions, 2
        P, M, V = tensors(F, Cn, n, 4)
        G = gradients(F, Cn, n, 4)
        bad = [g.copy() for g in G]
        bad[0][1, 63, F - 1] = np.inf                              # the last element of the last chunk of w1
        call = AdamCall(env, P, bad, M, V, mid_state(4))
        probe = TableProbe(env, 3)
        load(env, call)
        env.adam_reserve()
        call.launch(**HYPER)
        env.sync()
        got = call.get("skip")
        for a, b in zip(got[0] + got[1] + got[2], P + M + V):
            assert a.tobytes() == b.tobytes(), "a skipped call moved something"
        st = got[3]
        assert st[5] == 1.0 and st[4] == 0.0 and np.array_equal(st[[0, 1, 2, 6, 7]], mid_state(4)[[0, 1, 2, 6, 7]]), st.tolist()
        probe.check("skip", P)
        want = adam.host_adam_step(P, bad, M, V, mid_state(4), 3, **model_kw(HYPER))
        assert np.array_equal(want[3][[0, 1, 2, 4, 5, 6, 7]], st[[0, 1, 2, 4, 5, 6, 7]])
        # only set 1 is poisoned: a call on set 0 alone does not read it
        call.launch(sets=(0,), **HYPER)
        env.sync()
        state = st.copy()
        want = adam.host_adam_step(P, bad, M, V, state, 1, **model_kw(HYPER))
        same("set 0 alone", call.get("set 0 alone"), want)
        # the next finite call proceeds from t
        call.set_grads(G)
        call.launch(**HYPER)
        env.sync()
        want = adam.host_adam_step(want[0], G, want[1], want[2], want[3], 3, **model_kw(HYPER))
        same("after the skip", call.get("after the skip"), want)
        assert want[3][0] == 6.0 and want[3][5] == 1.0
        probe.check("after the skip", want[0])
        probe.free()
        call.free()
    finally:
        env.close()


def test_refusals_write_nothing():
    env = crowded(2)
    try:
        lib = _native.lib()
        assert lib.cz_adam_chunk() == adam.ADAM_CHUNK == 1024 and lib.cz_sizeof_params() == C.sizeof(_native.CzParams)
        F, Cn, n = env.F, env.num_actions, 3
        P, M, V = tensors(F, Cn, n, 5)
        call = AdamCall(env, P, gradients(F, Cn, n, 5), M, V, mid_state())
        first = call.get("start")
        run = lambda **kw: call.launch(**{**HYPER, **kw})

        def refused(message, fn):
            with pytest.raises(_native.NativeError, match=message):
                fn()
            env.sync()
            got = call.get(message)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0] + got[1] + got[2], first[0] + first[1] + first[2])) and \
                got[3].tobytes() == first[3].tobytes(), f"a refused call ({message}) wrote something"

        refused("no weight table loaded", run)
        v = views(call)
        env.load_policy(*v[:4])
        refused("no partials reserved", run)
        cs = CallerStream(env)
        with cs.capture():
            env.load_policy(*v[:4])
            with pytest.raises(_native.NativeError, match="outside the capture"):
                env.adam_reserve()                                 # (the first call allocates)
        cs.close()
        refused("no partials reserved", run)
        env.adam_reserve()
        refused("set_mask is empty", lambda: run(sets=()))
        refused("names a set past the 3 loaded", lambda: run(sets=(0, 3)))
        refused("past the 0 value heads loaded", run)
        env.load_value(View(v[4].ptr, (2, 64)), View(v[5].ptr, (2, 1)))
        refused("past the 2 value heads loaded", lambda: run(sets=(1, 2)))
        groups = [list(g) for g in call.groups()]
        state = call.state.ptr + 8 * GUARD

        def raw(groups=groups, mask=0b011, state=state, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, max_norm=0.0, flags=0, null_group=None):
            structs = [_native.CzParams(*g) for g in groups]
            refs = [None if k == null_group else C.byref(s) for k, s in enumerate(structs)]
            _native.check(env._h, lib.cz_adam_step_device(env._h, mask, *refs, state, lr, None, b1, b2, eps, wd, max_norm, flags))

        for k in range(4):
            refused("a group or the state pointer is null", lambda: raw(null_group=k))
            for i in range(4):
                g = [list(x) for x in groups]
                g[k][i] = None
                refused("a pointer of the policy's four tensors is null", lambda: raw(groups=g))
            for i in (4, 5):                                       # the value pointers: in all four groups or in none
                g = [list(x) for x in groups]
                g[k][i] = None
                refused("in all four groups or in none; 7 of 8", lambda: raw(groups=g))
        refused("a group or the state pointer is null", lambda: raw(state=None))
        for bad in (-1e-3, float("nan")):
            refused("lr is", lambda: raw(lr=bad))
            refused("weight_decay is", lambda: raw(wd=bad))
            refused("max_norm is", lambda: raw(max_norm=bad))
            refused("eps is", lambda: raw(eps=bad))
        refused("eps is", lambda: raw(eps=0.0))
        for bad in (-0.1, 1.0, 1.5, float("nan")):
            refused("beta1 is", lambda: raw(b1=bad))
            refused("beta2 is", lambda: raw(b2=bad))
        refused("unknown flag bits 0x6", lambda: raw(flags=6))
        with pytest.raises(ValueError, match="holds 5 buffers"):
            env.adam_step_device(groups[0][:5], groups[1], groups[2], groups[3], state)
        # what is legal at the edges: beta 0, a set past the value heads with the table kept, no value tensors at all
        raw(mask=0b100, flags=_native.CZ_ADAM_KEEP_TABLE, b1=0.0, b2=0.0)
        raw(groups=[g[:4] + [None, None] for g in groups], mask=0b100)
        env.sync()
        call.free()
    finally:
        env.close()


def test_gradient_and_optimiser_from_a_callers_graph():
    """ppo_grad_device + adam_step_device as one captured minibatch step, replayed three times with the index and *d_lr changed
    between replays: parameters, moments and state byte for byte the eager run's, and the chained numpy models'"""
    env = crowded(2)
    try:
        F, Cn, n, A = env.F, env.num_actions, 2, 2
        P, M, V = tensors(F, Cn, n, 6)
        zero = [np.zeros_like(p) for p in P]
        R, mb, sets, vsets = 96, 40, (0, 1), (0, 0)
        data = trajectory(R, A, F, P[:4], sets, 6)
        bufs = []
        for v, t in zip(data, (np.float32, np.int32, np.float32, np.float32, np.float32)):
            b = env.alloc(v.shape, t)
            b.from_host(v)
            bufs.append(b)
        d_index = env.alloc((mb,), np.int32)
        indices = [np.random.default_rng(k).integers(0, R, mb).astype(np.int32) for k in range(3)]
        lrs = (1e-2, 5e-3, 2.5e-3)
        hyper = dict(HYPER, lr=0.0)
        call = AdamCall(env, P, zero, zero, zero, adam.fresh_state())
        env.adam_reserve()

        def restart():
            for dev, host in ((call.P, P), (call.M, zero), (call.V, zero)):
                for i in range(6):
                    call.put(dev[i], host[i])
            call.set_state(adam.fresh_state())
            load(env, call)
            env.ppo_reserve(mb)

        def step():
            env.ppo_grad_device(*bufs, [call.G[i] for i in range(6)], d_index=d_index, sets=sets, vsets=vsets, rows=R, **COEF)
            call.launch(d_lr=call.lr, **hyper)

        restart()
        want = (P, zero, zero, adam.fresh_state())
        for k in range(3):
            d_index.from_host(indices[k])
            call.set_lr(lrs[k])
            step()
            env.sync()
            G = ppo.host_ppo_grad(*data, want[0][:4], want[0][4:], sets, vsets, index=indices[k], **COEF)[0]
            want = adam.host_adam_step(want[0], G, want[1], want[2], want[3], 3, **model_kw(hyper, lrs[k]))
        eager = call.get("eager")
        same("eager against the chained models", eager, want)
        assert want[3][0] == 3.0 and min(want[3][4], 1.0) > 0
        restart()
        env.sync()
        cs = CallerStream(env)
        with cs.capture():
            step()
        got = call.get("capture")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], P)) and got[3][0] == 0.0, "capturing must not have launched anything"
        for k in range(3):
            d_index.from_host(indices[k])
            call.set_lr(lrs[k])
            cs.replay()
            cs.sync()
        got = call.get("replays")
        for a, b in zip(got[0] + got[1] + got[2] + [got[3]], eager[0] + eager[1] + eager[2] + [eager[3]]):
            assert a.tobytes() == b.tobytes(), "the graph's replays differ from the eager calls"
        cs.close()
        TableProbe(env, 9).check("after the replays", want[0])
        call.free()
    finally:
        env.close()


def test_two_minibatch_updates_on_the_devices_own_trajectory():
    """rollout_policy_value -> logprob_device -> gae_device -> twice (ppo_grad_device -> adam_step_device) at 48 envs, T = 4, against
    the chained numpy models: no torch, no host between the calls"""
    n, T, A, ns = 48, 4, 2, 2
    env = make(n, "coop_test", "example", A, TWO, "scheme3", max_steps=3, num_layouts=3)
    try:
        F, Cn = env.F, env.num_actions
        P, M, V = tensors(F, Cn, ns, 11)
        zero = [np.zeros_like(p) for p in P]
        call = AdamCall(env, P, zero, zero, zero, adam.fresh_state())
        load(env, call)
        env.reset(return_obs=False)
        sets, vsets = (0, 1), (0, 0)
        b = dict(obs=env.alloc((T + 1, n, A, F), np.float32), act=env.alloc((T, n, A), np.int32), logits=env.alloc((T, n, A, Cn), np.float32),
                 rew=env.alloc((T, n, A), np.float64), term=env.alloc((T, n, A), np.uint8), trunc=env.alloc((T, n, A), np.uint8),
                 val=env.alloc((T + 1, n, A), np.float32), logp=env.alloc((T, n, A), np.float32), adv=env.alloc((T, n, A), np.float32),
                 ret=env.alloc((T, n, A), np.float32), before=env.alloc((T, n, A, F), np.float32))
        rows1 = env.alloc((T, n, A, F), np.float32)
        env.observe_device(d_obs32=b["obs"])
        env.rollout_policy_value(T, rows1, b["val"], b["act"], b["logits"], b["rew"], b["term"], b["trunc"], sets=sets, vsets=vsets, mode="sample", seed=5)
        env.logprob_device(b["logits"], b["act"], b["logp"], sets=sets, rows=T * n)
        env.gae_device(T, b["rew"], b["term"], b["trunc"], b["val"], b["adv"], b["ret"], gamma=GAMMA, lam=LAM)
        env.sync()
        before = np.concatenate([b["obs"].to_host()[:1], rows1.to_host()[:T - 1]]).reshape(T * n, A, F)      # the row in front of every step
        b["before"].from_host(before.reshape(T, n, A, F))
        data = (before, b["act"].to_host().reshape(T * n, A), b["logp"].to_host().reshape(T * n, A), b["adv"].to_host().reshape(T * n, A),
                b["ret"].to_host().reshape(T * n, A))
        R, mb = T * n, T * n // 2
        perm = np.random.default_rng(12).permutation(R).astype(np.int32)
        d_index = [env.alloc((mb,), np.int32) for _ in range(2)]
        for k in range(2):
            d_index[k].from_host(perm[k * mb:(k + 1) * mb])
        env.ppo_reserve(mb)
        env.adam_reserve()
        hyper = dict(HYPER, lr=1e-2)
        for k in range(2):                                         # four calls in a row, no wait in between
            env.ppo_grad_device(b["before"], b["act"], b["logp"], b["adv"], b["ret"], [call.G[i] for i in range(6)], d_index=d_index[k],
                                sets=sets, vsets=vsets, rows=R, **COEF)
            call.launch(**hyper)
        env.sync()
        want = (P, zero, zero, adam.fresh_state())
        for k in range(2):
            G, stats = ppo.host_ppo_grad(*data, want[0][:4], want[0][4:], sets, vsets, index=perm[k * mb:(k + 1) * mb], **COEF)
            assert k == 1 or stats[3] == 0.0, "the first minibatch runs on the weights that played: the ratio is 1"
            want = adam.host_adam_step(want[0], G, want[1], want[2], want[3], 3, **model_kw(hyper))
        same("two minibatches", call.get("two minibatches"), want)
        assert want[3][0] == 2.0 and 0.0 < want[3][4] <= 1.0 and not np.array_equal(want[0][0], P[0])
        TableProbe(env, 13).check("two minibatches", want[0])
        call.free()
    finally:
        env.close()
