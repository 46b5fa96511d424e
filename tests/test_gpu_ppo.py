"""GPU: cz_ppo_reserve and cz_ppo_grad_device (k_ppo_forward, k_ppo_outer, k_ppo_reduce) against the numpy model of
cooking_zoo_amd/ppo.py, as bits (zeros of either sign equal), on dense rows.

The smallest shapes that can go wrong: 1, 63, 64, 65 and 130 positions (the chunk edges and a third, partial chunk); A = 1 .. 4; F =
128 (no row tail), 283 (F % 4 != 0) and 639 (twenty feature tiles, the last one a remainder of 31); C = 5 and 8.  Conventions of the
other device tests: a sentinel in every output before every launch and GUARD sentinel elements before and behind each; every input
finite and of ordinary scale."""
import numpy as np
import pytest

from cooking_zoo_amd import _native, policy, ppo, targets
from policy_common import weights
from ppo_common import STAT_SENT, PpoCall, canon, check_grads, trajectory
from targets_common import F32_SENT, GAMMA, LAM
from value_common import value_weights
from vec_common import CROWDED4, HUGE3, TWO, CallerStream, make_env as make

pytestmark = pytest.mark.gpu

POSITIONS = (1, 63, 64, 65, 130)
COEF = dict(clip=0.2, c_value=0.5, c_entropy=0.01)


def crowded(A=4, n=8):
    return make(n, "crowded_6x5", "crowded_6x5", A, CROWDED4[:A], "scheme1", max_steps=4, num_layouts=3)


def loaded(env, n_sets, seed):
    W, V = weights(env.F, env.num_actions, n_sets, seed, scale2=0.3), value_weights(n_sets, seed)
    env.load_policy(*W)
    env.load_value(*V)
    return W, V


def model(data, W, V, sets, vsets, index=None, **kw):
    coef = dict(COEF)
    coef.update(kw)
    return ppo.host_ppo_grad(*data, W, V, sets, sets if vsets is None else vsets, index=index, **coef)


CASES = [("crowded_6x5", "crowded_6x5", a, CROWDED4[:a], "scheme1", 8) for a in (1, 2, 3, 4)] + \
        [("coop_test", "example_odd", 2, TWO, "scheme3", 5), ("huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", 8)]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[2]}agents" for c in CASES])
def test_every_chunk_edge_on_every_handle(case):
    """whole trajectories of 1 .. 130 rows with no index: agent 0 on a shared trunk, the next one with a critic of its own, the
    last of three or four without a policy or without anything"""
    level, meta, A, recipes, scheme, Cn = case
    env = make(8, level, meta, A, recipes, scheme, max_steps=4, num_layouts=3)
    try:
        F = env.F
        assert env.num_actions == Cn and (A < 4 or F == 128) and (level != "coop_test" or F % 4 == 3) and (level != "huge_20x20" or F == 639)
        W, V = loaded(env, 3, F + A)
        sets = ((0,), (0, 1), (0, 1, None), (0, 1, None, None))[A - 1]
        vsets = ((0,), (0, 2), (0, 2, 2), (0, 2, 1, None))[A - 1]
        assert env.ppo_reserve(max(POSITIONS)) == max(POSITIONS)
        seen = np.zeros(8)
        for R in POSITIONS:
            data = trajectory(R, A, F, W, sets, F + R)
            call = PpoCall(env, data, 3)
            want = model(data, W, V, sets, vsets)
            check_grads(f"{level}, {A} agents, F = {F}, {R} rows", call.run(f"{R} rows", sets=sets, vsets=vsets, **COEF), want)
            seen = np.maximum(seen, want[1])
            call.free()
        assert seen[4] > 0 and seen[5] > 0 and seen[6] > 0, f"no clipped ratio, policy part or value part in any case: {seen}"
    finally:
        env.close()


@pytest.mark.parametrize("tile", (16, 32, 64))
def test_every_k_ppo_outer_instance_the_library_carries(monkeypatch, tile):
    """CZ_PPO_TILE is read when a handle is made: F = 639 leaves every tile a remainder (15, 31, 63 features) behind several whole
    ones; the bits do not depend on the tile"""
    monkeypatch.setenv("CZ_PPO_TILE", str(tile))
    env = make(8, "huge_20x20", "huge_20x20", 3, HUGE3, "scheme1", max_steps=4, num_layouts=3)
    try:
        W, V = loaded(env, 2, tile)
        sets, vsets, R = (0, 1, None), (0, 0, 1), 70
        data = trajectory(R, 3, env.F, W, sets, tile)
        call = PpoCall(env, data, 2)
        env.ppo_reserve(R)
        check_grads(f"tile {tile}", call.run(f"tile {tile}", sets=sets, vsets=vsets, **COEF), model(data, W, V, sets, vsets))
        call.free()
    finally:
        env.close()


def test_a_tile_the_library_does_not_carry_is_refused(monkeypatch):
    monkeypatch.setenv("CZ_PPO_TILE", "8")
    env = crowded(2)
    try:
        W, V = loaded(env, 2, 1)
        call = PpoCall(env, trajectory(4, 2, env.F, W, (0, 0), 1), 2)
        env.ppo_reserve(4)
        call.fill()
        with pytest.raises(_native.NativeError, match="carries 16, 32 and 64"):
            call.launch(sets=(0, 0), **COEF)
        call.free()
    finally:
        env.close()


def test_the_index_permuted_repeated_and_out_of_range():
    env = crowded(2)
    try:
        W, V = loaded(env, 2, 1)
        R, sets = 70, (1, 0)
        data = trajectory(R, 2, env.F, W, sets, 3)
        call = PpoCall(env, data, 2)
        env.ppo_reserve(130)
        rng = np.random.default_rng(4)
        whole = model(data, W, V, sets, None)
        perm = rng.permutation(R).astype(np.int32)
        repeated = rng.integers(0, R, 130).astype(np.int32)
        outside = repeated[:65].copy()
        outside[[0, 7, 63, 64]] = (-1, R, 2 ** 31 - 1, -2 ** 31)
        for name, index in (("none", None), ("permutation", perm), ("repeated rows", repeated), ("out of range", outside), ("one position", perm[:1])):
            call.set_index(index)
            want = whole if index is None else model(data, W, V, sets, None, index=index)
            got = call.run(name, sets=sets, **COEF)
            check_grads(f"index: {name}", got, want)
            assert got[1].view(np.float64)[7] == (4.0 if name == "out of range" else 0.0)
            if name == "permutation":                              # the same rows in another order: another summation, other bits
                assert not np.array_equal(canon(want[0][0]), canon(whole[0][0])), "a permutation gives the same bits: the order shows nothing"
        call.free()
    finally:
        env.close()


def test_sets_per_agent_holes_unused_sets_and_null_outputs():
    """four sets loaded: every agent on another set; agents at 0xFF in one word or both; one set used and the others zero; NULL
    statistics; no critic at all with NULL value gradients"""
    env = crowded(4)
    try:
        W, V = loaded(env, 4, 2)
        R = 65
        data = trajectory(R, 4, env.F, W, (0, 1, 2, 3), 5)
        call = PpoCall(env, data, 4)
        env.ppo_reserve(R)
        none4 = (None,) * 4
        for sets, vsets in (((0, 1, 2, 3), (0, 1, 2, 3)), ((3, 2, 1, 0), (0, 1, 2, 3)), ((1, None, 2, None), (None, None, 2, 0)),
                            ((2, 2, 2, 2), (2, 2, 2, 2)), (none4, (1, 1, None, 3)), ((0, 3, None, None), none4)):
            critic = any(v is not None for v in vsets)
            want = model(data, W, V, sets, vsets)
            got = call.run(f"sets {sets} vsets {vsets}", sets=sets, vsets=vsets, with_value=critic, **COEF)
            check_grads(f"sets {sets}, vsets {vsets}", got, want, with_value=critic)
            used = {s for s in sets + vsets if s is not None}
            for k in set(range(4)) - used:
                assert all(((g[k] & 0x7FFFFFFF) == 0).all() for g in got[0][:4 + 2 * critic]), f"sets {sets}, vsets {vsets}: unused set {k} is not zero"
            assert want[1][5] == 0 or np.abs(want[0][2]).max() > 0
        sets = (0, 1, 2, 3)
        check_grads("no statistics", call.run("no statistics", sets=sets, with_stats=False, **COEF), model(data, W, V, sets, None), with_stats=False)
        # other coefficients: no entropy term, no value term, a clip of 0 (everything off 1.0 on the advantage's side is clipped)
        for kw in (dict(clip=0.2, c_value=0.5, c_entropy=0.0), dict(clip=0.0, c_value=0.0, c_entropy=0.01), dict(clip=0.05, c_value=1.0, c_entropy=0.5)):
            check_grads(f"{kw}", call.run(f"{kw}", sets=sets, **kw), model(data, W, V, sets, None, **kw))
        call.free()
    finally:
        env.close()


def test_a_reload_is_seen_and_a_captured_graph_equals_the_eager_calls():
    env = crowded(2)
    try:
        Wa, Va = loaded(env, 2, 7)
        Wb, Vb = weights(env.F, env.num_actions, 2, 8, scale2=0.3), value_weights(2, 8)
        R, sets, vsets = 130, (0, 1), (0, 0)
        data = trajectory(R, 2, env.F, Wa, sets, 9)
        call = PpoCall(env, data, 2)
        env.ppo_reserve(R)
        first = call.run("first weights", sets=sets, vsets=vsets, **COEF)
        check_grads("first weights", first, model(data, Wa, Va, sets, vsets))
        dev = [env.alloc(w.shape, np.float32) for w in Wb + Vb]
        for d, w in zip(dev, Wb + Vb):
            d.from_host(w)
        call.fill()
        env.load_policy(*dev[:4])                                  # three stream-ordered calls, no wait in between
        env.load_value(*dev[4:])
        call.launch(sets=sets, vsets=vsets, **COEF)
        env.sync()
        eager = call.get("reloaded weights")
        check_grads("reloaded weights", eager, model(data, Wb, Vb, sets, vsets))
        assert not np.array_equal(eager[0][0], first[0][0])
        env.sync()
        cs = CallerStream(env)
        call.fill()
        with cs.capture():
            assert env.ppo_reserve(R) == R                         # nothing to allocate: legal inside the capture
            env.load_policy(*dev[:4])
            env.load_value(*dev[4:])
            call.launch(sets=sets, vsets=vsets, **COEF)
            with pytest.raises(_native.NativeError, match="outside the capture"):
                env.ppo_reserve(R + 1)
        got = call.get("capture")
        assert all((g == F32_SENT).all() for g in got[0]) and (got[1] == STAT_SENT).all(), "capturing must not have launched anything"
        for k in range(2):
            call.fill()
            cs.replay()
            cs.sync()
            got = call.get(f"replay {k}")
            assert all(np.array_equal(g, e) for g, e in zip(got[0], eager[0])) and np.array_equal(got[1], eager[1]), f"replay {k} differs from the eager call"
        cs.close()
        call.free()
    finally:
        env.close()


def test_refusals_write_nothing():
    env = crowded(2)
    try:
        lib = _native.lib()
        assert lib.cz_ppo_chunk() == ppo.PPO_CHUNK == 64
        F, Cn = env.F, env.num_actions
        W, V = weights(F, Cn, 3, 0, scale2=0.3), value_weights(2, 0)
        R = 20
        data = trajectory(R, 2, F, W, (0, 0), 1)
        call = PpoCall(env, data, 3)
        call.fill()
        run = lambda **kw: call.launch(**{**dict(sets=(0, 0), **COEF), **kw})

        def refused(message, fn):
            with pytest.raises(_native.NativeError, match=message):
                fn()
            env.sync()
            got = call.get(message)
            assert all((g == F32_SENT).all() for g in got[0]) and (got[1] == STAT_SENT).all(), f"a refused call ({message}) wrote something"

        refused("no weight table loaded", lambda: env.ppo_reserve(R))
        refused("no weight table loaded", run)
        assert lib.cz_ppo_reserved(env._h) == 0
        env.load_policy(*W)
        refused("but the workspace holds 0", lambda: run(vsets=(None, None)))
        refused("max_positions is 0", lambda: env.ppo_reserve(0))
        assert env.ppo_reserve(R) == R and env.ppo_reserve(R - 5) == R
        refused("value head of set 0, but 3 sets and 0 value heads", run)
        env.load_value(*V)
        refused("weight set 3, but 3 are loaded", lambda: run(sets=(0, 3)))
        refused("value head of set 2, but 3 sets and 2 value heads", lambda: run(vsets=(0, 2)))
        refused("0xFF in both sets and vsets", lambda: run(sets=(None, None), vsets=(None, None)))
        call.set_index(np.zeros(R + 1, np.int32))
        refused(f"{R + 1} positions, but the workspace holds {R}", run)
        call.set_index(None)
        p = [b.ptr for b in call.inputs] + [b.ptr + 256 for b in call.grads]
        raw = lambda rows, positions, index, ptrs, clip=0.2, cv=0.5, ce=0.01, vsets=0x0000: _native.check(env._h, lib.cz_ppo_grad_device(
            env._h, rows, positions, index, *ptrs[:5], 0x0000 | 0xFFFF0000, vsets | 0xFFFF0000, clip, cv, ce, *ptrs[5:], None))
        refused("positions is 0", lambda: raw(R, 0, None, p))
        refused("rows is 0", lambda: raw(0, R, None, p))
        refused("without an index positions", lambda: raw(R, R - 1, None, p))
        for k in range(9):                                         # every required pointer
            refused("pointer", lambda: raw(R, R, None, p[:k] + [None] + p[k + 1:]))
        refused("value-gradient pointer is null", lambda: raw(R, R, None, p[:9] + [None, p[10]]))
        raw(R, R, None, p[:9] + [None, None], vsets=0xFFFF)       # no critic: no value gradients needed
        env.sync()
        call.fill()
        for bad in (-0.5, float("nan")):
            refused("clip is", lambda: raw(R, R, None, p, clip=bad))
            refused("c_value is", lambda: raw(R, R, None, p, cv=bad))
            refused("c_entropy is", lambda: raw(R, R, None, p, ce=bad))
        env.load_policy(*weights(F, Cn, 4, 0, scale2=0.3))
        refused("4 sets are loaded, but the workspace was reserved for 3", run)
        env.load_policy(*W)
        check_grads("after the refusals", call.run("after", sets=(0, 0), **COEF), model(data, W, V, (0, 0), None))
        call.free()
    finally:
        env.close()


def test_on_the_devices_own_trajectory_the_ratio_is_one():
    """rollout_policy_value -> logprob_device -> gae_device -> ppo_grad_device at 48 envs, T = 4: the same arithmetic gives the same
    log-probability, so ratio == 1.0 exactly - stats[3] == 0.0, nothing is clipped - and the gradients are the model's"""
    n, T, A = 48, 4, 2
    env = make(n, "coop_test", "example", A, TWO, "scheme3", max_steps=3, num_layouts=3)
    try:
        F, Cn = env.F, env.num_actions
        W, V = loaded(env, 2, 11)
        env.reset(return_obs=False)
        sets, vsets = (0, 1), (0, 0)
        b = dict(obs=env.alloc((T + 1, n, A, F), np.float32), act=env.alloc((T, n, A), np.int32), logits=env.alloc((T, n, A, Cn), np.float32),
                 rew=env.alloc((T, n, A), np.float64), term=env.alloc((T, n, A), np.uint8), trunc=env.alloc((T, n, A), np.uint8),
                 val=env.alloc((T + 1, n, A), np.float32), logp=env.alloc((T, n, A), np.float32), adv=env.alloc((T, n, A), np.float32),
                 ret=env.alloc((T, n, A), np.float32))
        rows1 = env.alloc((T, n, A, F), np.float32)
        env.observe_device(d_obs32=b["obs"])
        env.rollout_policy_value(T, rows1, b["val"], b["act"], b["logits"], b["rew"], b["term"], b["trunc"], sets=sets, vsets=vsets, mode="sample", seed=5)
        env.logprob_device(b["logits"], b["act"], b["logp"], sets=sets, rows=T * n)
        env.gae_device(T, b["rew"], b["term"], b["trunc"], b["val"], b["adv"], b["ret"], gamma=GAMMA, lam=LAM)
        env.sync()
        before = np.concatenate([b["obs"].to_host()[:1], rows1.to_host()[:T - 1]]).reshape(T * n, A, F)      # the row in front of every step
        data = (before, b["act"].to_host().reshape(T * n, A), b["logp"].to_host().reshape(T * n, A), b["adv"].to_host().reshape(T * n, A),
                b["ret"].to_host().reshape(T * n, A))
        assert len(np.unique(data[1])) >= 3 and np.abs(data[3]).max() > 0
        call = PpoCall(env, data, 2)
        env.ppo_reserve(T * n)
        got = call.run("own trajectory", sets=sets, vsets=vsets, **COEF)
        want = model(data, W, V, sets, vsets)
        check_grads("own trajectory", got, want)
        st = got[1].view(np.float64)
        assert st[3] == 0.0 and st[4] == 0.0 and st[5] == T * n * A and st[6] == T * n * A and st[7] == 0.0, st.tolist()
        # ratio == 1.0: the surrogate is minus the mean advantage, summed in the model's order
        lone = ppo.host_ppo_grad(*data[:2], np.zeros_like(data[2]), *data[3:], W, V, sets, vsets, **COEF)
        assert lone[1][3] != 0.0, "any logp_old gives a KL estimate of 0.0: the case shows nothing"
        call.free()
    finally:
        env.close()
