"""GPU: the lean one-step kernel (k_step_lean, cz_kernels.h) against the generic one (k_step<..., 0>, forced with CZ_LEAN=0).

launch_step picks the lean kernel when the handle's settings allow it (narrow recipe tables, no despawn / respawn, float64
observations of at most 384 features with write-through stores, no compact output, no marks buffer).  Both kernels must give
the same observations, rewards, flags, records and statistics bit for bit: every golden set replayed through cz_step_device by
both, and a few hundred steps of the state-aware fuzz policy on the small-instance levels, also checked against the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from fuzz_policy import BumperActions
from golden_io import GoldenSet, golden_sets
from gpu_common import handle_for_set, strip_golden
from vec_common import bits, last_lean, lean, make_env, oracle_for, strip

pytestmark = pytest.mark.gpu

make = functools.partial(make_env, num_layouts=16)          # coop_test, two agents, 30 steps; 16 layouts


def handle_last_lean(L, h):
    L.cz_diag_last_step_lean.restype = C.c_int32
    L.cz_diag_last_step_lean.argtypes = [C.c_void_p]
    return int(L.cz_diag_last_step_lean(h))


def replay_device(gs, enabled):
    """the golden episodes of one set through cz_step_device; -> per-step (records, obs, rewards, term, trunc), final stats, lean flag"""
    eps = gs.episodes
    with lean(enabled):
        h, rids, _ = handle_for_set(gs)
    n, A, F = len(eps), eps[0].dims.A, eps[0].dims.F
    h.reset(np.arange(n), rids, want_obs=False)
    d_act, d_obs = h.dev_alloc(n * A * 4), h.dev_alloc(n * A * F * 8)
    d_rew, d_term, d_trunc = h.dev_alloc(n * A * 8), h.dev_alloc(n * A), h.dev_alloc(n * A)
    out, flags = [], set()
    for t in range(max(len(ep.actions) for ep in eps)):
        acts = np.zeros((n, A), dtype=np.int32)
        for i, ep in enumerate(eps):
            if t < len(ep.actions):
                acts[i] = ep.actions[t]
        h.h2d(d_act, acts)
        h.ck(h.L.cz_step_device(h.h, C.c_void_p(d_act), C.c_void_p(d_obs), C.c_void_p(d_rew), C.c_void_p(d_term), C.c_void_p(d_trunc)))
        flags.add(handle_last_lean(h.L, h.h))
        out.append((h.get_state(), h.d2h(d_obs, (n, A, F), np.float64), h.d2h(d_rew, (n, A), np.float64),
                    h.d2h(d_term, (n, A), np.uint8), h.d2h(d_trunc, (n, A), np.uint8)))
    st = h.stats()
    h.close()
    return out, st, flags


def lean_eligible(gs):
    d = gs.episodes[0].dims
    return d.D <= 64 and d.W * d.H <= 64 and d.F <= 384 and gs.recipe_table.shape[1] == 9


@pytest.mark.parametrize("name", golden_sets())
def test_golden_lean_and_generic(name):
    gs = GoldenSet(name)
    a, st_a, fa = replay_device(gs, True)
    b, st_b, fb = replay_device(gs, False)
    assert fb == {0}
    assert fa == ({1} if lean_eligible(gs) else {0}), f"{name}: lean kernel taken {fa}"
    for t, (x, y) in enumerate(zip(a, b)):
        for k, (u, v) in enumerate(zip(x, y)):
            assert u.tobytes() == v.tobytes(), f"{name} step {t}: output {k} differs between the lean and the generic kernel"
    assert st_a == st_b
    # and both are the reference's
    for t, (rec, obs, rew, term, trunc) in enumerate(a):
        for i, ep in enumerate(gs.episodes):
            if t >= len(ep.actions):
                continue
            ctx = f"{name} ep{i} step {t}"
            assert np.array_equal(strip_golden(rec[i]), strip_golden(ep.states[t + 1])), f"{ctx}: state"
            assert np.array_equal(bits(rew[i]), bits(ep.rewards[t])), f"{ctx}: reward"
            assert np.array_equal(term[i], ep.terms[t]) and np.array_equal(trunc[i], ep.truncs[t]), f"{ctx}: flags"
            assert np.array_equal(bits(obs[i]), bits(ep.obs[t + 1])), f"{ctx}: obs"


FUZZ = [
    ("scheme3", "coop_test", 2, ["TomatoLettuceSalad", "CarrotBanana"], "example", 60),
    ("scheme1", "coop_test", 2, ["TomatoLettuceSalad", "CarrotBanana"], "example", 45),
    ("scheme3", "coop_test", 1, ["TomatoLettuceSalad"], "example", 80),
    ("scheme1", "switch_test", 2, ["MashedCarrotBanana", "TomatoSalad"], "example", 50),
    ("scheme3", "crowded_6x5", 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], "crowded_6x5", 40),
    ("scheme3", "edge_8x8", 3, ["TomatoSalad", "MashedCarrotBanana", "TomatoLettuceSalad"], "edge", 35),
]


@pytest.mark.parametrize("scheme,level,agents,recipes,meta,max_steps", FUZZ)
def test_fuzz_lean_and_generic(scheme, level, agents, recipes, meta, max_steps):
    """300 steps of the biased fuzz policy with next-step auto-reset; lean vs generic byte for byte, lean vs the oracle"""
    n, T = 64, 300
    kw = dict(level=level, meta=meta, agents=agents, recipes=recipes, scheme=scheme, max_steps=max_steps,
              num_layouts=24, end_condition_all_dishes=level == "crowded_6x5")
    with lean(True):
        ea = make(n, **kw)
    with lean(False):
        eb = make(n, **kw)
    orc = oracle_for(ea)
    ea.reset(return_obs=False), eb.reset(return_obs=False), orc.reset()
    pol = BumperActions(ea.dims, ea.scheme_class.CODE, np.random.default_rng(100 * agents + len(level) + (7 if scheme == "scheme1" else 0)))
    A, F = ea.num_agents, ea.F
    bufs = [(e.alloc((n, A), np.int32), e.alloc((n, A, F), np.float64), e.alloc((n, A), np.float64), e.alloc((n, A), np.uint8),
             e.alloc((n, A), np.uint8)) for e in (ea, eb)]
    for t in range(T):
        acts = pol.act(orc.records)
        outs = []
        for e, (d_act, *o) in zip((ea, eb), bufs):
            d_act.from_host(acts)
            e.step_device(d_act, *o)
            outs.append([b.to_host() for b in o] + [e.get_state()])
        assert last_lean(ea) == 1
        for k, (u, v) in enumerate(zip(*outs)):
            assert u.tobytes() == v.tobytes(), f"step {t}: output {k} differs between the lean and the generic kernel"
        oo, ro, to, uo = orc.step(acts)
        pol.observe_result(orc.records)
        obs, rew, term, trunc, rec = outs[0]
        assert np.array_equal(bits(obs), bits(oo)), f"step {t}: obs vs oracle"
        assert np.array_equal(bits(rew), bits(ro)), f"step {t}: reward vs oracle"
        assert np.array_equal(term, to) and np.array_equal(trunc, uo), f"step {t}: flags vs oracle"
        assert np.array_equal(strip(rec), orc.records), f"step {t}: state vs oracle"
    assert ea.stats() == eb.stats()
    ea.close(), eb.close()


def test_bench_workload_takes_lean_kernel():
    """the bench's headline call (cz_step_device_ring, 4096 envs of BASELINE config 2) launches k_step_lean; the same steps with
    the generic kernel give the same outputs, records and statistics"""
    from cooking_zoo_amd.vec_env import CookingVecEnv
    N, A, P, K = 4096, 2, 16, 48
    res = []
    for enabled in (True, False):
        with lean(enabled):
            env = CookingVecEnv(N, "coop_test", "example", A, 400, ["TomatoLettuceSalad", "CarrotBanana"], action_scheme="scheme3",
                                num_layouts=256, auto_reset=True)
        env.reset(return_obs=False)
        d_ring = env.alloc((P, N, A), np.int32)
        d_ring.from_host(np.random.default_rng(3).integers(0, env.n_actions, size=(P, N, A), dtype=np.int32))
        outs = (env.alloc((N, A, env.F), np.float64), env.alloc((N, A), np.float64), env.alloc((N, A), np.uint8), env.alloc((N, A), np.uint8))
        env.rollout(300, 3, 0)                       # (worlds a few hundred steps old, like the bench's timed regions)
        env.step_device_ring(K, d_ring, N * A, P, 0, *outs)
        env.sync()
        assert last_lean(env) == (1 if enabled else 0)
        res.append(([o.to_host().tobytes() for o in outs], env.get_state().tobytes(), env.stats()))
        env.close()
    assert res[0] == res[1]
