"""GPU: cz_rollout_actions - T fused steps over the CALLER'S actions ([T][N][A] int32 in HBM) - against the oracle stepped
over the same rows, on every level family / kernel instance / scheme, incl. on-device auto-reset inside the launch, negative
("does not act") actions, chunked launches that continue each other, and BASELINE config 2 at full size."""
import numpy as np
import pytest

from cooking_zoo_amd import soa
from vec_common import bits, make_env as make, strip

pytestmark = pytest.mark.gpu


def run_and_compare(env, orc, acts, chunks=1, check_every=1):
    """acts [T, n, A]: the rollout in `chunks` launches, every step's outputs against the oracle"""
    T, n, A = acts.shape
    F = env.F
    Tc = T // chunks
    assert Tc * chunks == T
    d_act = env.alloc((Tc, n, A), np.int32)
    d_obs, d_rew = env.alloc((Tc, n, A, F), np.float64), env.alloc((Tc, n, A), np.float64)
    d_t, d_u = env.alloc((Tc, n, A), np.uint8), env.alloc((Tc, n, A), np.uint8)
    for c in range(chunks):
        d_act.from_host(acts[c * Tc:(c + 1) * Tc])
        env.rollout_actions(d_act, Tc, d_obs, d_rew, d_t, d_u)
        env.sync()
        obs, rew, term, trunc = d_obs.to_host(), d_rew.to_host(), d_t.to_host(), d_u.to_host()
        for t in range(Tc):
            oo, ro, to, uo = orc.step(acts[c * Tc + t], want_obs=(t % check_every == 0))
            if oo is not None:
                assert np.array_equal(bits(obs[t]), bits(oo)), f"obs @ chunk {c} step {t}"
            assert np.array_equal(bits(rew[t]), bits(ro)), f"rewards @ chunk {c} step {t}"
            assert np.array_equal(term[t], to) and np.array_equal(trunc[t], uo), f"flags @ chunk {c} step {t}"
        assert np.array_equal(strip(env.get_state()), orc.records), f"records after chunk {c}"
    for b in (d_act, d_obs, d_rew, d_t, d_u):
        b.free()


@pytest.mark.parametrize("scheme,level,agents,recipes,meta", [
    ("scheme3", "coop_test", 2, ["TomatoLettuceSalad", "CarrotBanana"], "example"),
    ("scheme1", "switch_test", 2, ["MashedCarrotBanana", "TomatoSalad"], "example"),
    ("scheme3", "coexistence_test", 1, ["TomatoLettuceOnionSalad"], "example"),
    ("scheme3", "crowded_6x5", 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], "crowded_6x5"),
    ("scheme1", "crowded_6x5", 3, ["TomatoSalad", "TomatoLettuceSalad", "MashedCarrotBanana"], "crowded_6x5"),
    ("scheme3", "large_16x16", 4, ["TomatoLettuceSalad", "CarrotBanana", "AppleWatermelon", "CucumberOnion"], "large_16x16"),
    ("scheme1", "large_16x16", 2, ["TomatoLettuceOnionSalad", "MashedCarrotBanana"], "large_16x16"),
    ("scheme3", "edge_8x8", 3, ["TomatoSalad", "MashedCarrotBanana", "TomatoLettuceSalad"], "edge"),
    ("scheme3", "edge_empty", 2, ["TomatoSalad", "no_recipe"], "edge"),
    ("scheme3", "huge_20x20", 2, ["TomatoLettuceSalad", "CarrotBanana"], "huge_20x20"),
])
def test_rollout_actions_matches_oracle(scheme, level, agents, recipes, meta):
    from oracle_binding import VecOracle
    n, T = 72, 90
    try:
        env = make(n, level, meta, agents, recipes, scheme)
    except FileNotFoundError:
        pytest.skip(f"level {level} not shipped")
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    orc.reset()
    rng = np.random.default_rng(11)
    acts = rng.integers(0, env.n_actions, size=(T, n, agents), dtype=np.int32)
    acts[rng.random(acts.shape) < 0.03] = -1                      # an agent that is not in the list world_step acts on
    run_and_compare(env, orc, acts, chunks=3)
    assert int(env.get_state()[:, soa.W_EPISODE].min()) >= 2      # auto-reset passes happened inside the launches
    env.close()


def test_rollout_actions_equals_step_device_launches():
    """the same rows through cz_step_device one launch at a time end in the same records and last-step outputs"""
    n, T, A = 200, 64, 2
    env = make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=25)
    twin = make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=25)
    env.reset(return_obs=False)
    twin.reset(return_obs=False)
    acts = np.random.default_rng(2).integers(0, 5, size=(T, n, A), dtype=np.int32)
    d_act = env.alloc((T, n, A), np.int32)
    d_act.from_host(acts)
    d_obs = env.alloc((T, n, A, env.F), np.float64)
    env.rollout_actions(d_act, T, d_obs)
    env.sync()
    t_act = twin.alloc((n, A), np.int32)
    outs = [twin.alloc((n, A, twin.F), np.float64), twin.alloc((n, A), np.float64), twin.alloc((n, A), np.uint8), twin.alloc((n, A), np.uint8)]
    for t in range(T):
        t_act.from_host(acts[t])
        twin.step_device(t_act, *outs)
    twin.sync()
    assert np.array_equal(strip(env.get_state()), strip(twin.get_state()))
    assert np.array_equal(bits(d_obs.to_host()[T - 1]), bits(outs[0].to_host()))
    assert env.stats() == twin.stats()
    env.close()
    twin.close()


def test_rollout_actions_config2_full_size():
    """BASELINE config 2: 4096 envs, coop_test, 2 agents; 48 fused steps over a caller's action tensor against the oracle on host
    threads (observations compared every 8th step, everything else every step)"""
    from oracle_binding import ShardedOracle
    n, T, A = 4096, 48, 2
    env = make(n, "coop_test", "example", A, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=400, num_layouts=256)
    orc = ShardedOracle(env)
    env.reset(return_obs=False)
    orc.reset()
    acts = np.random.default_rng(4).integers(0, 5, size=(T, n, A), dtype=np.int32)
    run_and_compare(env, orc, acts, chunks=2, check_every=8)
    env.close()


def test_rollout_actions_argument_errors():
    from cooking_zoo_amd import _native
    env = make(8, "coop_test", "example", 2, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3")
    env.reset(return_obs=False)
    L = _native.lib()
    assert L.cz_rollout_actions(env._h, 4, None, None, None, None, None) != 0
    assert b"actions" in L.cz_last_error(env._h)
    d = env.alloc((1, 8, 2), np.int32)
    assert L.cz_rollout_actions(env._h, 0, d.ptr, None, None, None, None) != 0
    env.close()
