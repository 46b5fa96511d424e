"""GPU parity (run with -m gpu on an MI355X): the HIP path, called through the C-ABI, must agree bit for bit
with (a) the golden traces captured from the reference and (b) the oracle, on state, float64 observations,
float64 rewards and flags."""
import numpy as np
import pytest

from cooking_zoo_amd import soa
from golden_io import GoldenSet, golden_sets
from gpu_common import Handle, handle_for_set, oracle_for_set, strip_golden
from vec_common import bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", golden_sets())
def test_hip_replays_golden(name):
    gs = GoldenSet(name)
    eps = gs.episodes
    h, rids, lays = handle_for_set(gs)
    n = len(eps)
    obs0 = h.reset(np.arange(n), rids)
    st = h.get_state()
    for i, ep in enumerate(eps):
        assert np.array_equal(strip_golden(st[i]), strip_golden(ep.states[0])), f"{name} ep{i}: reset state"
        assert np.array_equal(bits(obs0[i]), bits(ep.obs[0])), f"{name} ep{i}: reset obs"
    T = max(len(ep.actions) for ep in eps)
    A = eps[0].dims.A
    for t in range(T):
        acts = np.zeros((n, A), dtype=np.int32)
        for i, ep in enumerate(eps):
            if t < len(ep.actions):
                acts[i] = ep.actions[t]
        obs, rew, term, trunc = h.step(acts)
        st = h.get_state()
        for i, ep in enumerate(eps):
            if t >= len(ep.actions):
                continue
            ctx = f"{name} ep{i} (seed {ep.seed}, {ep.policy}) step {t} actions {ep.actions[t].tolist()}"
            if not np.array_equal(strip_golden(st[i]), strip_golden(ep.states[t + 1])):
                pytest.fail(f"{ctx}: state differs\n-- hip\n{soa.describe_record(ep.dims, st[i])}\n-- reference\n"
                            f"{soa.describe_record(ep.dims, ep.states[t + 1])}\n-- before\n"
                            f"{soa.describe_record(ep.dims, ep.states[t])}")
            assert np.array_equal(bits(rew[i]), bits(ep.rewards[t])), f"{ctx}: reward {rew[i]} vs {ep.rewards[t]}"
            assert np.array_equal(term[i], ep.terms[t]) and np.array_equal(trunc[i], ep.truncs[t]), ctx
            if not np.array_equal(bits(obs[i]), bits(ep.obs[t + 1])):
                bad = np.argwhere(bits(obs[i]) != bits(ep.obs[t + 1]))
                pytest.fail(f"{ctx}: obs differs at {bad[:8].tolist()}: {obs[i][tuple(bad[0])]} vs "
                            f"{ep.obs[t + 1][tuple(bad[0])]}")
    h.close()


@pytest.mark.parametrize("name", ["cfg2_coop_2agents", "switch_2agents", "scheme1_coop_2agents", "large16_4agents",
                                  "crowded_4agents"])
def test_set_state_observe_roundtrip(name):
    """cz_set_state / cz_get_state / cz_observe on mid-episode states from the reference."""
    gs = GoldenSet(name)
    h, rids, lays = handle_for_set(gs)
    eps = gs.episodes
    h.reset(np.arange(len(eps)), rids)
    for t in (1, 17, 60):
        recs = np.stack([ep.states[min(t, len(ep.states) - 1)] for ep in eps]).copy()
        for i in range(len(eps)):
            recs[i, soa.W_LAYOUT] = i
        h.set_state(recs)
        assert np.array_equal(h.get_state(), recs)
        obs = h.observe()
        for i, ep in enumerate(eps):
            assert np.array_equal(bits(obs[i]), bits(ep.obs[min(t, len(ep.states) - 1)]))
    h.close()


@pytest.mark.parametrize("name", __import__("golden_io").spawn_sets())
def test_hip_replays_despawn_respawn_steps(name):
    """Steps captured with agent despawn / respawn on (action -1 = the agent is not in the list world_step acts on):
    every step on its own, from its captured start state to the world right before the reference's spawn handling."""
    gs = GoldenSet(name)
    eps = gs.episodes
    h, rids, lays = handle_for_set(gs)
    n, A = len(eps), eps[0].dims.A
    h.reset(np.arange(n), rids)
    base = h.get_state()
    T = max(len(ep.actions) for ep in eps)
    inactive = 0
    for t in range(T):
        recs = base.copy()
        acts = np.zeros((n, A), dtype=np.int32)
        for i, ep in enumerate(eps):
            k = min(t, len(ep.actions) - 1)
            keep = {w: recs[i, w] for w in (soa.W_LAYOUT, soa.W_EPISODE, soa.W_POOL, soa.W_RECIPES)}
            recs[i] = ep.states[k]
            for w, v in keep.items():
                recs[i, w] = v
            acts[i] = ep.actions[k]
        h.set_state(recs)
        obs, rew, term, trunc = h.step(acts)
        st = h.get_state()
        for i, ep in enumerate(eps):
            if t >= len(ep.actions):
                continue
            ctx = f"{name} ep{i} (seed {ep.seed}) step {t} actions {ep.actions[t].tolist()}"
            if not np.array_equal(strip_golden(st[i]), strip_golden(ep.pre_states[t])):
                pytest.fail(f"{ctx}: state differs\n-- device\n{soa.describe_record(ep.dims, st[i])}\n-- reference\n"
                            f"{soa.describe_record(ep.dims, ep.pre_states[t])}")
            assert np.array_equal(bits(obs[i]), bits(ep.pre_obs[t])), ctx
            assert np.array_equal(bits(rew[i]), bits(ep.rewards[t])), f"{ctx}: reward {rew[i]} vs {ep.rewards[t]}"
            assert np.array_equal(term[i], ep.terms[t]) and np.array_equal(trunc[i], ep.truncs[t]), ctx
            inactive += int((ep.actions[t] < 0).sum())
    assert inactive > 20
    h.close()
