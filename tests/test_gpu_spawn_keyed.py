"""GPU: the despawn / respawn rule inside the step kernels (cz_set_spawn, Ops::handle_agent_spawn) against trajectories of the
UNMODIFIED reference (tests/golden/spawn_keyed_*.npz: cooking_world.py:267-290 handle_agent_spawn / parsing.py:154-167
generate_location fed with the batched build's keyed draws - tools/gen_golden.py capture_spawn_keyed_episode).  One handle per
captured world (its env id is part of the key), driven through the raw C-ABI: cz_step step by step, cz_rollout_actions over
the captured actions, and - for the worlds whose actions are the device's own stream - cz_rollout.  Records incl. the status
word, observations of every agent (also despawned ones), rewards, flags incl. the truncated-once report: bit for bit.
All three kernel instances, both action schemes, 2-4 agents."""
import ctypes as C

import numpy as np
import pytest

from cooking_zoo_amd import soa
from golden_io import GoldenSet, layout_from_episode, spawn_keyed_sets
from gpu_common import Handle, _ptr
from vec_common import bits

pytestmark = pytest.mark.gpu


def strip_keyed(rec):
    """a golden record against the device's: the status word stays (it holds the spawn bookkeeping), the episode word too"""
    r = rec.copy()
    r[..., soa.W_LAYOUT] = 0
    r[..., soa.W_POOL] = 0
    r[..., soa.RET_WORD0:soa.RET_WORD0 + 8] = 0        # running returns: device-side statistics only
    return r


def keyed_handle(gs, ep):
    dims = ep.dims
    h = Handle(dims, 1, scheme=gs.scheme, max_steps=gs.cfg["max_steps"], end_all=gs.cfg["end_condition_all_dishes"],
               num_recipes=len(gs.cfg["recipes"]), reward_scheme=gs.cfg.get("reward_scheme"), table=gs.recipe_table,
               env_id_base=ep.env_id)
    lay = layout_from_episode(ep)
    h.load_layouts(lay.init_record(dims, 0, gs.recipe_ids)[None], lay.obs_descriptor(gs.meta, dims)[None])
    A = dims.A
    stride = max(max(len(xs), len(ys)) for xs, ys in ep.spawn_areas)
    sx, sy = np.zeros((1, A, stride), dtype=np.uint8), np.zeros((1, A, stride), dtype=np.uint8)
    nx, ny = np.zeros((1, A), dtype=np.int32), np.zeros((1, A), dtype=np.int32)
    for a, (xs, ys) in enumerate(ep.spawn_areas):
        nx[0, a], ny[0, a] = len(xs), len(ys)
        sx[0, a, :len(xs)], sy[0, a, :len(ys)] = xs, ys
    d, r, g = gs.cfg["rates"]
    h.ck(h.L.cz_set_spawn(h.h, d, r, g, gs.cfg["spawn_seed"], 1, None, stride, _ptr(sx), _ptr(nx), _ptr(sy), _ptr(ny)))
    return h


def start_record(ep):
    rec = ep.states[0].copy()[None]
    rec[0, soa.W_LAYOUT] = 0
    return rec


@pytest.mark.parametrize("name", spawn_keyed_sets())
def test_hip_replays_keyed_despawn_respawn(name):
    gs = GoldenSet(name)
    n_gone = 0
    for ei, ep in enumerate(gs.episodes):
        h = keyed_handle(gs, ep)
        T, A, F = len(ep.actions), ep.dims.A, ep.dims.F
        ctx0 = f"{name} ep{ei} (seed {ep.seed}, {ep.policy}, env {ep.env_id}, episode {ep.episode_no})"
        # ---- the reset path: a fresh world gets everybody present and the grace periods running
        rid = np.full((1, 4), 0xFF, dtype=np.uint8)
        rid[0, :len(gs.recipe_ids)] = gs.recipe_ids
        h.reset([0], rid)
        st = h.get_state()
        assert st[0, soa.W_STATUS] == ep.states[0][soa.W_STATUS], f"{ctx0}: status word after cz_reset"
        # ---- cz_step, one step at a time
        h.set_state(start_record(ep))
        for t in range(T):
            obs, rew, term, trunc = h.step(ep.actions[t][None])
            st = h.get_state()
            ctx = f"{ctx0} step {t} actions {ep.actions[t].tolist()}"
            if not np.array_equal(strip_keyed(st[0]), strip_keyed(ep.states[t + 1])):
                pytest.fail(f"{ctx}: state differs (status {st[0][soa.W_STATUS]:#x} vs {ep.states[t + 1][soa.W_STATUS]:#x})\n-- device\n"
                            f"{soa.describe_record(ep.dims, st[0])}\n-- reference\n{soa.describe_record(ep.dims, ep.states[t + 1])}")
            assert np.array_equal(bits(obs[0]), bits(ep.obs[t + 1])), f"{ctx}: observation"
            assert np.array_equal(bits(rew[0]), bits(ep.rewards[t])), f"{ctx}: reward {rew[0]} vs {ep.rewards[t]}"
            assert np.array_equal(term[0], ep.terms[t]) and np.array_equal(trunc[0], ep.truncs[t]), f"{ctx}: flags {trunc[0]} vs {ep.truncs[t]}"
        n_gone += int(ep.truncs.sum())
        # ---- the fused forms from the same start: the caller's actions, and (stream episodes) the device's own action stream
        d_act = h.dev_alloc(T * A * 4)
        d_obs, d_rew = h.dev_alloc(T * A * F * 8), h.dev_alloc(T * A * 8)
        d_t, d_u = h.dev_alloc(T * A), h.dev_alloc(T * A)
        h.h2d(d_act, ep.actions.astype(np.int32))
        forms = [("cz_rollout_actions", lambda: h.L.cz_rollout_actions(h.h, T, d_act, d_obs, d_rew, d_t, d_u))]
        if ep.policy == "stream":
            forms.append(("cz_rollout", lambda: h.L.cz_rollout(h.h, T, gs.cfg["spawn_seed"], 0, d_obs, d_rew, d_t, d_u)))
        for what, launch in forms:
            h.set_state(start_record(ep))
            h.ck(launch())
            h.ck(h.L.cz_sync(h.h))
            obs, rew = h.d2h(d_obs, (T, A, F), np.float64), h.d2h(d_rew, (T, A), np.float64)
            term, trunc = h.d2h(d_t, (T, A), np.uint8), h.d2h(d_u, (T, A), np.uint8)
            assert np.array_equal(bits(obs), bits(ep.obs[1:])), f"{ctx0}: {what} observations"
            assert np.array_equal(bits(rew), bits(ep.rewards)), f"{ctx0}: {what} rewards"
            assert np.array_equal(term, ep.terms) and np.array_equal(trunc, ep.truncs), f"{ctx0}: {what} flags"
            assert np.array_equal(strip_keyed(h.get_state()[0]), strip_keyed(ep.states[-1])), f"{ctx0}: {what} final record"
        assert h.L.cz_spawn_exhausted(h.h) == 0
        h.close()
    assert n_gone >= 4


def test_exhausted_respawn_is_counted_not_raised():
    """huge_20x20 gives its first two agents a one-cell spawn area, which a despawned agent occupies itself: the reference's
    generate_location raises ValueError after 1001 tries (parsing.py:166-167); the device puts the agent back where it stood and
    counts the event (documented deviation, include/cookingzoo.h)."""
    from cooking_zoo_amd.vec_env import CookingVecEnv
    n = 32
    env = CookingVecEnv(n, "huge_20x20", "huge_20x20", 3, 60, ["TomatoLettuceSalad", "MashedCarrotBanana", "TomatoSalad"], action_scheme="scheme3",
                        num_layouts=4, agent_despawn_rate=0.5, agent_respawn_rate=0.5, grace_period=0, spawn_seed=1)
    env.reset(return_obs=False)
    before = env.get_state()[:, soa.AGENT_WORD0:soa.AGENT_WORD0 + 2] & 0xFFFF
    rng = np.random.default_rng(0)
    for t in range(30):
        env.step(np.zeros((n, 3), dtype=np.int32), return_obs=False)       # nobody moves: agents 0 / 1 can only ever come back in place
    after = env.get_state()[:, soa.AGENT_WORD0:soa.AGENT_WORD0 + 2] & 0xFFFF
    assert np.array_equal(before, after)
    assert env.spawn_exhausted() > 0
    env.close()
