"""GPU: the three kernel instances and the lean one-step kernel at the edges of the rules that pick them, against the oracle bit
for bit (float64 values as uint64).

cz_create picks the instance from the slot count D and the cell count C (small Inst<1,1>: D <= 64 and C <= 64; large
Inst<2,4>: D <= 128 and C <= 256; huge Inst<4,16> otherwise); launch_step takes k_step_lean on the small instance when
F <= 128 * OBS_PAIRS = 384, the stores are write-through (N <= 10 240), the tables are narrow, nothing spawns and no codes or
marks are asked for.  Here:
  * one coop_test world padded to D = 64 | 65 | 128 | 129 | 255 runs on every instance, through cz_step_device,
    cz_rollout_actions and cz_step_device_compact: observations, rewards and flags are the natural-D oracle's bytes at every
    D, records its records on the shared words with the padding slots zero, statistics those of the natural-D run;
  * dense_8x8 (all 64 slots in use, F = 466: the generic kernel's chunk loop on the small instance), with 1-4 agents, both
    schemes, once on the large instance, and once with despawn / respawn on;
  * which kernel a launch took at F = 384 | 385 and N = 1 | 9 | 10 240 | 10 241, and with null reward / flag outputs.
Every output buffer is filled with 0xFF bytes before a launch, so a feature or flag the kernel leaves unwritten cannot pass
for a value written earlier.  cz_diag_instance / cz_diag_last_step_lean say which instance and kernel ran."""
import functools

import numpy as np
import pytest

from cooking_zoo_amd import soa
from oracle_binding import ShardedOracle, VecOracle
from vec_common import (DENSE_RECIPES, PADDED, Outs, bits, check_step, instance, junk, last_lean, make_env, one_world_trajectory, policy,
                        run_compact, strip, widen)

pytestmark = pytest.mark.gpu

make = functools.partial(make_env, max_steps=40)


# ---------------------------------------------------------------------------------------------------------------------------
# one world on every instance
# ---------------------------------------------------------------------------------------------------------------------------

def run_step_device(env, acts, want, dn):
    o = Outs(env)
    for t, a in enumerate(acts):
        ctx = f"D={env.dims.D} cz_step_device step {t}"
        check_step(ctx, o.step(env, a), want[t])
        assert np.array_equal(strip(env.get_state()), widen(want[t][4], dn, env.dims)), f"{ctx}: records"
    return env.stats()


def run_rollout_actions(env, acts, want, dn, chunks=2):
    T, n, A = acts.shape
    Tc, F = T // chunks, env.F
    spec = [((Tc, n, A, F), np.float64), ((Tc, n, A), np.float64), ((Tc, n, A), np.uint8), ((Tc, n, A), np.uint8)]
    d_act, bufs = env.alloc((Tc, n, A), np.int32), [env.alloc(s, t) for s, t in spec]
    for c in range(chunks):
        for b, (s, t) in zip(bufs, spec):
            b.from_host(junk(s, t))
        d_act.from_host(acts[c * Tc:(c + 1) * Tc])
        env.rollout_actions(d_act, Tc, *bufs)
        env.sync()
        outs = [b.to_host() for b in bufs]
        for t in range(Tc):
            check_step(f"D={env.dims.D} cz_rollout_actions chunk {c} step {t}", [x[t] for x in outs], want[c * Tc + t])
        assert np.array_equal(strip(env.get_state()), widen(want[(c + 1) * Tc - 1][4], dn, env.dims)), f"D={env.dims.D} chunk {c}: records"
    return env.stats()


@pytest.mark.parametrize("scheme", ["scheme3", "scheme1"])
def test_one_world_on_every_instance(scheme):
    n, T = 32, 200
    # the trajectory: the state-aware policy over the natural-D oracle
    dn, obs0, rec0, acts, want, episodes = one_world_trajectory(scheme, n, T)
    assert episodes >= 3
    first = {}
    for D, inst in PADDED:
        for path, run in (("step_device", run_step_device), ("rollout_actions", run_rollout_actions), ("compact", run_compact)):
            env = make(n, scheme=scheme, max_dyn=D)
            assert env.dims.D == (D or 12) and instance(env) == inst, f"max_dyn={D}: instance {instance(env)}"
            assert np.array_equal(bits(env.reset()), bits(obs0)), f"D={D}: reset observation"
            assert np.array_equal(strip(env.get_state()), widen(rec0, dn, env.dims)), f"D={D}: reset records"
            st = run(env, acts, want, dn)
            if path == "step_device":
                assert last_lean(env) == (1 if inst == 0 else 0), f"D={D}: lean flag"
            assert instance(env) == inst
            first.setdefault(path, st)
            assert st == first[path], f"D={D} {path}: statistics differ from the natural-D run"
            env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# dense_8x8: every slot lane of the small instance in use, two observation chunks
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme,agents,max_dyn,inst", [
    ("scheme3", 1, None, 0), ("scheme1", 1, None, 0), ("scheme3", 2, None, 0), ("scheme1", 2, None, 0),
    ("scheme3", 3, None, 0), ("scheme1", 3, None, 0), ("scheme3", 4, None, 0), ("scheme1", 4, None, 0),
    ("scheme3", 4, 65, 1),
])
def test_dense_8x8_matches_oracle(scheme, agents, max_dyn, inst):
    n, T = 32, 300
    env = make(n, "dense_8x8", "dense_8x8", agents, DENSE_RECIPES[:agents], scheme, max_steps=70, max_dyn=max_dyn)
    assert (env.dims.W * env.dims.H, env.dims.D, env.F) == (64, max_dyn or 64, 466) and instance(env) == inst
    orc = VecOracle.from_vec_env(env)
    assert np.array_equal(bits(env.reset()), bits(orc.reset()))
    assert np.array_equal(strip(env.get_state()), orc.records)
    alive = ((orc.records[:, env.dims.dyn0_word0:env.dims.dyn0_word0 + env.dims.D] >> 24) & soa.DYN_ALIVE) != 0
    assert (alive.sum(1) == 48).all()                                  # every Counter holds an object from reset on
    pol = policy(env, 40 + 2 * agents + (scheme == "scheme1"))
    o = Outs(env)
    for t in range(T):
        acts = pol.act(orc.records)
        got = o.step(env, acts)
        assert last_lean(env) == 0
        check_step(f"step {t}", got, orc.step(acts))
        pol.observe_result(orc.records)
        assert np.array_equal(strip(env.get_state()), orc.records), f"step {t}: records"
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 3
    env.close()


def test_dense_8x8_despawn_respawn_matches_oracle_rule():
    """the cramped floor with despawn / respawn on: the fourth agent's spawn area is the two-cell passage, so respawns run out of
    free cells (the reference raises there, the build leaves the agent out for that step); records, observations, rewards and
    flags against the oracle's restatement of the keyed rule"""
    n, A, T = 64, 4, 300
    env = make(n, "dense_8x8", "dense_8x8", A, DENSE_RECIPES, "scheme3", max_steps=70, agent_despawn_rate=0.25,
               agent_respawn_rate=0.4, grace_period=1, spawn_seed=17)
    assert instance(env) == 0
    orc = VecOracle.from_vec_env(env)
    assert np.array_equal(bits(env.reset()), bits(orc.reset()))
    pol = policy(env, 77)
    n_gone = 0
    for t in range(T):
        acts = pol.act(orc.records)
        got = env.step(acts)
        check_step(f"step {t}", got, orc.step(acts))
        pol.observe_result(orc.records)
        assert np.array_equal(strip(env.get_state()), orc.records), f"step {t}: records"
        n_gone += int((((orc.records[:, soa.W_STATUS] >> 8) & 0xF) != 0).sum())
    assert n_gone > 100
    assert env.spawn_exhausted() > 0
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the lean / generic split
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("meta,F,n,lean", [
    ("example_f384", 384, 64, 1),             # the last feature count of one observation chunk
    ("example_f385", 385, 64, 0),             # the first past it
    ("example", 278, 1, 1),
    ("example", 278, 9, 1),
    ("example", 278, 10240, 1),               # the last batch with write-through stores
    ("example", 278, 10241, 0),
])
def test_lean_split(meta, F, n, lean):
    T = 20
    env = make(n, meta=meta, num_layouts=16)
    assert env.F == F and instance(env) == 0
    orc = ShardedOracle(env) if n > 1024 else VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    orc.reset()
    pol = policy(env, n + F)
    o = Outs(env)
    for t in range(T):
        acts = pol.act(orc.records)
        got = o.step(env, acts)
        check_step(f"F={F} N={n} step {t}", got, orc.step(acts))
        assert last_lean(env) == lean, f"step {t}: lean flag"
        pol.observe_result(orc.records)
    assert np.array_equal(strip(env.get_state()), orc.records)
    env.close()


@pytest.mark.parametrize("skip", [("rew",), ("term",), ("trunc",), ("rew", "term", "trunc")])
def test_lean_step_with_null_outputs(skip):
    """an observation buffer but null rewards / terminations / truncations: the lean kernel still runs (those outputs go to the
    handle's scratch block), and what was asked for, and the state, is the oracle's"""
    n, T = 48, 60
    env = make(n, max_steps=25)
    orc = VecOracle.from_vec_env(env)
    env.reset(return_obs=False)
    orc.reset()
    pol = policy(env, 5 + len(skip[0]) + len(skip))
    o = Outs(env, skip=skip)
    for t in range(T):
        acts = pol.act(orc.records)
        got = o.step(env, acts)
        assert last_lean(env) == 1, f"step {t}: lean flag"
        check_step(f"null {skip} step {t}", got, orc.step(acts))
        pol.observe_result(orc.records)
        assert np.array_equal(strip(env.get_state()), orc.records), f"step {t}: records"
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 1
    env.close()
