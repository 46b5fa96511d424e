"""GPU: cz_set_ring_split - a run of cz_step_device_ring / cz_step_device_many issued as two launch chains over the two halves of
the batch, on two streams of the handle - against the same run issued unsplit on a second handle from the same seed: state records,
observations, rewards, flags, statistics, per-env episode records and launch counts bit for bit, and once against the oracle.  Small
shapes: no split (1 env), parts of one env, odd split points, partial last workgroups; episodes end, auto-reset passes and layout
changes fall inside the runs (max_steps = 7); the runs cover ring wrap, graph pieces and direct pieces.  And what is never split: a
run inside a stream capture of the caller, any run of a process held to fewer than 4 hardware queues."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from vec_common import CallerStream, TWO, bits, make_env, oracle_for, strip

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 9, 17, 200]
LEVELS = [
    ("coop_test", "example", 2, TWO, "scheme3"),                                                                                   # small instance
    ("large_16x16", "large_16x16", 4, ["TomatoLettuceSalad", "CarrotBanana", "AppleWatermelon", "CucumberOnion"], "scheme3"),     # large instance
]
RUNS = [(2, 8, 0), (37, 16, 5), (3, 3, 2), (60, 64, 63)]           # (K, period, first_slot): direct pieces, ring wrap, a graph piece of 59


@contextlib.contextmanager
def graph_min_run(value):
    """CZ_GRAPH_MIN_RUN is read by cz_create"""
    old = os.environ.get("CZ_GRAPH_MIN_RUN")
    os.environ["CZ_GRAPH_MIN_RUN"] = str(value)
    try:
        yield
    finally:
        if old is None:
            del os.environ["CZ_GRAPH_MIN_RUN"]
        else:
            os.environ["CZ_GRAPH_MIN_RUN"] = old


def make(n, level=LEVELS[0], mode=0):
    name, meta, agents, recipes, scheme = level
    env = make_env(n, name, meta, agents, recipes, scheme, max_steps=7)
    env.reset(return_obs=False)
    was = env.set_ring_split(mode)
    assert was == -1, f"a fresh handle is in automatic mode, not {was}"
    return env


def counts(env):
    g, d = C.c_int64(), C.c_int64()
    _native.check(env._h, _native.lib().cz_launch_counts(env._h, C.byref(g), C.byref(d), 0))
    return g.value, d.value


class Run:
    """the buffers of one handle; every run leaves (outputs, records, stats, episodes found, launch counts)"""

    def __init__(self, env):
        n, A = env.num_envs, env.num_agents
        self.env = env
        self.out = (env.alloc((n, A, env.F), np.float64), env.alloc((n, A), np.float64), env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8))

    def ring(self, K, period, first, actions, many=False):
        env = self.env
        n, A = env.num_envs, env.num_agents
        d_ring = env.alloc((period, n, A), np.int32)
        d_ring.from_host(actions)
        if many:
            _native.check(env._h, _native.lib().cz_step_device_many(env._h, K, d_ring.ptr, n * A, period, *(b.ptr for b in self.out)))
        else:
            env.step_device_ring(K, d_ring, n * A, period, first, *self.out)
        env.sync()
        d_ring.free()
        return self.result()

    def result(self):
        env = self.env
        return (tuple(b.to_host().tobytes() for b in self.out), env.get_state().tobytes(), env.stats(), env.finished_episodes().tobytes(), counts(env))


def same(ctx, a, b):
    for name, x, y in zip(("observations", "rewards", "terminations", "truncations"), a[0], b[0]):
        assert x == y, f"{ctx}: {name} differ"
    assert a[1] == b[1], f"{ctx}: state records differ"
    assert a[2] == b[2], f"{ctx}: statistics differ: {a[2]} / {b[2]}"
    assert a[3] == b[3], f"{ctx}: episode records differ"
    assert a[4] == b[4], f"{ctx}: launch counts differ: {a[4]} / {b[4]}"


def actions_of(rng, env, period):
    a = rng.integers(0, env.n_actions, size=(period, env.num_envs, env.num_agents), dtype=np.int32)
    a[rng.random(a.shape) < 0.03] = -1
    return a


@pytest.mark.parametrize("level", LEVELS, ids=[lv[0] for lv in LEVELS])
@pytest.mark.parametrize("n", SIZES)
def test_split_runs_equal_unsplit_runs(n, level):
    split, whole = make(n, level, 2), make(n, level, 0)
    assert split.ring_split_parts() == (2 if n >= 2 else 1) and whole.ring_split_parts() == 1
    rs, rw = Run(split), Run(whole)
    rng = np.random.default_rng(100 + n)
    for K, period, first in RUNS:
        acts = actions_of(rng, split, period)
        same(f"{level[0]}, {n} envs, run {(K, period, first)}", rs.ring(K, period, first, acts), rw.ring(K, period, first, acts))
    g, d = counts(split)
    assert g == 59 and g + d == sum(K for K, _, _ in RUNS), "launch counts count steps: one graph piece of 59, the rest direct"
    assert int(split.get_state()[:, soa.W_EPISODE].min()) >= 2, "auto-reset passes fell inside the runs"
    # ... and the same through cz_step_device_many
    acts = actions_of(rng, split, 5)
    same(f"{level[0]}, {n} envs, cz_step_device_many", rs.ring(13, 5, 0, acts, many=True), rw.ring(13, 5, 0, acts, many=True))
    split.close(); whole.close()


def test_tiny_graphs_are_replayed_split():
    """CZ_GRAPH_MIN_RUN=4: pieces of four and more steps are graphs, replayed several times"""
    with graph_min_run(4):
        split, whole = make(17, mode=2), make(17, mode=0)
    rs, rw = Run(split), Run(whole)
    rng = np.random.default_rng(7)
    acts = actions_of(rng, split, 6)
    for rep in range(3):                                          # slots 1..5 (a graph of 5), 0..5 (of 6), 0..3 (of 4): 15 steps, replayed
        same(f"repetition {rep}", rs.ring(15, 6, 1, acts), rw.ring(15, 6, 1, acts))
    assert counts(split) == (45, 0)
    split.close(); whole.close()


def test_split_run_matches_oracle():
    n = 17
    env = make(n, mode=2)
    orc = oracle_for(env)
    orc.reset()
    run, rng = Run(env), np.random.default_rng(3)
    for K, period, first in RUNS:
        acts = actions_of(rng, env, period)
        run.ring(K, period, first, acts)
        obs, rew, term, trunc = (b.to_host() for b in run.out)
        for k in range(K):
            oo, ro, to, uo = orc.step(acts[(first + k) % period], want_obs=(k == K - 1))
        assert np.array_equal(bits(obs), bits(oo)) and np.array_equal(bits(rew), bits(ro)), f"run {(K, period, first)}: rows differ from the oracle's"
        assert np.array_equal(term, to) and np.array_equal(trunc, uo), f"run {(K, period, first)}: flags differ from the oracle's"
        assert np.array_equal(strip(env.get_state()), orc.records), f"run {(K, period, first)}: records differ from the oracle's"
    env.close()


def test_run_inside_a_callers_capture_is_not_split():
    n, A, K, R, period = 17, 2, 6, 5, 8
    env, ref = make(n, mode=2), make(n, mode=0)
    re_, rr = Run(env), Run(ref)
    acts = actions_of(np.random.default_rng(11), env, period)
    de, dr = env.alloc((period, n, A), np.int32), ref.alloc((period, n, A), np.int32)
    de.from_host(acts); dr.from_host(acts)
    cs = CallerStream(env)
    with cs.capture():
        env.step_device_ring(K, de, n * A, period, 1, *re_.out)
    nodes = C.c_size_t()
    cs.hip.lib.hipGraphGetNodes.restype = C.c_int
    cs.hip.ck(cs.hip.lib.hipGraphGetNodes(cs.graph, None, C.byref(nodes)), "hipGraphGetNodes")
    assert nodes.value == K, f"{K} captured steps are {nodes.value} nodes of the caller's graph: one launch per step, no second chain"
    cs.replay(R)
    cs.sync()
    for _ in range(R):                                             # the eager loop
        ref.step_device_ring(K, dr, n * A, period, 1, *rr.out)
    ref.sync()
    a, b = re_.result(), rr.result()
    same("captured and replayed against eager", a[:4] + ((0, 0),), b[:4] + ((0, 0),))        # (captured steps are not counted)
    cs.close()
    env.close(); ref.close()


def test_setter_returns_previous_mode_and_drops_graphs():
    L = _native.lib()
    L.cz_diag_ring_graphs.restype, L.cz_diag_ring_graphs.argtypes = C.c_int32, [C.c_void_p]
    with graph_min_run(4):
        env = make(9, mode=2)                                     # (make: the fresh handle reported -1)
    run = Run(env)
    acts = actions_of(np.random.default_rng(1), env, 8)
    run.ring(8, 8, 0, acts)
    assert L.cz_diag_ring_graphs(env._h) == 1
    assert env.set_ring_split(2) == 2 and L.cz_diag_ring_graphs(env._h) == 1      # no change: the graphs stay
    assert env.set_ring_split(0) == 2 and L.cz_diag_ring_graphs(env._h) == 0
    assert env.ring_split_parts() == 1
    run.ring(8, 8, 0, acts)
    assert L.cz_diag_ring_graphs(env._h) == 1
    assert env.set_ring_split(-1) == 0 and L.cz_diag_ring_graphs(env._h) == 0
    assert env.ring_split_parts() == 1, "automatic mode leaves 9 envs whole"
    with pytest.raises(_native.NativeError):
        env.set_ring_split(3)
    assert env.set_ring_split(2) == -1
    env.close()


CHILD = """
import sys
sys.path[:0] = {paths!r}
from vec_common import make_env
env = make_env(9, max_steps=7)
print("parts", env.set_ring_split(2), env.ring_split_parts())
env.close()
"""


def test_fewer_than_four_hardware_queues_never_split():
    """the decision only: the child creates a handle, asks, and makes no run"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = {}
    for queues in ("2", "4"):
        p = subprocess.run([sys.executable, "-c", CHILD.format(paths=[os.path.dirname(here), here])], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, GPU_MAX_HW_QUEUES=queues))
        assert p.returncode == 0, p.stderr[-2000:]
        out[queues] = [line for line in p.stdout.split("\n") if line.startswith("parts")]
    assert out == {"2": ["parts -1 1"], "4": ["parts -1 2"]}, out
