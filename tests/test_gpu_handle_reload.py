"""GPU: what one handle owns over its life.  Every table a handle can be given again - recipes, layouts, level programs, rank rows,
spawn tables, sprites, partner table, goal table, policy weights, value heads - is loaded at least twice into one handle, and after
the last load of each the batch still steps with the oracle, one step at a time and in a ring run long enough to be replayed from a
captured graph; then a setting that makes the cached graphs stale, the run again, and close().  And twelve create-use-close cycles
in one process, each touching what a handle makes lazily (the host step's staging, the compact staging, the layout copy stream, the
second chain's stream, the timing events): the last cycle's outputs are the first's bit for bit.  Outputs only - how much device
memory is free on the card is not this process's to read.  9 envs: one whole workgroup of 8 and a partial one."""
import ctypes as C

import numpy as np
import pytest

from cooking_zoo_amd import _native, render, soa
from vec_common import Outs, bits, check_step, env_of, make_env, oracle_for, policy, strip, tables_of

pytestmark = pytest.mark.gpu

N, K_RING = 9, 50                  # K_RING >= the handle's graph_min_run (48): the run is one captured piece
SPAWN = dict(agent_despawn_rate=0.1, agent_respawn_rate=0.4, grace_period=2, spawn_seed=3)


def counts(env):
    g, d = C.c_int64(), C.c_int64()
    _native.check(env._h, _native.lib().cz_launch_counts(env._h, C.byref(g), C.byref(d), 0))
    return g.value, d.value


def ring_graphs(env):
    f = _native.lib().cz_diag_ring_graphs
    f.restype, f.argtypes = C.c_int32, [C.c_void_p]
    return int(f(env._h))


class Life:
    """one env and its oracle twin, stepped together"""

    def __init__(self, env):
        self.env, self.orc, self.pol, self.o = env, oracle_for(env), policy(env, 5), Outs(env)
        self.rng = np.random.default_rng(11)
        self.d_ring = env.alloc((K_RING, env.num_envs, env.num_agents), np.int32)
        self.d_codes = None
        assert np.array_equal(bits(env.reset()), bits(self.orc.reset())), "reset observation"

    def records(self, ctx):
        assert np.array_equal(strip(self.env.get_state()), self.orc.records), f"{ctx}: records"

    def steps(self, ctx, T=3):
        for t in range(T):
            acts = self.pol.act(self.orc.records)
            check_step(f"{ctx}, step {t}", self.o.step(self.env, acts), self.orc.step(acts))
            self.pol.observe_result(self.orc.records)
            self.records(f"{ctx}, step {t}")

    def ring(self, ctx):
        """K_RING steps as one ring run: replayed from a graph, the last step's outputs and the records with the oracle's"""
        env, n, A = self.env, self.env.num_envs, self.env.num_agents
        acts = self.rng.integers(0, env.n_actions, size=(K_RING, n, A), dtype=np.int32)
        self.d_ring.from_host(acts)
        self.o.fill()
        g0, _ = counts(env)
        b = self.o.buf
        env.step_device_ring(K_RING, self.d_ring, n * A, K_RING, 0, b["obs"], b["rew"], b["term"], b["trunc"])
        env.sync()
        for a in acts:
            want = self.orc.step(a)
        check_step(f"{ctx}, ring run", self.o.get(), want)
        self.records(f"{ctx}, ring run")
        assert counts(env)[0] - g0 == K_RING, f"{ctx}: the ring run was not replayed from a graph"
        assert ring_graphs(env) == 1, f"{ctx}: {ring_graphs(env)} cached graphs, not the one of this run"
        if self.d_codes is not None:
            codes = self.d_codes.to_host()
            assert np.array_equal(bits(env.obs_table()[codes[:, :, :env.F]]), bits(want[0])), f"{ctx}: the compact rows of the run's last step"
        self.pol = policy(env, 6)                    # (the state-aware policy starts over on the records the run left)

    def check(self, ctx):
        self.steps(ctx)
        self.ring(ctx)


def same(ctx, a, b):
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), f"{ctx}: the answer changed over a reload of the same table"


def test_every_table_reloads_in_one_life():
    L = _native.lib()
    env = make_env(N, max_steps=12, **SPAWN)
    assert (env.dims.W, env.dims.H, env.num_agents) == (7, 7, 2)
    life = Life(env)
    h, book = env._h, len(env.book_names)
    life.check("fresh handle")

    # recipes (the load drops the partner and the goal table: they follow)
    for _ in range(2):
        _native.check(h, L.cz_load_recipes(h, env.recipe_table.ctypes.data_as(C.c_void_p), book, env.recipe_nodes))
    for _ in range(2):
        _native.check(h, L.cz_load_partner_table(h, env.partner_rows.ctypes.data_as(C.c_void_p), book))
        _native.check(h, L.cz_load_goal_table(h, env.goal_table.ctypes.data_as(C.c_void_p), book, env.num_goals))
    life.check("recipes")

    # partner table, rank rows, goal table: the queries that read them answer as before the reload
    partner = env.partner()
    for _ in range(2):
        _native.check(h, L.cz_load_partner_table(h, env.partner_rows.ctypes.data_as(C.c_void_p), book))
    same("partner table", env.partner(), partner)
    assert env.partner_bad_recipes() == 0
    life.check("partner table")
    partner = env.partner()
    for _ in range(2):
        env._upload_ranks(0, env.layouts)
    same("rank rows", env.partner(), partner)
    life.check("rank rows")
    infos = env.infos()
    for _ in range(2):
        _native.check(h, L.cz_load_goal_table(h, env.goal_table.ctypes.data_as(C.c_void_p), book, env.num_goals))
    same("goal table", tuple(env.infos()[k] for k in sorted(infos)), tuple(infos[k] for k in sorted(infos)))
    life.check("goal table")

    # layouts (the same pool: the oracle's stays; set_layouts gives the spawn tables their layout map again), level programs
    partner = env.partner()
    for _ in range(2):
        env.set_layouts(list(env.layouts))
    same("layouts", env.partner(), partner)
    life.check("layouts")
    for _ in range(2):
        env.load_level_programs()
    assert env.generate_failures() == 0
    life.check("level programs")

    # spawn tables
    for _ in range(2):
        env.set_spawn_rates(*env._spawn_cfg)
    assert env.spawn_exhausted() == 0
    life.check("spawn tables")

    # sprites: another sheet in between shows that a load takes effect
    env.load_sprites(M=16)
    frame = env.render(env_count=2, P=8)
    env.load_sprites(255 - render.builtin_sprites(8))
    assert env.render(env_count=2, P=8).tobytes() != frame.tobytes(), "sprites: another sheet draws the same frame"
    env.load_sprites(M=16)
    same("sprites", env.render(env_count=2, P=8), frame)
    life.check("sprites")

    # policy weights and value heads, likewise
    A, F, Cn = env.num_agents, env.F, env.num_actions
    rng = np.random.default_rng(3)
    w = [rng.standard_normal(s).astype(np.float32) * 0.1 for s in ((64, F), (64,), (Cn, 64), (Cn,), (64,), (1,))]
    d_rows, d_logits, d_values = env.alloc((N, A, F), np.float32), env.alloc((N, A, Cn), np.float32), env.alloc((N, A), np.float32)
    env.observe_device(d_obs32=d_rows)

    def logits():
        d_logits.from_host(np.zeros((N, A, Cn), np.float32))
        env.policy_device(d_rows, d_logits=d_logits)
        return d_logits.to_host()

    def values():
        d_values.from_host(np.zeros((N, A), np.float32))
        env.value_device(d_rows, d_values)
        return d_values.to_host()

    env.load_policy(*w[:4])
    first_logits = logits()
    assert np.abs(first_logits).max() > 0
    env.load_policy(w[0] * 2, *w[1:4])
    assert logits().tobytes() != first_logits.tobytes(), "policy weights: other weights give the same logits"
    env.load_policy(*w[:4])
    same("policy weights", logits(), first_logits)
    life.check("policy weights")
    env.load_value(*w[4:])
    first = values()
    assert np.abs(first).max() > 0
    env.load_value(w[4] * 2, w[5])
    assert values().tobytes() != first.tobytes(), "value heads: other weights give the same values"
    env.load_value(*w[4:])
    same("value heads", values(), first)
    same("policy weights beside the value heads", logits(), first_logits)
    life.check("value heads")

    # a setting the cached graphs carry: they are dropped, the run is captured again and also writes the compact rows
    life.d_codes = env.alloc((N, A, env.codes_pitch), np.uint8)
    env.set_compact_output(life.d_codes)
    life.ring("compact output on")
    env.set_compact_output(None)
    life.d_codes = None
    life.check("compact output off")
    assert int(life.orc.records[:, soa.W_EPISODE].min()) >= 3, "episodes ended and auto-reset passes ran between the loads"
    env.close()


def one_cycle(tables, acts, ring_acts):
    """a handle from create to close, through everything it makes on first use; what it computed, as bytes"""
    L = _native.lib()
    env = env_of(tables)
    n, A = env.num_envs, env.num_agents
    out = [env.reset().tobytes()]
    for a in acts:                                                        # the host step: its staging blocks
        out += [x.tobytes() for x in env.step(a)]
    out.append(env.observe_compact().tobytes())                           # the compact staging
    env.update_layouts(0, env.layouts[:2])                                # the copy stream, its events and staging (same content)
    env.set_ring_split(2)
    assert env.ring_split_parts() == 2, "two chains: the second stream and its events are made by this run"
    d_ring = env.alloc(ring_acts.shape, np.int32)
    d_ring.from_host(ring_acts)
    o = Outs(env)
    o.fill()
    b = o.buf
    env.step_device_ring(K_RING, d_ring, n * A, K_RING, 0, b["obs"], b["rew"], b["term"], b["trunc"])
    env.sync()
    out += [x.tobytes() for x in o.get()]
    _native.check(env._h, L.cz_kernel_time_reset(env._h, 1))              # kernel timing: its events
    for a in acts:
        out += [x.tobytes() for x in o.step(env, a)]
    ms, launches = C.c_double(), C.c_int64()
    _native.check(env._h, L.cz_kernel_time_read(env._h, C.byref(ms), C.byref(launches)))
    assert launches.value == len(acts) and ms.value > 0.0, f"kernel timing saw {launches.value} launches in {ms.value} ms"
    _native.check(env._h, L.cz_kernel_time_reset(env._h, 0))
    out += [env.get_state().tobytes(), repr(sorted(env.stats().items())).encode()]
    env.close()
    return out


def test_create_use_close_cycles_compute_the_same():
    tables = tables_of(N, "coop_test", "example", 2, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", 12, 8)
    rng = np.random.default_rng(21)
    acts = rng.integers(0, 5, size=(3, N, 2), dtype=np.int32)
    ring_acts = rng.integers(0, 5, size=(K_RING, N, 2), dtype=np.int32)
    first = one_cycle(tables, acts, ring_acts)
    for cycle in range(1, 12):
        last = one_cycle(tables, acts, ring_acts)
    assert len(first) == len(last)
    for k, (x, y) in enumerate(zip(first, last)):
        assert x == y, f"output {k} of cycle 11 differs from cycle 0's"
