"""The grid observation on the device (cz_observe_grid_device, k_observe_grid): exact against `grid.host_bits` of the oracle's
records, on every kernel instance, in every subset of the four outputs, over ranges, behind a step on the stream, inside a
caller's graph, sharded, and through the host convenience."""
import numpy as np
import pytest

from cooking_zoo_amd import _native, grid, soa
from grid_common import CASES, FORM_SUBSETS, FORMS, Coverage, GridBufs, checkpoints
from vec_common import COOP, CallerStream, env_of, instance, oracle_for, policy, strip, tables_of

pytestmark = pytest.mark.gpu

# (case, despawn / respawn on)
RUNS = [(name, False) for name in CASES] + [("coop_test", True)]


@pytest.mark.parametrize("name,spawn", RUNS, ids=[f"{n}{'-spawn' if s else ''}" for n, s in RUNS])
def test_every_instance_state_and_form(name, spawn):
    """set_state(oracle records) then the grid call: the kernel is a pure function of the record.  Every checkpoint in all four
    forms, plain and extended; the last one in all 15 non-empty subsets of the outputs, plain and extended"""
    n = 6
    tables, points = checkpoints(name, n, spawn)
    assert len(points) >= 3
    env = env_of(tables)
    assert instance(env) == CASES[name][5], "the case runs on another kernel instance"
    env.reset(return_obs=False)
    dims = env.dims
    bufs = {ext: GridBufs(env, n, ext) for ext in (False, True)}
    if spawn:
        gone = (points[:, :, soa.W_STATUS] >> 8) & 0xF
        assert gone.any(), "no checkpoint has a despawned agent"                                   # (the oracle alone)
    for k, recs in enumerate(points):
        env.set_state(recs)
        for ext in (False, True):
            for forms in (FORM_SUBSETS if k == len(points) - 1 else [FORMS]):
                b = bufs[ext]
                b.fill()
                env.observe_grid_device(extended=ext, **b.args(forms))
                b.check(f"{name} checkpoint {k} extended={ext} forms={forms}", forms, dims, recs)
    assert env.grid_shape() == (dims.W, dims.H, 32) and env.grid_shape(True) == (dims.W, dims.H, 48)
    env.close()


def test_the_states_reach_what_the_channels_show():
    """over the checkpoints above: held objects, filled plates, chopped and mashed food, a toggled blender, a pressed switch, a
    despawned agent (the oracle alone; computed once, shared with the test above)"""
    cov = Coverage()
    for name, spawn in RUNS:
        tables, points = checkpoints(name, 6, spawn)
        cov.add(grid.host_bits(tables.dims, points.reshape(-1, points.shape[-1]), True))
    missing = set(cov.never(1))
    for ch in ("object.held", "object.in_plate", "Tomato.chopped", "Carrot.mashed", "Banana.mashed", "Blender.toggle", "Switch.active",
               "Block.walkable", "agent.despawned", "agent3", "Cutboard.ready", "Blender.ready"):
        assert ch not in missing, f"no checkpoint sets {ch}"


def test_ranges_and_refusals():
    n = 13
    tables, points = checkpoints("coop_test", n)
    env = env_of(tables)
    env.reset(return_obs=False)
    env.set_state(points[-1])
    for ext in (False, True):
        b = GridBufs(env, 5, ext)                                         # rows laid out for 5 envs, the guard right behind them
        env.observe_grid_device(extended=ext, env_begin=3, env_count=5, **b.args(FORMS))
        b.check(f"envs 3..7 extended={ext}", FORMS, env.dims, points[-1][3:8])
        b.fill()
        env.observe_grid_device(extended=ext, env_begin=7, env_count=0, **b.args(FORMS))
        b.check("env_count = 0", (), env.dims, points[-1][:5])
    assert np.array_equal(env.get_state(), points[-1]), "the grid call wrote a record"
    b = GridBufs(env, n, False)
    L = _native.lib()
    P = lambda f: b.buf[f].ptr
    assert L.cz_grid_channels(0) == 32 and L.cz_grid_channels(1) == 48 and L.cz_grid_channels(2) == -1 and L.cz_grid_channels(-1) == -1
    for args, msg in (((0, n, 0, None, None, None, None), "null"), ((0, n, 2, P("bits"), None, None, None), "extended"),
                      ((0, n, -1, P("bits"), None, None, None), "extended"), ((10, 5, 0, P("bits"), None, None, None), "range"),
                      ((-1, 2, 0, P("bits"), None, None, None), "range"), ((0, n + 1, 1, None, P("grid8"), None, None), "range")):
        assert L.cz_observe_grid_device(env._h, *args) != 0, f"{args} was accepted"
        text = L.cz_last_error(env._h).decode()
        assert msg in text, f"{args}: message {text!r}"
    with pytest.raises(_native.NativeError, match="null"):
        env.observe_grid_device()
    b.check("after the refusals", (), env.dims, points[-1])
    env.close()


def closed_loop_env(n=9):
    """coop_test with auto-reset and episodes of 7 steps onto 3 layouts, its oracle and policy, and the loop's device buffers"""
    tables = tables_of(n, **dict(COOP, max_steps=7))
    env = env_of(tables)
    A = env.num_agents
    d = dict(act=env.alloc((n, A), np.int32), rew=env.alloc((n, A), np.float64), term=env.alloc((n, A), np.uint8),
             trunc=env.alloc((n, A), np.uint8))
    return env, d


def test_stream_order_behind_a_step():
    """step_device then observe_grid_device with no synchronisation in between, 20 steps with auto-resets onto other layouts"""
    n = 9
    env, d = closed_loop_env(n)
    orc, pol = oracle_for(env), policy(env, 3)
    env.reset(return_obs=False)
    orc.reset()
    b = GridBufs(env, n, True)
    layouts_seen = set()
    for t in range(20):
        acts = pol.act(orc.records)
        d["act"].from_host(acts)
        b.fill()
        env.step_device(d["act"], None, d["rew"], d["term"], d["trunc"])
        env.observe_grid_device(extended=True, **b.args(FORMS))
        orc.step(acts, want_obs=False)
        pol.observe_result(orc.records)
        b.check(f"step {t}", FORMS, env.dims, orc.records)
        assert np.array_equal(strip(env.get_state()), strip(orc.records)), f"step {t}: records"
        layouts_seen |= set(orc.records[:, soa.W_LAYOUT].tolist())
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 2 and len(layouts_seen) >= 2, "no auto-reset onto another layout"
    env.close()


def test_captured_into_a_callers_graph():
    """the pair captured once and replayed 5 times = the eager loop of a twin, grids and records"""
    n = 9
    env, d = closed_loop_env(n)
    twin, dt = closed_loop_env(n)
    orc, pol = oracle_for(env), policy(env, 4)
    for e in (env, twin):
        e.reset(return_obs=False)
    orc.reset()
    b, bt = GridBufs(env, n, True), GridBufs(twin, n, True)
    cs = CallerStream(env)
    with cs.capture():
        env.step_device(d["act"], None, d["rew"], d["term"], d["trunc"])
        env.observe_grid_device(extended=True, **b.args(FORMS))
    assert np.array_equal(env.get_state(), twin.get_state()), "capturing executed something"
    for r in range(5):
        acts = pol.act(orc.records)
        d["act"].from_host(acts)
        dt["act"].from_host(acts)
        cs.replay()
        cs.sync()
        twin.step_device(dt["act"], None, dt["rew"], dt["term"], dt["trunc"])
        twin.observe_grid_device(extended=True, **bt.args(FORMS))
        orc.step(acts, want_obs=False)
        pol.observe_result(orc.records)
        b.check(f"replay {r}", FORMS, env.dims, orc.records)
        for f in FORMS:
            assert np.array_equal(b.buf[f].to_host(), bt.buf[f].to_host()), f"replay {r}: {f} differs from the eager loop"
        assert np.array_equal(env.get_state(), twin.get_state()), f"replay {r}: records differ from the eager loop"
    cs.close()
    env.close()
    twin.close()


def test_sharded_equals_one_handle():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n = 11
    level, meta, agents, recipes, scheme, _inst, _steps = CASES["crowded_6x5"]
    tables, points = checkpoints("crowded_6x5", n)
    kw = dict(action_scheme=scheme, num_layouts=4)
    sh = ShardedVecEnv(n, level, meta, agents, 241, recipes, device_ids=[0, 0, 0], **kw)
    assert len({s.num_envs for s in sh.shards}) > 1, "the shards are equal"
    one = env_of(tables)
    sh.reset(return_obs=False)
    one.reset(return_obs=False)
    sh.set_state(points[-1])
    one.set_state(points[-1])
    W, H, C = sh.grid_shape(True)
    assert (W, H, C) == one.grid_shape(True)
    sb = dict(bits=sh.alloc((W, H, 2), np.uint32), grid8=sh.alloc((W, H, C), np.uint8), grid32=sh.alloc((W, H, C), np.float32),
              agent_xy=sh.alloc((agents, 2), np.int32))
    sh.observe_grid_device(sb["bits"], sb["grid8"], sb["grid32"], sb["agent_xy"], extended=True)
    sh.sync()
    b = GridBufs(one, n, True)
    one.observe_grid_device(extended=True, **b.args(FORMS))
    b.check("one handle", FORMS, one.dims, points[-1])
    for f in FORMS:
        got = sb[f].to_host()
        want = b.buf[f].to_host()[:b.size[f]].reshape(b.shape[f])
        assert np.array_equal(got.view(np.uint32) if f in ("grid32", "agent_xy") else got, want), f"{f}: the shards differ from one handle"
    sh.close()
    one.close()


def test_host_convenience():
    tables, points = checkpoints("limit_8x31", 6)
    env = env_of(tables)
    env.reset(return_obs=False)
    env.set_state(points[1])
    for ext in (False, True):
        g, xy = env.observe_grid(extended=ext)
        want = grid.expand(grid.host_bits(env.dims, points[1], ext), np.uint8)
        assert g.dtype == np.uint8 and g.shape == (6,) + env.grid_shape(ext) and np.array_equal(g, want)
        assert xy.dtype == np.int32 and np.array_equal(xy, grid.agent_xy(env.dims, points[1]))
    g, xy = env.observe_grid(env_begin=2, env_count=3)
    assert np.array_equal(g, grid.expand(grid.host_bits(env.dims, points[1][2:5]), np.uint8)) and xy.shape == (3, 2, 2)
    env.close()
