"""Shortest-path navigation on the device (cz_navigate_device, k_navigate): exact against `nav.host_navigate` of the oracle's
records on every kernel instance, in every subset of the three outputs, against the answers of the unmodified reference, on
worst-case corridors, over ranges, in a closed loop with the step on the stream, inside a caller's graph, sharded, and through
the host convenience."""
import numpy as np
import pytest

from cooking_zoo_amd import _native, nav, soa
from grid_common import CASES, case_tables, checkpoints
from nav_common import (COUNTER, FLOOR, OUTPUT_SUBSETS, OUTPUTS, NavBufs, agent_cells, all_cell_targets, draw_targets, golden,
                        golden_answers, serpentine, with_cells)
from vec_common import DENSE_RECIPES, CallerStream, env_of, instance, make_env, oracle_for, strip

pytestmark = pytest.mark.gpu


def run(env, bufs, targets, outputs=OUTPUTS, **kw):
    bufs.fill()
    bufs.target.from_host(targets)
    env.navigate_device(bufs.target, **bufs.args(outputs), **kw)


# (case, despawn / respawn on)
RUNS = [(name, False) for name in CASES] + [("coop_test", True)]


@pytest.mark.parametrize("name,spawn", RUNS, ids=[f"{n}{'-spawn' if s else ''}" for n, s in RUNS])
def test_every_case_against_the_host_model(name, spawn):
    """set_state(oracle records) then the call: the kernel is a pure function of the record.  Every checkpoint with one target
    per agent and both flag values, all three outputs; the last one also with eight targets, in all 7 non-empty subsets of the
    outputs.  With despawn / respawn on, a despawned agent is routed from its stored location"""
    n = 6
    tables, points = checkpoints(name, n, spawn)
    if spawn:
        assert ((points[:, :, soa.W_STATUS] >> 8) & 0xF).any(), "no checkpoint has a despawned agent"     # (the oracle alone)
    env = env_of(tables)
    assert instance(env) == CASES[name][5], "the case runs on another kernel instance"
    env.reset(return_obs=False)
    dims = env.dims
    bufs = {T: NavBufs(env, n, T) for T in (1, 8)}
    for k, recs in enumerate(points):
        env.set_state(recs)
        last = k == len(points) - 1
        for T in ((1, 8) if last else (1,)):
            tg = draw_targets(dims, recs, T, 7 * k + T)
            for wb in (False, True):
                want = nav.host_navigate(dims, recs, tg, wb)
                for outputs in (OUTPUT_SUBSETS if last else [OUTPUTS]):
                    run(env, bufs[T], tg, outputs, walkable_blocks=wb)
                    bufs[T].check(f"{name} checkpoint {k} T={T} walkable_blocks={wb} outputs={outputs}", outputs, want)
        assert np.array_equal(env.get_state(), recs), "the call wrote a record"
    env.close()


def test_the_targets_reach_every_kind_of_answer():
    """over the draws above (the host model alone): every walk code, goals reached and not, the agent's own cell, goals that are
    not Floor, and a result that the flag changes"""
    codes, kinds = set(), set()
    for name in CASES:
        tables, points = checkpoints(name, 6)
        recs, dims = points[-1], tables.dims
        tg = draw_targets(dims, recs, 8, 7 * (len(points) - 1) + 8)
        act, steps, _f = nav.host_navigate(dims, recs, tg)
        act2, steps2, _f2 = nav.host_navigate(dims, recs, tg, True)
        codes |= set(np.unique(act).tolist())
        kinds |= {"reached"} if (steps > 0).any() else set()
        kinds |= {"unreachable"} if ((steps < 0) & (tg[..., 0] >= 0) & (tg[..., 0] < dims.W) & (tg[..., 1] >= 0) & (tg[..., 1] < dims.H)).any() else set()
        kinds |= {"own cell"} if (steps == 0).any() else set()
        kinds |= {"flag"} if not np.array_equal(steps, steps2) else set()
        for e, rec in enumerate(recs):
            floor = nav.floor_set(dims, rec)
            for a in range(dims.A):
                for t in range(8):
                    x, y = tg[e, a, t]
                    if steps[e, a, t] > 0 and not floor[x, y]:
                        kinds.add("not Floor")
    assert codes == {0, 1, 2, 3, 4}, codes
    assert kinds == {"reached", "unreachable", "own cell", "flag", "not Floor"}, kinds


LEVEL_ARGS = {"coop_test": ("coop_test", "example", ["TomatoLettuceSalad", "CarrotBanana"]),
              "switch_test": ("switch_test", "example", ["MashedCarrotBanana", "TomatoSalad"]),
              "crowded_6x5": ("crowded_6x5", "crowded_6x5", ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"]),
              "dense_8x8": ("dense_8x8", "dense_8x8", DENSE_RECIPES)}


@pytest.mark.parametrize("k", range(5))
def test_against_the_reference(k):
    """the records of tests/golden/nav_ref.json.gz on the device, every agent and every cell as the goal, against what the
    unmodified BaseAgent.walk_to_location and reachable returned.  The stored cells and agents go into records of an env of the
    episode's level and agent count (the call reads nothing else of a record)."""
    ep = golden()["episodes"][k]
    level, meta, recipes = LEVEL_ARGS[ep["level"]]
    gd = soa.Dims(*ep["dims"])
    n = len(ep["states"])
    env = make_env(n, level, meta, gd.A, recipes[:gd.A], ep["scheme"], max_steps=50, num_layouts=2)
    dims = env.dims
    assert (dims.W, dims.H, dims.A) == (gd.W, gd.H, gd.A)
    env.reset(return_obs=False)
    recs = env.get_state()
    for e, st in enumerate(ep["states"]):
        g = np.array(st["record"], dtype=np.uint32)
        soa.record_cells(dims, recs[e])[:] = soa.record_cells(gd, g)
        recs[e, soa.AGENT_WORD0:soa.AGENT_WORD0 + dims.A] = g[soa.AGENT_WORD0:soa.AGENT_WORD0 + gd.A]
    env.set_state(recs)
    want = [golden_answers(ep, st) for st in ep["states"]]
    want_act = np.stack([w[0] for w in want]).reshape(n, dims.A, dims.C)
    want_reach = np.stack([w[1] for w in want]).reshape(n, dims.A, dims.C)
    bufs = NavBufs(env, n, 8)
    for tg, idx in all_cell_targets(dims, n):
        run(env, bufs, tg, ("action", "steps"))
        act, steps = bufs.read("action")[0], bufs.read("steps")[0]
        for t, c in enumerate(idx):
            if c < 0:
                assert (act[:, :, t] == 0).all() and (steps[:, :, t] == -1).all(), "padding target"
                continue
            ctx = f"{ep['set']} seed {ep['seed']}: goal {divmod(c, dims.H)}"
            assert np.array_equal(act[:, :, t], want_act[:, :, c]), f"{ctx}: actions {act[:, :, t].tolist()}, the reference {want_act[:, :, c].tolist()}"
            assert np.array_equal(steps[:, :, t] >= 0, want_reach[:, :, c]), f"{ctx}: steps {steps[:, :, t].tolist()}, reachable {want_reach[:, :, c].tolist()}"
    env.close()


@pytest.mark.parametrize("name,longest", [("huge_32x32", 400), ("dense_8x8", 30)])
def test_serpentine_corridor(name, longest):
    """one corridor through the whole grid: the longest fill the instance can be asked for, field included"""
    n = 6
    tables, points = checkpoints(name, n)
    env = env_of(tables)
    env.reset(return_obs=False)
    dims = env.dims
    path = serpentine(dims.W, dims.H)
    L = len(path)
    recs = []
    for e in range(n):
        at = [path[(e * 37 + a * (L // 5)) % L] if (e, a) != (0, 0) else path[0] for a in range(dims.A)]
        recs.append(with_cells(dims, points[-1][e], path, at))
    recs = np.stack(recs)
    env.set_state(recs)
    tg = draw_targets(dims, recs, 8, 3)
    tg[:, :, 0] = path[-1]                                                       # every agent to the far end
    tg[:, :, 1] = path[0]                                                        # ... and to the near one
    want = nav.host_navigate(dims, recs, tg)
    assert want[1][0, 0, 0] == L - 1 > longest, f"the corridor has {want[1][0, 0, 0]} steps from end to end"
    x0, y0 = path[0]
    assert int(want[2][0, 0, 0, x0 * dims.H + y0]) == L - 1, "the field of the far end at the near end"
    bufs = NavBufs(env, n, 8)
    for outputs in (OUTPUTS, ("action", "steps")):                               # both instantiations of the fill
        run(env, bufs, tg, outputs)
        bufs.check(f"{name} serpentine outputs={outputs}", outputs, want)
    env.close()


@pytest.mark.parametrize("name", ["huge_32x32", "dense_8x8"])
def test_walled_in_pocket(name):
    """an agent in a floor pocket with walls all around: every target outside gives -1, whatever lies outside"""
    n = 6
    tables, points = checkpoints(name, n)
    env = env_of(tables)
    env.reset(return_obs=False)
    dims = env.dims
    W, H = dims.W, dims.H
    pocket = [(W - 3, H - 3), (W - 2, H - 3), (W - 3, H - 2), (W - 2, H - 2)]
    outside_floor = [(x, y) for x in range(W - 4) for y in range(H)] + [(x, y) for x in range(W) for y in range(H - 4)]
    recs = np.stack([with_cells(dims, points[-1][e], pocket + outside_floor, [pocket[(e + a) % 4] for a in range(dims.A)]) for e in range(n)])
    env.set_state(recs)
    near = set(pocket) | {(x + dx, y + dy) for x, y in pocket for _c, dx, dy in nav.DELTAS}
    far = [(x, y) for x in range(W) for y in range(H) if (x, y) not in near]
    rng = np.random.default_rng(11)
    tg = np.array(far, dtype=np.int32)[rng.integers(0, len(far), (n, dims.A, 8))]
    want = nav.host_navigate(dims, recs, tg)
    assert (want[1] == -1).all() and (want[0] == 0).all(), "the host model walks out of the pocket"
    bufs = NavBufs(env, n, 8)
    run(env, bufs, tg)
    bufs.check(f"{name} pocket, targets outside", OUTPUTS, want)
    tg = np.array(sorted(near), dtype=np.int32)[rng.integers(0, len(near), (n, dims.A, 8))]    # inside and on the wall: reached
    want = nav.host_navigate(dims, recs, tg)
    assert (want[1] >= 0).all()
    run(env, bufs, tg)
    bufs.check(f"{name} pocket, targets inside", OUTPUTS, want)
    env.close()


def test_ranges_and_refusals():
    n = 13
    tables, points = checkpoints("coop_test", n)
    env = env_of(tables)
    env.reset(return_obs=False)
    recs = points[-1]
    env.set_state(recs)
    dims = env.dims
    for T in (1, 8):
        b = NavBufs(env, 5, T)                                                   # laid out for 5 envs, the guard right behind them
        tg = draw_targets(dims, recs[3:8], T, 5)
        run(env, b, tg, env_begin=3, env_count=5)
        b.check(f"envs 3..7 T={T}", OUTPUTS, nav.host_navigate(dims, recs[3:8], tg))
        run(env, b, tg, env_begin=7, env_count=0)
        b.check("env_count = 0", (), (None, None, None))
    b = NavBufs(env, n, 8)
    L = _native.lib()
    assert L.cz_nav_max_targets() == 8 == nav.MAX_TARGETS
    P = lambda f: b.buf[f].ptr
    tp = b.target.ptr
    for args, msg in (((0, n, 8, 0, tp, None, None, None), "null"), ((0, n, 0, 0, tp, P("action"), None, None), "T is 0"),
                      ((0, n, 9, 0, tp, P("action"), None, None), "T is 9"), ((0, n, 8, 2, tp, P("action"), None, None), "flags"),
                      ((0, n, 8, 0x80000001, tp, None, P("steps"), None), "flags"), ((10, 5, 8, 0, tp, P("action"), None, None), "range"),
                      ((-1, 2, 8, 0, tp, None, None, P("field")), "range"), ((0, n + 1, 1, 1, tp, P("action"), None, None), "range"),
                      ((0, n, 8, 0, None, P("action"), None, None), "d_target is null")):
        assert L.cz_navigate_device(env._h, *args) != 0, f"{args} was accepted"
        text = L.cz_last_error(env._h).decode()
        assert msg in text, f"{args}: message {text!r}"
    with pytest.raises(_native.NativeError, match="null"):
        env.navigate_device(b.target)
    with pytest.raises(ValueError, match="shape"):
        env.navigate_device(b.buf["action"], d_action=b.buf["action"])
    b.check("after the refusals", (), (None, None, None))
    assert np.array_equal(env.get_state(), recs), "a call wrote a record"
    env.close()


def pick_target(dims, records, kind):
    """the cell of type `kind` that is farthest from the nearest agent, every env's agent getting there in at least 2 steps"""
    cells = soa.record_cells(dims, records[0]) & soa.CELL_TYPE_MASK
    best = None
    for c in np.nonzero(cells == kind)[0]:
        x, y = int(c) % dims.W, int(c) // dims.W
        tg = np.broadcast_to(np.array([x, y], np.int32), (len(records), dims.A, 1, 2))
        steps = nav.host_navigate(dims, records, tg)[1]
        if steps.min() >= 2 and (best is None or steps.min() > best[0]):
            best = (int(steps.min()), (x, y))
    assert best is not None, "no such cell"
    return best[1]


@pytest.mark.parametrize("kind", [FLOOR, COUNTER], ids=["floor", "counter"])
def test_closed_loop_with_no_host_in_it(kind):
    """navigate_device -> step_device on the stream with nothing in between, for as many steps as the first call reported: the
    records are the oracle's under the host model's actions, and the agent stands on the target (next to it: a Counter)"""
    n = 6
    tables = case_tables("dense_8x8", n)
    assert tables.dims.A == 1 and CASES["dense_8x8"][4] == "scheme3"
    env = env_of(tables)
    orc = oracle_for(env)
    env.reset(return_obs=False)
    orc.reset()
    dims = env.dims
    target = pick_target(dims, orc.records, kind)
    tg = np.broadcast_to(np.array(target, np.int32), (n, 1, 1, 2)).copy()
    d_t, d_act, d_steps0, d_steps = env.alloc((n, 1, 1, 2), np.int32), env.alloc((n, 1), np.int32), env.alloc((n, 1, 1), np.int32), env.alloc((n, 1, 1), np.int32)
    d = dict(rew=env.alloc((n, 1), np.float64), term=env.alloc((n, 1), np.uint8), trunc=env.alloc((n, 1), np.uint8))
    d_t.from_host(tg)
    env.navigate_device(d_t, d_steps=d_steps0)
    first = d_steps0.to_host().reshape(n)
    want_first = nav.host_navigate(dims, orc.records, tg)[1].reshape(n)
    assert np.array_equal(first, want_first) and first.min() >= 2, f"steps of the first call {first.tolist()}, host model {want_first.tolist()}"
    assert len(set(first.tolist())) > 1, "every env is equally far from the target"
    for _ in range(int(first.max())):
        env.navigate_device(d_t, d_act, d_steps)
        env.step_device(d_act, None, d["rew"], d["term"], d["trunc"])
    for t in range(int(first.max())):
        acts = nav.host_navigate(dims, orc.records, tg)[0].reshape(n, 1)
        orc.step(acts, want_obs=False)
    assert np.array_equal(strip(env.get_state()), strip(orc.records)), "the records differ from the oracle's under the host model's actions"
    off = np.abs(agent_cells(dims, orc.records).reshape(n, 2) - np.array(target)).sum(axis=1)
    assert (off == (0 if kind == FLOOR else 1)).all(), f"agents at {agent_cells(dims, orc.records).reshape(n, 2).tolist()}, target {target}"
    assert (orc.records[:, soa.W_EPISODE] == orc.records[0, soa.W_EPISODE]).all() and int(orc.records[:, soa.W_T].min()) == int(first.max())
    env.close()


def test_captured_into_a_callers_graph():
    """[navigate_device, step_device] captured once, replayed on two different states"""
    n = 6
    tables, points = checkpoints("crowded_6x5", n)
    env = env_of(tables)
    orc = oracle_for(env)
    env.reset(return_obs=False)
    orc.reset()
    dims = env.dims
    A = dims.A
    b = NavBufs(env, n, 1)
    d_act = env.alloc((n, A), np.int32)
    d = dict(rew=env.alloc((n, A), np.float64), term=env.alloc((n, A), np.uint8), trunc=env.alloc((n, A), np.uint8))
    before = env.get_state()
    cs = CallerStream(env)
    with cs.capture():
        env.navigate_device(b.target, d_act, b.buf["steps"], b.buf["field"], walkable_blocks=True, T=1)
        env.step_device(d_act, None, d["rew"], d["term"], d["trunc"])
    assert np.array_equal(env.get_state(), before), "capturing executed something"
    for r, recs in enumerate((points[1], points[-1])):
        env.set_state(recs)
        orc.records[:] = recs
        tg = draw_targets(dims, recs, 1, 40 + r)
        b.fill()
        b.target.from_host(tg)
        d_act.from_host(np.full((n, A), 0x5A5A5A5A, np.int32))
        cs.replay()
        cs.sync()
        want = nav.host_navigate(dims, recs, tg, True)
        assert np.array_equal(d_act.to_host(), want[0].reshape(n, A)), f"replay {r}: actions"
        b.check(f"replay {r}", ("steps", "field"), want)
        orc.step(want[0].reshape(n, A), want_obs=False)
        assert np.array_equal(strip(env.get_state()), strip(orc.records)), f"replay {r}: records behind the captured step"
    cs.close()
    env.close()


def test_sharded_unequal_shards():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n = 13
    level, meta, agents, recipes, scheme, _inst, _steps = CASES["crowded_6x5"]
    tables, points = checkpoints("crowded_6x5", n)
    sh = ShardedVecEnv(n, level, meta, agents, 241, recipes, device_ids=[0, 0], action_scheme=scheme, num_layouts=4)
    assert [s.num_envs for s in sh.shards] == [7, 6]
    sh.reset(return_obs=False)
    recs = points[-1]
    sh.set_state(recs)
    dims = tables.dims
    C = dims.W * dims.H
    for T in (1, 8):
        tg = draw_targets(dims, recs, T, 60 + T)
        d_t, d_a, d_s, d_f = sh.alloc((agents, T, 2), np.int32), sh.alloc((agents, T), np.int32), sh.alloc((agents, T), np.int32), sh.alloc((agents, T, C), np.uint16)
        d_t.from_host(tg)
        sh.navigate_device(d_t, d_a, d_s, d_f)
        sh.sync()
        want = nav.host_navigate(dims, recs, tg)
        for got, w, what in zip((d_a, d_s, d_f), want, OUTPUTS):
            assert np.array_equal(got.to_host(), w), f"T={T}: {what} over the shards differs from the host model"
    sh.close()


def test_host_convenience():
    tables, points = checkpoints("limit_8x31", 6)
    env = env_of(tables)
    env.reset(return_obs=False)
    recs = points[1]
    env.set_state(recs)
    dims = env.dims
    for T in (1, 5):
        tg = draw_targets(dims, recs, T, 80 + T)
        act, steps = env.navigate(tg)
        want = nav.host_navigate(dims, recs, tg)
        assert act.dtype == steps.dtype == np.int32 and act.shape == steps.shape == (6, dims.A, T)
        assert np.array_equal(act, want[0]) and np.array_equal(steps, want[1])
    act, steps = env.navigate(tg[2:5], walkable_blocks=True, env_begin=2, env_count=3)
    want = nav.host_navigate(dims, recs[2:5], tg[2:5], True)
    assert np.array_equal(act, want[0]) and np.array_equal(steps, want[1])
    act, steps = env.navigate(np.zeros((0, dims.A, 1, 2), np.int32), env_count=0)
    assert act.shape == (0, dims.A, 1)
    env.close()
