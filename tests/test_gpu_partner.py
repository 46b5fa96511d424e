"""The scripted partner on the device (cz_partner_device, k_partner): exact against `partner.host_partner` of the oracle's records
on every kernel instance and agent count, with the envs' own recipes and with overrides that cover the book; every answer of the
unmodified reference's CookingAgent; output subsets and agent masks with sentinels and guards; refusals and ranges; ties that the
static list order decides; device-generated layouts; long corridors and pockets; the closed loop with the step on the stream, also
inside a caller's graph; unequal shards; despawned agents; the host convenience."""
import numpy as np
import pytest

from cooking_zoo_amd import _native, partner, soa
from cooking_zoo_amd.cooking_book import recipe_drawer
from cooking_zoo_amd.cooking_world.layout import Layout
from grid_common import CASES, case_tables, checkpoints
from nav_common import serpentine, with_cells
from partner_common import (KAT_ACTIONS, KAT_REWARD, OUTPUT_SUBSETS, OUTPUTS, PartnerBufs, book_of, golden, kat_tables, override_indices)
from vec_common import CallerStream, env_of, instance, make_env

pytestmark = pytest.mark.gpu
CUTBOARD = soa.STATIC_CLASSES.index("Cutboard")


def run(env, bufs, outputs=OUTPUTS, **kw):
    bufs.fill()
    env.partner_device(**bufs.args(outputs), **kw)


RUNS = [(name, False) for name in CASES] + [("coop_test", True), ("crowded_6x5", True)]


@pytest.mark.parametrize("name,spawn", RUNS, ids=[f"{n}{'-spawn' if s else ''}" for n, s in RUNS])
def test_every_case_against_the_host_model(name, spawn):
    """set_state(oracle records) then the call: the kernel is a pure function of the record.  Every checkpoint with the envs' own
    recipes; the last one in all 7 subsets of the outputs and with recipe overrides that cover every name of the book.  With
    despawn / respawn on, a despawned agent is ABSENT."""
    n = 6
    tables, points = checkpoints(name, n, spawn)
    env = env_of(tables)
    assert instance(env) == CASES[name][5], "the case runs on another kernel instance"
    env.reset(return_obs=False)
    dims, book = env.dims, book_of(tables)
    R = len(book)
    bufs = PartnerBufs(env, n)
    d_idx = env.alloc((n, dims.A), np.int32)
    seen = set()
    for k, recs in enumerate(points):
        env.set_state(recs)
        last = k == len(points) - 1
        want = partner.host_partner(dims, tables.layouts, recs, book)
        seen |= set(np.unique(want[2]).tolist())
        for outputs in (OUTPUT_SUBSETS if last else [OUTPUTS]):
            run(env, bufs, outputs)
            bufs.check(f"{name} checkpoint {k} own recipes outputs={outputs}", outputs, want)
        for shift in (range(0, R, 2) if last else ()):
            idx = override_indices(n, dims.A, R, shift)
            d_idx.from_host(idx)
            want = partner.host_partner(dims, tables.layouts, recs, book, recipe_idx=idx)
            seen |= set(np.unique(want[2]).tolist())
            run(env, bufs, d_recipe=d_idx)
            bufs.check(f"{name} checkpoint {k} recipes {idx.tolist()}", OUTPUTS, want)
        assert np.array_equal(env.get_state(), recs), "the call wrote a record"
    assert partner.WALK in seen and (not spawn or partner.ABSENT in seen), seen
    assert env.partner_bad_recipes() == 0
    env.close()


STEPPED = [("coop_test", 300), ("crowded_6x5", 300), ("dense_16x16", 300), ("large_16x16", 300), ("huge_20x20", 200)]


@pytest.mark.parametrize("name,steps", STEPPED, ids=[c[0] for c in STEPPED])
def test_states_the_device_stepped_itself(name, steps):
    """a few hundred DEVICE steps into biased-fuzz episodes (the state-aware policy's actions, auto-reset on), on every kernel
    instance: the records the step kernels left behind, read back, against the host model - every 100 steps, with the envs' own
    recipes and with overrides"""
    from vec_common import oracle_for, policy, strip
    n = 6
    tables = case_tables(name, n)
    env = env_of(tables)
    orc = oracle_for(env)
    env.reset(return_obs=False)
    orc.reset()
    dims, book = env.dims, book_of(tables)
    pol = policy(env, 9)
    A = dims.A
    d_act, d_idx = env.alloc((n, A), np.int32), env.alloc((n, A), np.int32)
    d = dict(rew=env.alloc((n, A), np.float64), term=env.alloc((n, A), np.uint8), trunc=env.alloc((n, A), np.uint8))
    bufs = PartnerBufs(env, n)
    seen = set()
    for t in range(1, steps + 1):
        acts = pol.act(orc.records)
        orc.step(acts, want_obs=False)
        pol.observe_result(orc.records)
        d_act.from_host(np.ascontiguousarray(acts, dtype=np.int32))
        env.step_device(d_act, None, d["rew"], d["term"], d["trunc"])
        if t % 100:
            continue
        recs = env.get_state()
        assert np.array_equal(strip(recs), strip(orc.records)), f"{name} step {t}: the device's records are not the oracle's"
        want = partner.host_partner(dims, tables.layouts, recs, book)
        run(env, bufs)
        bufs.check(f"{name} after {t} device steps, own recipes", OUTPUTS, want)
        idx = override_indices(n, A, len(book), t // 100)
        d_idx.from_host(idx)
        want2 = partner.host_partner(dims, tables.layouts, recs, book, recipe_idx=idx)
        run(env, bufs, d_recipe=d_idx)
        bufs.check(f"{name} after {t} device steps, recipes {idx.tolist()}", OUTPUTS, want2)
        seen |= set(np.unique(want[2]).tolist()) | set(np.unique(want2[2]).tolist())
    assert partner.WALK in seen, seen
    env.close()


def golden_env(ep):
    """an env whose one layout is the episode's (its static lists are the reference's), holding the stored records"""
    gd = soa.Dims(*ep["dims"])
    rec0 = np.array(ep["states"][0]["record"], dtype=np.uint32)
    cells = soa.record_cells(gd, rec0) & soa.CELL_TYPE_MASK
    classes, xy = [], []
    for s in range(gd.D):
        x, y, c, f = soa.unpack_dyn0(rec0[gd.dyn0_word0 + s])
        if f & soa.DYN_ALIVE:
            if not classes or classes[-1][0] != c:
                classes.append([c, 0])
            classes[-1][1] += 1
            xy.append((x, y))
    agents = [soa.unpack_agent(rec0[soa.AGENT_WORD0 + a])[:2] for a in range(gd.A)]
    layout = Layout(gd.W, gd.H, cells, {k: list(v) for k, v in ep["static_lists"].items()}, classes, xy, agents)
    meta = {"coop_test": "example", "switch_test": "example"}.get(ep["level"], ep["level"])
    n = len(ep["states"])
    env = make_env(n, ep["level"], meta, gd.A, ep["recipes"], ep["scheme"], max_steps=500, layouts=[layout], max_dyn=gd.D, auto_reset=False)
    assert env.dims.as_tuple() == gd.as_tuple()
    env.reset(return_obs=False)
    recs = np.array([st["record"] for st in ep["states"]], dtype=np.uint32)
    env.set_state(recs)
    return env, layout, recs


N_EPISODES = 11


@pytest.mark.parametrize("k", range(N_EPISODES))
def test_against_the_reference(k):
    """the records of tests/golden/partner_ref.json.gz on the device: every stored answer of the unmodified CookingAgent - the
    action, the walk's target where a walk produced it, RAISES exactly where it raised"""
    doc = golden()
    assert len(doc["episodes"]) == N_EPISODES
    ep = doc["episodes"][k]
    env, _layout, recs = golden_env(ep)
    n, A = len(recs), env.num_agents
    bufs = PartnerBufs(env, n)
    d_idx = env.alloc((n, A), np.int32)
    checked = 0
    for r in range(len(doc["recipe_names"])):
        asked = [(e, ans) for e, st in enumerate(ep["states"]) for ans in st["answers"] if ans[1] == r]
        if not asked:
            continue
        d_idx.from_host(np.full((n, A), r, np.int32))
        run(env, bufs, d_recipe=d_idx)
        act, tg, st = (bufs.read(f)[0] for f in OUTPUTS)
        for e, ans in asked:
            a = ans[0]
            ctx = f"{ep['set']} step {ep['states'][e]['step']} agent {a} {doc['recipe_names'][r]}: stored {ans[2:]}, device {act[e, a]} {tg[e, a].tolist()} {st[e, a]}"
            if isinstance(ans[2], str):
                assert st[e, a] == partner.RAISES and act[e, a] == 0, ctx
            else:
                assert st[e, a] != partner.RAISES and act[e, a] == ans[2], ctx
                if st[e, a] == partner.WALK:
                    assert ans[3] > 0 and tuple(tg[e, a]) == (ans[4], ans[5]), ctx
                else:
                    assert tuple(tg[e, a]) == (-1, -1) and act[e, a] == 0, ctx
            checked += 1
    assert checked == sum(len(st["answers"]) for st in ep["states"])
    env.close()


def test_ties_the_static_list_order_decides():
    """coop_test states in which two Cutboards or Counters are equally near and the list order is not the cell order: the device
    gives the reference's answer, which differs from the one cell order would give"""
    doc = golden()
    book = [recipe_drawer.RECIPES[nm]() for nm in doc["recipe_names"]]
    decided = 0
    for ep in doc["episodes"]:
        if ep["level"] != "coop_test" or decided:
            continue
        assert any(sorted(v) != list(v) for v in ep["static_lists"].values())
        dims = soa.Dims(*ep["dims"])
        recs = np.array([st["record"] for st in ep["states"]], dtype=np.uint32)
        cells = soa.record_cells(dims, recs[0]) & soa.CELL_TYPE_MASK
        ascending = Layout(dims.W, dims.H, cells, {k: sorted(v) for k, v in ep["static_lists"].items()}, [], [], [])
        listed = Layout(dims.W, dims.H, cells, {k: list(v) for k, v in ep["static_lists"].items()}, [], [], [])
        n, A = len(recs), dims.A
        wants = []
        for r in range(len(book)):
            idx = np.full((n, A), r, np.int32)
            want = partner.host_partner(dims, [listed], recs, book, recipe_idx=idx)
            other = partner.host_partner(dims, [ascending], recs, book, recipe_idx=idx)
            wants.append((idx, want))
            decided += int((want[1] != other[1]).any(axis=-1).sum())
        if not decided:
            continue
        env, _layout, _recs = golden_env(ep)
        bufs = PartnerBufs(env, n)
        d_idx = env.alloc((n, A), np.int32)
        for idx, want in wants:
            d_idx.from_host(idx)
            run(env, bufs, d_recipe=d_idx)
            bufs.check(f"{ep['set']} recipe {idx[0, 0]}", OUTPUTS, want)
        env.close()
    assert decided > 0, "no answer depends on the list order"


def test_agent_masks_leave_the_other_agents_alone():
    for name, masks in (("coop_test", (1, 2, 3)), ("crowded_6x5", (1, 8, 5, 10, 14, 15))):
        tables, points = checkpoints(name, 6)
        env = env_of(tables)
        env.reset(return_obs=False)
        env.set_state(points[-1])
        want = partner.host_partner(env.dims, tables.layouts, points[-1], book_of(tables))
        bufs = PartnerBufs(env, 6)
        for m in masks:
            for outputs in (OUTPUTS, ("action",), ("target", "status")):
                run(env, bufs, outputs, agents=m)
                bufs.check(f"{name} agents={m:#x} outputs={outputs}", outputs, want, agents=m)
        env.close()


def test_ranges_and_refusals():
    n = 13
    tables, points = checkpoints("coop_test", n)
    env = env_of(tables)
    env.reset(return_obs=False)
    recs = points[-1]
    env.set_state(recs)
    book = book_of(tables)
    b = PartnerBufs(env, 5)                                                      # laid out for 5 envs, the guard right behind them
    run(env, b, env_begin=3, env_count=5)
    b.check("envs 3..7", OUTPUTS, partner.host_partner(env.dims, tables.layouts, recs[3:8], book))
    run(env, b, env_begin=7, env_count=0)
    b.check("env_count = 0", (), (None, None, None))
    b = PartnerBufs(env, n)
    L = _native.lib()
    P = lambda f: b.buf[f].ptr
    for args, msg in (((0, n, 3, 0, None, None, None, None), "null"), ((0, n, 0, 0, None, P("action"), None, None), "agents"),
                      ((0, n, 4, 0, None, P("action"), None, None), "agents"), ((0, n, 0x80000001, 0, None, P("action"), None, None), "agents"),
                      ((0, n, 3, 1, None, P("action"), None, None), "flags"), ((10, 5, 3, 0, None, P("action"), None, None), "range"),
                      ((-1, 2, 3, 0, None, None, None, P("status")), "range"), ((0, n + 1, 1, 0, None, P("action"), None, None), "range")):
        assert L.cz_partner_device(env._h, *args) != 0, f"{args} was accepted"
        text = L.cz_last_error(env._h).decode()
        assert msg in text, f"{args}: message {text!r}"
    with pytest.raises(_native.NativeError, match="null"):
        env.partner_device()
    # a recipe index outside the table: IDLE, counted
    idx = override_indices(n, 2, len(book), 0)
    idx[::3, 0], idx[1::4, 1] = len(book), -1
    d_idx = env.alloc((n, 2), np.int32)
    d_idx.from_host(idx)
    before = env.partner_bad_recipes()
    run(env, b, d_recipe=d_idx)
    b.check("recipe indices outside the table", OUTPUTS, partner.host_partner(env.dims, tables.layouts, recs, book, recipe_idx=idx))
    gone = ((recs[:, soa.W_STATUS, None] >> (partner.SPAWN_GONE0 + np.arange(2))) & 1) != 0
    assert env.partner_bad_recipes() - before == int((((idx < 0) | (idx >= len(book))) & ~gone).sum())
    # what cz_load_partner_table itself refuses
    rows = np.ascontiguousarray(env.partner_rows)
    assert L.cz_load_partner_table(env._h, rows.ctypes.data, len(book) - 1) != 0 and "rows for the" in L.cz_last_error(env._h).decode()
    bad = rows.copy()
    bad[0, 1] |= 9 << 8
    assert L.cz_load_partner_table(env._h, bad.ctypes.data, len(book)) != 0 and "conditions" in L.cz_last_error(env._h).decode()
    assert np.array_equal(env.get_state(), recs), "a call wrote a record"
    env.close()
    bare = _native.lib()
    env2 = env_of(tables)
    env2.reset(return_obs=False)
    b2 = PartnerBufs(env2, n)
    env2.partner_device(b2.buf["action"])
    # a missing partner table: cz_load_recipes drops it (its rows were built from the book that call replaces), whatever the new
    # book's size; cz_load_partner_table brings the call back
    _native.check(env2._h, bare.cz_load_recipes(env2._h, env2.recipe_table.ctypes.data, len(env2.book_names), env2.recipe_nodes))
    b2.fill()
    assert bare.cz_partner_device(env2._h, 0, n, 3, 0, None, b2.buf["action"].ptr, None, None) != 0, "accepted without a partner table"
    assert "no partner table" in bare.cz_last_error(env2._h).decode(), bare.cz_last_error(env2._h).decode()
    with pytest.raises(_native.NativeError, match="cz_load_partner_table"):
        env2.partner_device(b2.buf["action"], b2.buf["target"], b2.buf["status"])
    b2.check("refused without a partner table", (), (None, None, None))
    rows2 = np.ascontiguousarray(env2.partner_rows)
    _native.check(env2._h, bare.cz_load_partner_table(env2._h, rows2.ctypes.data, len(env2.book_names)))
    env2.set_state(recs)
    run(env2, b2)
    b2.check("after cz_load_partner_table", OUTPUTS, partner.host_partner(env2.dims, tables.layouts, recs, book))
    env2.update_layouts(0, [env2.layouts[1]])                                    # the rank rows follow the layouts
    env2.partner_device(b2.buf["action"])
    lay = env2.layouts[0]
    recs0 = np.stack([lay.init_record(env2.dims, 0)])
    desc = np.stack([lay.obs_descriptor(env2.meta, env2.dims)])
    _native.check(env2._h, bare.cz_update_layouts(env2._h, 0, 1, recs0.ctypes.data, desc.ctypes.data))
    assert bare.cz_partner_device(env2._h, 0, n, 3, 0, None, b2.buf["action"].ptr, None, None) != 0
    assert "rank row" in bare.cz_last_error(env2._h).decode()
    env2.close()


def test_device_generated_layouts():
    """after generate_layouts the rank rows are the generator's own: the answers equal the host model on the host twin of the draw"""
    from layout_keyed_common import FOUR
    n = 8
    for level, meta, agents in (("coop_test", "example", 2), ("crowded_6x5", "crowded_6x5", 4), ("large_16x16", "large_16x16", 4)):
        env = make_env(n, level, meta, agents, FOUR[:agents], "scheme3", max_steps=50, num_layouts=4)
        env.generate_layouts(0, 4, generation=3, seed=17)
        assert env.generate_failures() == 0
        env.reset(return_obs=False)
        recs = env.get_state()
        assert len(set(recs[:, soa.W_LAYOUT].tolist())) > 1
        book = book_of(env.tables)
        bufs = PartnerBufs(env, n)
        d_idx = env.alloc((n, agents), np.int32)
        for shift in range(0, len(book), 3):
            idx = override_indices(n, agents, len(book), shift)
            d_idx.from_host(idx)
            run(env, bufs, d_recipe=d_idx)
            bufs.check(f"{level} generated, recipes shift {shift}", OUTPUTS, partner.host_partner(env.dims, env.layouts, recs, book, recipe_idx=idx))
        env.close()


@pytest.mark.parametrize("name", ["huge_32x32", "dense_8x8"])
def test_long_corridor_and_cut_corridor(name):
    """one corridor through the whole grid, a Tomato and a Cutboard at its far end: a long fill and a long walk; with the corridor
    cut, the Tomato is unreachable (the walk returns 0) and no Cutboard can be reached (`closest` finds none: RAISES)"""
    n = 6
    tables, points = checkpoints(name, n)
    env = env_of(tables)
    env.reset(return_obs=False)
    dims, book = env.dims, book_of(tables)
    path = serpentine(dims.W, dims.H)
    fx, fy = path[-1]
    side = [(fx + dx, fy + dy) for dx, dy in ((0, 1), (0, -1), (1, 0), (-1, 0)) if 0 <= fx + dx < dims.W and 0 <= fy + dy < dims.H and (fx + dx, fy + dy) not in path]
    assert len(side) >= 2
    recs = []
    for e in range(n):
        floor = path if e % 2 == 0 else path[:len(path) // 2] + path[len(path) // 2 + 1:]
        rec = with_cells(dims, points[-1][e], floor, [path[(3 * a + e) % 7] for a in range(dims.A)])
        soa.record_cells(dims, rec)[side[0][1] * dims.W + side[0][0]] = CUTBOARD
        for s in range(dims.D):                                                 # one Tomato, fresh, at the far end; nothing else alive
            rec[dims.dyn0_word0 + s], rec[dims.dyn1_word0 + s] = 0, 0
        rec[dims.dyn0_word0] = soa.pack_dyn0(side[1][0], side[1][1], soa.TOMATO, soa.DYN_ALIVE | soa.DYN_FREE)
        for a in range(dims.A):
            rec[soa.AGENT_WORD0 + a] &= 0x00FFFFFF                              # empty hands
        rec[soa.W_STATUS] = 0
        recs.append(rec)
    recs = np.stack(recs)
    env.set_state(recs)
    idx = np.full((n, dims.A), tables.book_names.index("TomatoSalad"), np.int32)
    want = partner.host_partner(dims, tables.layouts, recs, book, recipe_idx=idx)
    assert (want[2][0::2] == partner.WALK).all() and (want[0][0::2] != 0).all() and (want[1][0::2] == side[1]).all(), "the open corridor"
    assert (want[2][1::2] == partner.RAISES).all() and (want[0][1::2] == 0).all(), "the cut corridor: no Cutboard in reach, `closest` finds none"
    d_idx = env.alloc((n, dims.A), np.int32)
    d_idx.from_host(idx)
    bufs = PartnerBufs(env, n)
    run(env, bufs, d_recipe=d_idx)
    bufs.check(f"{name} corridor, Tomato at the far end", OUTPUTS, want)
    recs[:, dims.dyn0_word0] |= soa.DYN_CHOPPED << 24                           # chopped: the Plate node is next, and no Plate exists
    env.set_state(recs)
    want = partner.host_partner(dims, tables.layouts, recs, book, recipe_idx=idx)
    assert (want[2] == partner.RAISES).all(), want[2].tolist()
    run(env, bufs, d_recipe=d_idx)
    bufs.check(f"{name} corridor, no object of the node's class", OUTPUTS, want)
    recs[:, dims.dyn0_word0] = soa.pack_dyn0(0, 0, soa.PLATE, soa.DYN_ALIVE | soa.DYN_FREE)       # a Plate alone: a recipe whose ingredients the level lacks
    env.set_state(recs)
    idx[:] = tables.book_names.index("CarrotBanana")
    d_idx.from_host(idx)
    want = partner.host_partner(dims, tables.layouts, recs, book, recipe_idx=idx)
    run(env, bufs, d_recipe=d_idx)
    bufs.check(f"{name} corridor, a recipe without its ingredients", OUTPUTS, want)
    env.close()


def closed_loop(env, steps, d):
    n = env.num_envs
    for t in range(steps):
        act = d["act"].ptr + t * n * 4
        env.partner_device(act)
        env.step_device(act, None, d["rew"].ptr + t * n * 8, d["term"], d["trunc"])


def kat_env(n):
    tables, rec0 = kat_tables(n)
    env = env_of(tables)
    env.reset(return_obs=False)
    env.finished_episodes()
    d = dict(act=env.alloc((30, n, 1), np.int32), rew=env.alloc((30, n, 1), np.float64), term=env.alloc((n, 1), np.uint8), trunc=env.alloc((n, 1), np.uint8))
    return env, np.tile(rec0, (n, 1)), d


def check_kat(env, d, ctx):
    n = env.num_envs
    acts = d["act"].to_host().reshape(30, n)
    assert all("".join(map(str, acts[:, e])) == KAT_ACTIONS for e in range(n)), f"{ctx}: actions {''.join(map(str, acts[:, 0]))}"
    rew = d["rew"].to_host().reshape(30, n)
    assert (rew[29] == KAT_REWARD).all() and (rew[:29] == -0.0125).all(), f"{ctx}: rewards {rew[:, 0].tolist()}"
    assert (d["term"].to_host() == 1).all() and (d["trunc"].to_host() == 0).all(), f"{ctx}: the 30th step does not terminate"
    eps = env.finished_episodes()
    assert len(eps) == n and (eps["length"] == 30).all(), f"{ctx}: {len(eps)} episodes, lengths {sorted(set(eps['length'].tolist()))}"


def test_closed_loop_with_no_host_in_it():
    """64 envs from kat_c3's initial record: partner_device -> step_device 30 times on the stream, then one read: the pinned actions,
    19.9875 and termination at step 30, 64 episodes of length 30; then the same loop captured into a caller's graph and replayed"""
    n = 64
    env, recs, d = kat_env(n)
    env.set_state(recs)
    closed_loop(env, 30, d)
    check_kat(env, d, "direct")
    env.set_state(recs)
    env.finished_episodes()
    d["act"].from_host(np.full((30, n, 1), 0x5A5A5A5A, np.int32))
    cs = CallerStream(env)
    with cs.capture():
        closed_loop(env, 30, d)
    assert (d["act"].to_host() == 0x5A5A5A5A).all(), "capturing executed something"
    cs.replay()
    cs.sync()
    check_kat(env, d, "replayed graph")
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
    book = book_of(tables)
    idx = override_indices(n, agents, len(book), 1)
    want = partner.host_partner(tables.dims, tables.layouts, recs, book, recipe_idx=idx)
    d_a, d_t, d_s, d_r = sh.alloc((agents,), np.int32), sh.alloc((agents, 2), np.int32), sh.alloc((agents,), np.uint8), sh.alloc((agents,), np.int32)
    d_r.from_host(idx)
    sh.partner_device(d_a, d_t, d_s, d_recipe=d_r)
    sh.sync()
    for got, w, what in zip((d_a, d_t, d_s), want, OUTPUTS):
        assert np.array_equal(got.to_host(), w), f"{what} over the shards differs from the host model"
    own = partner.host_partner(tables.dims, tables.layouts, recs, book, agents=0b0110)
    for got, w in zip(sh.partner(agents=0b0110), own):
        assert np.array_equal(got, w), "the host convenience over the shards"
    for got, w in zip(sh.partner(recipes=idx), want):                            # [N, A]: every shard gets the rows of its envs
        assert np.array_equal(got, w), "the host convenience over the shards, recipes per env"
    with pytest.raises(ValueError, match="rows"):
        sh.partner(recipes=idx[:5])
    sh.close()


def test_host_convenience():
    tables, points = checkpoints("limit_8x31", 6)
    env = env_of(tables)
    env.reset(return_obs=False)
    recs = points[1]
    env.set_state(recs)
    book = book_of(tables)
    got = env.partner()
    want = partner.host_partner(env.dims, tables.layouts, recs, book)
    assert got[0].dtype == np.int32 and got[2].dtype == np.uint8 and got[1].shape == (6, 2, 2)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    names = ["CarrotBanana", "TomatoSalad"]
    idx = np.tile(np.array([tables.book_names.index(nm) for nm in names], np.int32), (3, 1))
    got = env.partner(agents=2, recipes=names, env_begin=2, env_count=3)
    want = partner.host_partner(env.dims, tables.layouts, recs[2:5], book, agents=2, recipe_idx=idx)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert env.partner(env_count=0)[1].shape == (0, 2, 2)
    env.close()
