"""GPU: tasks on the device - cz_set_tasks_device / k_set_tasks and cz_infos_device / k_infos against the host definition
(cooking_zoo_amd/tasks.py) and the oracle.  Everything is compared exactly: records word for word (running-return words stripped where
a step was taken), goal vectors, flags and indices as integers, float32 goals as bits, rewards as uint64.  Every output buffer of
`infos_device` is pre-filled with a sentinel and guarded on both sides."""
import ctypes as C
import functools

import numpy as np
import pytest

import matrix_common as mc
from cooking_zoo_amd import _native, partner, soa, tasks
from cooking_zoo_amd.cooking_book import recipe_drawer as rd
from fuzz_policy import BumperActions
from partner_common import OUTPUTS as PARTNER_OUTPUTS, PartnerBufs, book_of
from tasks_common import OUTPUT_SUBSETS, OUTPUTS, InfoBufs, fresh_user_registry, task_list_draws
from vec_common import COOP, CROWDED4, TWO, CallerStream, Outs, check_step, env_of, instance, last_lean, oracle_for, oracle_reset, strip, tables_of, widen

pytestmark = pytest.mark.gpu

TASK_LIST = np.array([[0, 1, 7, 200], [3, 2, 0xFF, 9], [1, 5, 77, 0]], dtype=np.uint8)     # K = 3; the bytes of slots >= R = 2 are junk
LOOP_SEED = 11


def model_call(tables, records, mask=None, ids=None, task_list=None, seed=0):
    """what one set_tasks_device call over the whole batch must make of `records`: (records, refused envs, chosen bool [n])"""
    records = np.asarray(records, dtype=np.uint32)
    chosen = (records[:, soa.W_T] == 0) if mask is None else (np.asarray(mask) != 0)
    new, refused = tasks.host_set_tasks(tables, records, chosen, recipe_ids=ids, task_list=None if ids is not None else task_list, seed=seed)
    return new, int(refused.sum()), chosen


class TaskBufs:
    """the inputs of set_tasks_device for one handle: mask, ids, a K-row list"""

    def __init__(self, env, K=len(TASK_LIST)):
        n = env.num_envs
        self.mask, self.ids, self.list = env.alloc((n,), np.uint8), env.alloc((n, 4), np.uint8), env.alloc((K, 4), np.uint8)


def check_infos(ctx, env, tables, records, bufs=None):
    b = bufs or InfoBufs(env, env.num_envs)
    b.fill()
    env.infos_device(**b.args(OUTPUTS))
    env.sync()
    b.check(ctx, OUTPUTS, tasks.host_infos(tables, records))
    return b


def follow_oracle(ctx, env, tables, records, steps, seed, outs=None, lean=None):
    """`steps` steps of step_device from `records` (the device holds them) against the oracle, which reads the recipe ids from the
    records: rewards, flags, float64 rows and records at every step"""
    orc = oracle_for(tables)
    orc.records[:] = records
    pol = BumperActions(tables.dims, tables.scheme_class.CODE, np.random.default_rng(seed))
    o = outs or Outs(env)
    for t in range(steps):
        acts = np.ascontiguousarray(pol.act(orc.records), dtype=np.int32)
        want = orc.step(acts)
        pol.observe_result(orc.records)
        got = o.step(env, acts)
        if lean is not None:
            assert last_lean(env) == lean, f"{ctx} step {t}: the launch's lean flag is {last_lean(env)}"
        check_step(f"{ctx} step {t}", got, want)
        mc.check_records(f"{ctx} step {t}", strip(env.get_state()), orc.records)
    return orc


# ---------------------------------------------------------------------------------------------------------------------------
# 1: the matrix
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", range(len(mc.CELLS)), ids=mc.CELL_IDS)
def test_matrix(cell):
    inst, agents, scheme = mc.CELLS[cell]
    n, max_dyn = 48, mc.INSTANCES[inst][0]
    tn, points = mc.natural_checkpoints(agents, scheme)
    t = tables_of(n, mc.LEVEL, mc.META, agents, CROWDED4[:agents], scheme, max_steps=mc.MAX_STEPS, num_layouts=mc.LAYOUTS, max_dyn=max_dyn)
    recs = widen(np.concatenate(list(points))[np.arange(n) % (mc.POINTS * mc.N)], tn.dims, t.dims)
    rng = np.random.default_rng(900 + cell)
    ids = rng.integers(0, 256, (n, 4)).astype(np.uint8)                 # (slots >= R: any byte)
    ids[:, :agents] = rng.integers(0, len(t.book_names), (n, agents))
    want, refused, _ = model_call(t, recs, np.ones(n), ids)
    assert refused == 0 and (want[:, soa.W_MARKS] != recs[:, soa.W_MARKS]).sum() >= n // 8, "the reassignment changes marks"
    env = env_of(t)
    try:
        assert instance(env) == inst and env.num_goals == 26
        b = TaskBufs(env)
        env.set_state(recs)
        b.mask.from_host(np.ones(n, np.uint8))
        b.ids.from_host(ids)
        env.set_tasks_device(b.mask, b.ids)
        mc.check_records(f"{mc.CELL_IDS[cell]}: set_tasks_device", env.get_state(), want)
        assert env.set_tasks_refused() == 0
        check_infos(f"{mc.CELL_IDS[cell]}: infos_device", env, t, want)
        mc.check_records(f"{mc.CELL_IDS[cell]}: get_state after infos_device", env.get_state(), want)
        follow_oracle(mc.CELL_IDS[cell], env, t, want, mc.STEP_T, 77 + cell)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2: output subsets and ranges
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def crowded_state(agents=4, n=13, steps=60):
    """a crowded_6x5 batch worked on for `steps` steps by the state-aware policy, then given random recipes by the host model"""
    t = tables_of(n, mc.LEVEL, mc.META, agents, CROWDED4[:agents], "scheme3", max_steps=mc.MAX_STEPS, num_layouts=mc.LAYOUTS)
    orc = oracle_for(t)
    orc.reset()
    pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(5))
    for _ in range(steps):
        orc.step(pol.act(orc.records), want_obs=False)
        pol.observe_result(orc.records)
    ids = np.random.default_rng(6).integers(0, len(t.book_names), (n, 4)).astype(np.uint8)
    recs, refused, _ = model_call(t, orc.records, np.ones(n), ids)
    assert refused == 0
    recs.setflags(write=False)
    return t, recs, ids


def test_every_subset_of_outputs_and_ranges():
    t, recs, _ = crowded_state()
    n = t.num_envs
    env = env_of(t)
    try:
        env.set_state(recs)
        goal = tasks.host_infos(t, recs)[0]
        assert goal.any() and not goal.all()
        for begin, count in ((0, n), (3, 5), (n - 1, 1), (0, 4)):       # (4 envs: one whole workgroup; 5 and 13: a part of the last one)
            b = InfoBufs(env, count)
            for outputs in OUTPUT_SUBSETS:
                b.fill()
                env.infos_device(env_begin=begin, env_count=count, **b.args(outputs))
                env.sync()
                b.check(f"envs [{begin}, {begin + count}) outputs {outputs}", outputs, tasks.host_infos(t, recs[begin:begin + count]))
        env.infos_device(env_begin=n, env_count=0, **b.args(OUTPUTS))   # an empty range: nothing to do
        mc.check_records("get_state after infos_device", env.get_state(), recs)
        got = env.infos()
        want = tasks.host_infos(t, recs)
        for k, w in zip(("goal_vector", "recipe_done", "task", "t"), want):
            mc.check_equal(f"infos()[{k!r}]", got[k], w)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3: who is chosen
# ---------------------------------------------------------------------------------------------------------------------------

def test_choice_rules():
    n, seed = 67, 21
    t = tables_of(n, **dict(COOP, max_steps=5))
    env, orc = env_of(t, auto_reset=False), oracle_for(t, auto_reset=0)
    try:
        o, b = Outs(env, skip=("obs",)), TaskBufs(env)
        b.list.from_host(TASK_LIST)
        env.reset(return_obs=False)
        orc.reset()
        pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(3))

        def step(k):
            for _ in range(k):
                acts = np.ascontiguousarray(pol.act(orc.records), dtype=np.int32)
                check_step("step", o.step(env, acts), orc.step(acts))
                pol.observe_result(orc.records)

        def reset(mask):
            b.mask.from_host(mask.astype(np.uint8))
            env.reset_device(b.mask)
            for e in np.nonzero(mask)[0]:
                oracle_reset(orc, int(e))

        step(2)
        reset(np.arange(n) % 3 == 0)                                    # a third starts over: t = 0, then 3; the others reach t = 5
        step(3)
        done = (orc.records[:, soa.W_STATUS] & 1) != 0
        assert done.sum() >= n // 2 and (~done).sum() >= n // 4
        reset(done & (np.arange(n) % 2 == 0))                           # half of the finished envs: t = 0
        recs = orc.records.copy()
        mc.check_records("the prepared batch", strip(env.get_state()), recs)
        fresh, live = recs[:, soa.W_T] == 0, (recs[:, soa.W_T] != 0) & ((recs[:, soa.W_STATUS] & 1) == 0)
        finished = (recs[:, soa.W_STATUS] & 1) != 0
        assert fresh.sum() >= 10 and live.sum() >= 10 and finished.sum() >= 10 and not (fresh & finished).any()
        stats0 = env.stats()
        # no mask: exactly the envs at t == 0, each with the row its (global id, episode) draws
        want, refused, chosen = model_call(t, recs, None, None, TASK_LIST, seed)
        assert refused == 0 and np.array_equal(chosen, fresh)
        draws = task_list_draws(t, recs, TASK_LIST, seed)
        assert set(draws[fresh].tolist()) == {0, 1, 2}, "every row of the list is drawn by an env at the start of its episode"
        env.set_tasks_device(None, None, b.list, seed=seed)
        got = strip(env.get_state())
        mc.check_records("no mask: the envs at t == 0", got[fresh], want[fresh])
        mc.check_records("no mask: every env not chosen is byte-identical", got[~fresh], recs[~fresh])
        assert (got[fresh][:, soa.W_RECIPES] != recs[fresh][:, soa.W_RECIPES]).sum() >= fresh.sum() // 2
        env.set_tasks_device(None, None, b.list, seed=seed)
        mc.check_records("a second identical keyed call changes nothing", strip(env.get_state()), want)
        # a mask: mid-episode and finished envs; a finished env stays finished
        mask = ((np.arange(n) % 4 == 1) & ~fresh).astype(np.uint8) * 0x80
        assert (mask != 0)[live].sum() >= 3 and (mask != 0)[finished].sum() >= 3
        ids = np.random.default_rng(8).integers(0, len(t.book_names), (n, 4)).astype(np.uint8)
        want2, refused, chosen = model_call(t, want, mask, ids)
        assert refused == 0
        b.mask.from_host(mask)
        b.ids.from_host(ids)
        env.set_tasks_device(b.mask, b.ids, b.list, seed=seed)          # (ids win over the list)
        got = strip(env.get_state())
        mc.check_records("a mask: chosen envs", got[chosen], want2[chosen])
        mc.check_records("a mask: every env not chosen is byte-identical", got[~chosen], want[~chosen])
        assert np.array_equal(got[:, soa.W_STATUS], recs[:, soa.W_STATUS]) and np.array_equal(got[:, soa.W_T], recs[:, soa.W_T])
        assert env.set_tasks_refused() == 0
        assert env.stats() == stats0, "no statistics change"
        check_infos("after the masked call", env, t, want2)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4: refusals
# ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_and_host_side_errors():
    n, seed = 29, 4
    t = tables_of(n, **COOP)
    R, n_rec = t.num_recipes, len(t.book_names)
    env = env_of(t)
    try:
        env.reset(return_obs=False)
        recs = env.get_state()
        b = TaskBufs(env)
        rng = np.random.default_rng(1)
        ids = rng.integers(0, n_rec, (n, 4)).astype(np.uint8)
        ids[:, R:] = rng.integers(n_rec, 256, (n, 4 - R))               # slots >= R: ignored, stored as 0xFF
        bad = np.arange(n) % 5 == 2
        ids[bad, rng.integers(0, R, bad.sum())] = rng.choice([n_rec, n_rec + 1, 0x7F, 0xFF], bad.sum())
        want, refused, _ = model_call(t, recs, np.ones(n), ids)
        assert refused == bad.sum() > 0
        b.mask.from_host(np.ones(n, np.uint8))
        b.ids.from_host(ids)
        env.set_tasks_device(b.mask, b.ids)
        got = env.get_state()
        mc.check_records("ids: a refused env is untouched", got[bad], recs[bad])
        mc.check_records("ids: the other envs are served", got[~bad], want[~bad])
        assert ((got[~bad][:, soa.W_RECIPES] >> (8 * R)) == (0xFFFFFFFF >> (8 * R))).all()
        assert env.set_tasks_refused() == refused
        # from a row of the task list
        tl = TASK_LIST.copy()
        tl[1, 1] = n_rec
        draws = task_list_draws(t, got, tl, seed)
        assert (draws == 1).any() and (draws != 1).any()
        want2, refused2, chosen = model_call(t, got, None, None, tl, seed)
        assert chosen.all() and refused2 == (draws == 1).sum()
        b.list.from_host(tl)
        env.set_tasks_device(d_task_list=b.list, seed=seed)
        got2 = env.get_state()
        mc.check_records("list: the envs that draw the bad row are untouched", got2[draws == 1], got[draws == 1])
        mc.check_records("list: the other envs are served", got2[draws != 1], want2[draws != 1])
        assert env.set_tasks_refused() == refused + refused2
        # host-side errors, before anything is launched
        for kw in (dict(), dict(d_mask=b.mask), dict(d_task_list=b.list, K=0), dict(d_task_list=b.list, K=-3)):
            with pytest.raises(_native.NativeError):
                env.set_tasks_device(**kw)
        with pytest.raises(_native.NativeError):
            env.infos_device()
        with pytest.raises(_native.NativeError):
            env.infos_device(d_t=env.alloc((n,), np.int32), env_begin=1)            # a range outside the batch
        mc.check_records("the refused calls changed nothing", env.get_state(), got2)
        # cz_load_recipes drops the goal table, as it drops the partner table
        L = _native.lib()
        assert L.cz_num_goals(env._h) == 26
        _native.check(env._h, L.cz_load_recipes(env._h, t.recipe_table.ctypes.data_as(C.c_void_p), n_rec, t.recipe_nodes))
        assert L.cz_num_goals(env._h) == -1
        with pytest.raises(_native.NativeError):
            env.infos_device(d_t=env.alloc((n,), np.int32))
        for table, rows, G in ((t.goal_table, n_rec - 1, 26), (t.goal_table, n_rec, 0), (t.goal_table, n_rec, 256),
                               (np.where(t.goal_table == 25, 26, t.goal_table).astype(np.uint8), n_rec, 26),
                               (np.where(t.goal_table == 0xFF, 3, t.goal_table).astype(np.uint8), n_rec, 26)):
            table = np.ascontiguousarray(table)
            assert L.cz_load_goal_table(env._h, table.ctypes.data_as(C.c_void_p), rows, G) != 0
        _native.check(env._h, L.cz_load_goal_table(env._h, t.goal_table.ctypes.data_as(C.c_void_p), n_rec, 26))
        check_infos("after the goal table came back", env, t, got2)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5, 9: the keyed loop, eager and captured
# ---------------------------------------------------------------------------------------------------------------------------

class KeyedLoop:
    """The multi-task loop on the oracle alone, driven by tasks.task_draw: per step the actions, the step's outputs and the records
    after the step, the reset of the finished envs (auto_reset off) and the keyed task call"""

    def __init__(self, auto_reset, n=19, steps=32):
        self.tables = t = tables_of(n, **dict(COOP, max_steps=6))
        orc = oracle_for(t, auto_reset=1 if auto_reset else 0)
        orc.reset()
        self.rec0 = orc.records.copy()
        pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(17))
        self.steps, words = [], set()
        for _ in range(steps):
            acts = np.ascontiguousarray(pol.act(orc.records), dtype=np.int32)
            out = orc.step(acts)
            if not auto_reset:
                for e in np.nonzero(orc.records[:, soa.W_STATUS] & 1)[0]:
                    oracle_reset(orc, int(e))
            new, refused, chosen = model_call(t, orc.records, None, None, TASK_LIST, LOOP_SEED)
            assert refused == 0
            orc.records[:] = new
            pol.observe_result(orc.records)
            words |= set(new[chosen][:, soa.W_RECIPES].tolist())
            self.steps.append(dict(acts=acts, out=out, after=orc.records.copy()))
        self.episodes, self.words = int(orc.records[:, soa.W_EPISODE].min()), words


@functools.lru_cache(maxsize=None)
def keyed_loop(auto_reset):
    return KeyedLoop(auto_reset)


@pytest.mark.parametrize("auto_reset", [False, True])
def test_keyed_loop(auto_reset):
    s = keyed_loop(auto_reset)
    assert s.episodes >= 4 and len(s.words) == 3, (s.episodes, s.words)
    env = env_of(s.tables, auto_reset=auto_reset)
    try:
        o, b = Outs(env), TaskBufs(env)
        b.list.from_host(TASK_LIST)
        env.reset(return_obs=False)
        for k, st in enumerate(s.steps):
            got = o.step(env, st["acts"])
            if not auto_reset:
                env.reset_device()
            env.set_tasks_device(d_task_list=b.list, seed=LOOP_SEED)
            check_step(f"step {k}", got, st["out"])
            mc.check_records(f"step {k}", strip(env.get_state()), st["after"])
        assert env.set_tasks_refused() == 0
        check_infos("at the end of the loop", env, s.tables, s.steps[-1]["after"])
    finally:
        env.close()


def test_keyed_loop_inside_a_callers_capture():
    s = keyed_loop(False)
    assert int(s.steps[19]["after"][:, soa.W_EPISODE].min()) >= 2
    env = env_of(s.tables, auto_reset=False)
    try:
        o, b = Outs(env), TaskBufs(env)
        info = InfoBufs(env, env.num_envs)
        b.list.from_host(TASK_LIST)
        env.reset(return_obs=False)
        cs = CallerStream(env)
        with cs.capture():                                               # captured, not executed
            env.step_device(o.act, o.buf["obs"], o.buf["rew"], o.buf["term"], o.buf["trunc"])
            env.reset_device()
            env.set_tasks_device(d_task_list=b.list, seed=LOOP_SEED)
            env.infos_device(**info.args(OUTPUTS))
        mc.check_records("capturing changed nothing", strip(env.get_state()), s.rec0)
        for k, st in enumerate(s.steps[:20]):                          # (past the first restarts and task draws)
            o.fill()
            o.act.from_host(st["acts"])
            cs.replay()
            cs.sync()
            check_step(f"replay {k}", o.get(), st["out"])
            mc.check_records(f"replay {k}", strip(env.get_state()), st["after"])
            info.check(f"replay {k}: infos_device", OUTPUTS, tasks.host_infos(s.tables, st["after"]))
        cs.close()
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6: wide tables
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def user_recipes():
    with fresh_user_registry():
        yield


def test_wide_tables(user_recipes):
    n = 21
    t = tables_of(n, mc.LEVEL, mc.META, 4, ["FruitFeast", "PickyBanana", "BreadSnack", "FruitFeast"], "scheme3", max_steps=mc.MAX_STEPS,
                  num_layouts=mc.LAYOUTS)
    assert t.recipe_nodes == soa.MAX_NODES and t.num_goals == rd.NUM_GOALS <= 255
    orc = oracle_for(t)
    orc.reset()
    pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(41))
    for _ in range(60):
        orc.step(pol.act(orc.records), want_obs=False)
        pol.observe_result(orc.records)
    recs = orc.records.copy()
    ids = np.random.default_rng(42).integers(0, 3, (n, 4)).astype(np.uint8)
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    want, refused, chosen = model_call(t, recs, mask, ids)
    assert refused == 0 and want[chosen][:, soa.W_MARKS_HI].any() and (want[chosen] != recs[chosen]).any()
    env = env_of(t)
    try:
        assert env.num_goals == t.num_goals
        b = TaskBufs(env)
        env.set_state(recs)
        b.mask.from_host(mask)
        b.ids.from_host(ids)
        env.set_tasks_device(b.mask, b.ids)
        mc.check_records("wide tables: set_tasks_device", env.get_state(), want)
        check_infos("wide tables: infos_device", env, t, want)
        follow_oracle("wide tables", env, t, want, 8, 43)
    finally:
        env.close()


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_two_nodes_with_one_goal_id(wide):
    """the golden's SharedId recipe on the device: two leaves carry goal id 2, the entry is the LATER node's - the one whose `counts`
    bit k_infos reads - in states where the earlier leaf is marked and the later one is not"""
    from tasks_common import golden, shared_id_recipe
    n = 24
    with fresh_user_registry():
        if not wide:
            rd.RECIPE_STORE.clear()                                     # SharedId alone: four nodes, compact tables
        rd.register_recipe(shared_id_recipe(golden()["shared_id"]["nodes"]), "SharedId")
        if wide:
            t = tables_of(n, mc.LEVEL, mc.META, 4, ["SharedId", "PickyBanana", "BreadSnack", "SharedId"], "scheme3", max_steps=mc.MAX_STEPS,
                          num_layouts=mc.LAYOUTS)
        else:
            t = tables_of(n, "coop_test", "example", 2, ["SharedId", "SharedId"], "scheme3", max_steps=200, num_layouts=4)
        assert (t.recipe_nodes == soa.MAX_NODES) == wide
        r = t.book_names.index("SharedId")
        assert t.goal_table[r, :4].tolist() == [0, 1, 2, 2]
        orc = oracle_for(t)
        orc.reset()
        pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(7))
        for _ in range(120):
            orc.step(pol.act(orc.records), want_obs=False)
            pol.observe_result(orc.records)
        recs = orc.records.copy()
        marks = np.array([tasks.slot_marks(rec, 0, wide) for rec in recs])
        early_only = ((marks >> 2) & 1 == 1) & ((marks >> 3) & 1 == 0)
        goal = tasks.host_infos(t, recs)[0]
        assert early_only.sum() >= 5 and (goal[early_only, 0, 2] == 1).all(), "the earlier leaf marked, the later not: the entry stays 1"
        env = env_of(t)
        try:
            env.set_state(recs)
            check_infos("SharedId: infos_device", env, t, recs)
            b = TaskBufs(env)
            b.mask.from_host(np.ones(n, np.uint8))
            b.ids.from_host(np.ascontiguousarray(t.recipe_ids))
            env.set_tasks_device(b.mask, b.ids)                         # the same recipes again: the marks from scratch are the marks
            mc.check_records("SharedId: set_tasks_device with the env's own ids", env.get_state(), recs)
        finally:
            env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7: the lean kernel
# ---------------------------------------------------------------------------------------------------------------------------

def test_lean_step_after_a_reassignment():
    n = 64
    t = tables_of(n, "coop_test", "example", 2, TWO, "scheme3", max_steps=400, num_layouts=8)
    env = env_of(t)
    try:
        env.reset(return_obs=False)
        o = Outs(env)
        orc = follow_oracle("before the reassignment", env, t, strip(env.get_state()), 6, 50, outs=o, lean=1)
        ids = np.random.default_rng(51).integers(0, len(t.book_names), (n, 4)).astype(np.uint8)
        want, refused, _ = model_call(t, orc.records, np.ones(n), ids)
        assert refused == 0
        b = TaskBufs(env)
        b.mask.from_host(np.ones(n, np.uint8))
        b.ids.from_host(ids)
        env.set_tasks_device(b.mask, b.ids)
        mc.check_records("set_tasks_device", strip(env.get_state()), want)
        follow_oracle("after the reassignment", env, t, want, 20, 52, outs=o, lean=1)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8: the scripted partner plays the new recipes
# ---------------------------------------------------------------------------------------------------------------------------

def test_partner_follows_the_reassignment():
    t, recs, ids = crowded_state()
    n = t.num_envs
    env = env_of(t)
    try:
        env.reset(return_obs=False)
        orc = oracle_for(t)
        orc.reset()
        pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(5))
        o = Outs(env, skip=("obs",))
        for _ in range(20):
            acts = np.ascontiguousarray(pol.act(orc.records), dtype=np.int32)
            check_step("step", o.step(env, acts), orc.step(acts))
            pol.observe_result(orc.records)
        before = partner.host_partner(t.dims, t.layouts, orc.records, book_of(t))
        want, refused, _ = model_call(t, orc.records, np.ones(n), ids)
        after = partner.host_partner(t.dims, t.layouts, want, book_of(t))
        assert refused == 0 and any((x != y).any() for x, y in zip(before, after)), "the new recipes change the partner's answers"
        b, pb = TaskBufs(env), PartnerBufs(env, n)
        b.mask.from_host(np.ones(n, np.uint8))
        b.ids.from_host(ids)
        env.set_tasks_device(b.mask, b.ids)
        env.partner_device(**pb.args(PARTNER_OUTPUTS))
        env.sync()
        pb.check("partner_device after set_tasks_device", PARTNER_OUTPUTS, after)
        assert env.partner_bad_recipes() == 0
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 10: shards
# ---------------------------------------------------------------------------------------------------------------------------

def test_unequal_shards_equal_one_handle(monkeypatch):
    from cooking_zoo_amd import sharded
    n, A = 67, 2                                                        # 37 + 30
    t = tables_of(n, **dict(COOP, max_steps=6))
    monkeypatch.setattr(sharded, "plan_shards", lambda num_envs, world_size, k: [(0, 37), (37, 30)])
    many = sharded.ShardedVecEnv(n, tables=t, device_ids=[0, 0], auto_reset=False, level=None, meta_file=None, num_agents=None, max_steps=None,
                                 recipes=None)
    try:
        assert [c for _, c in many.ranges] == [37, 30] and many.num_goals == 26
        orc = oracle_for(t, auto_reset=0)
        orc.reset()
        many.reset(return_obs=False)
        act, rew, term, trunc = many.alloc((A,), np.int32), many.alloc((A,), np.float64), many.alloc((A,), np.uint8), many.alloc((A,), np.uint8)
        G = many.num_goals
        goal8, goal32, done = many.alloc((A, G), np.uint8), many.alloc((A, G), np.float32), many.alloc((A,), np.uint8)
        task, tt = many.alloc((A,), np.int32), many.alloc((), np.int32)
        lists = [env.alloc((len(TASK_LIST), 4), np.uint8) for env in many.shards]
        for l in lists:
            l.from_host(TASK_LIST)
        pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(17))
        words = set()
        for k in range(24):
            acts = np.ascontiguousarray(pol.act(orc.records), dtype=np.int32)
            _obs, wr, wt, wu = orc.step(acts, want_obs=False)
            for e in np.nonzero(orc.records[:, soa.W_STATUS] & 1)[0]:
                oracle_reset(orc, int(e))
            new, refused, chosen = model_call(t, orc.records, None, None, TASK_LIST, LOOP_SEED)
            orc.records[:] = new
            pol.observe_result(orc.records)
            words |= set(new[chosen][:, soa.W_RECIPES].tolist())
            act.from_host(acts)
            many.step_device(act, None, rew, term, trunc)
            many.reset_device()
            many.set_tasks_device(d_task_list=lists, seed=LOOP_SEED)
            many.infos_device(goal8, goal32, done, task, tt)
            check_step(f"step {k}", (None, rew.to_host(), term.to_host(), trunc.to_host()), (None, wr, wt, wu))
            mc.check_records(f"step {k}", strip(many.get_state()), orc.records)
            wg, wd, wk, wtt = tasks.host_infos(t, orc.records)
            for name, got, want in (("goal8", goal8, wg), ("goal32", goal32, wg.astype(np.float32)), ("recipe_done", done, wd), ("task", task, wk),
                                    ("t", tt, wtt)):
                mc.check_equal(f"step {k}: {name}", got.to_host(), want)
        assert len(words) == 3 and many.set_tasks_refused() == 0
        # the host conveniences: per-env names, cut along the env axis
        names = [[t.book_names[(e + r) % len(t.book_names)] for r in range(A)] for e in range(n)]
        mask = np.arange(n) % 2
        assert many.set_tasks(names, mask) == 0
        idx = np.array([[(e + r) % len(t.book_names) for r in range(A)] for e in range(n)])
        want, _, chosen = model_call(t, orc.records, mask, np.concatenate([idx, np.full((n, 2), 0xFF)], axis=1).astype(np.uint8))
        mc.check_records("set_tasks", strip(many.get_state()), want)
        mc.check_equal("infos()['task']", many.infos()["task"], tasks.host_infos(t, want)[2])
        for env, (lo, c) in zip(many.shards, many.ranges):
            ch = chosen[lo:lo + c]
            assert np.array_equal(env.recipe_ids[ch][:, :A], idx[lo:lo + c][ch]), "recipe_ids follows a host-side set_tasks"
    finally:
        many.close()
