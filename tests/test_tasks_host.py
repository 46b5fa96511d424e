"""CPU: the host definition of the task calls (cooking_zoo_amd/tasks.py) against what the unmodified reference computes
(tests/golden/tasks_ref.json.gz, tools/gen_tasks_golden.py) and against the C oracle, the goal table, the keyed draw, and the C-ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa, tasks
from cooking_zoo_amd.cooking_book import recipe_drawer as rd
from cooking_zoo_amd.cooking_book.recipe_drawer import RECIPES
from tasks_common import fresh_user_registry, golden, golden_tables, ids_rows, shared_id_recipe, switch_oracle
from vec_common import bits, oracle_for, tables_of

NEW_SYMBOLS = ["cz_load_goal_table", "cz_num_goals", "cz_set_tasks_device", "cz_set_tasks_refused", "cz_infos_device"]


def test_golden_book_is_the_default_book():
    doc = golden()
    assert doc["recipe_names"] == list(RECIPES.keys()) and doc["num_goals"] == rd.DEFAULT_NUM_GOALS == 26
    c = doc["census"]
    assert c["roots_marked"] > 0 and c["switch_presatisfied"] > 0 and c["switch_completed"] > 0
    assert all(c["info_keys"][k] > 0 for k in ("recipe_done", "task", "t"))
    # every node of every recipe a chosen level can complete is seen marked and unmarked
    assert any("MashedCarrotBanana" in names for names in c["completable"].values())
    for names in c["completable"].values():
        for name in names:
            for j in range(len(RECIPES[name]().node_list)):
                for m in (0, 1):
                    assert c["seen"].get(f"{name}:{j}:{m}", 0) > 0, (name, j, m)
    # ... and the stored states hold MashedCarrotBanana with its leaves, then its plate, then its root marked (the scripted episode)
    r = doc["recipe_names"].index("MashedCarrotBanana")
    stored = {st["marks"][r] for ep in doc["episodes"] for st in ep["states"]}
    assert {0b0100, 0b1100, 0b1110, 0b1111} <= stored, sorted(stored)


def test_golden_marks_and_goals():
    """host_set_tasks + host_infos reproduce every stored mark word and goal vector: every recipe of the book on every stored state"""
    doc = golden()
    names = doc["recipe_names"]
    checked = marked = 0
    for ep in doc["episodes"]:
        t = golden_tables(ep, ep["states"][0]["record"])
        A = t.dims.A
        own = [names.index(r) for r in ep["recipes"]]
        t_own = golden_tables(ep, ep["states"][0]["record"], R=len(own))
        for st in ep["states"]:
            rec = np.array(st["record"], dtype=np.uint32)
            ctx = f"{ep['set']} step {st['step']}"
            # the env's own recipes: the record the reference's own graphs gave, word for word
            got, refused = tasks.host_set_tasks(t_own, rec, [True], recipe_ids=ids_rows([own]))
            assert not refused.any() and np.array_equal(got[0], rec), f"{ctx}: the env's own recipes"
            for first in range(0, len(names), A):                       # every name of the book, A recipe slots at a time
                chunk = [(first + k) % len(names) for k in range(A)]
                scrambled = rec.copy()
                scrambled[soa.W_MARKS] = 0xDEADBEEF
                got, refused = tasks.host_set_tasks(t, scrambled, [True], recipe_ids=ids_rows([chunk]))
                assert not refused.any()
                rest = np.ones(t.dims.RW, dtype=bool)
                rest[[soa.W_MARKS, soa.W_RECIPES]] = False
                assert np.array_equal(got[0][rest], rec[rest]), f"{ctx}: a word other than the marks and the ids changed"
                goal, done, task, tt = tasks.host_infos(t, got)
                assert tt[0] == st["step"]
                for k, r in enumerate(chunk):
                    assert tasks.slot_marks(got[0], k, False) == st["marks"][r], f"{ctx}: marks of {names[r]}"
                    assert goal[0, k].tolist() == st["goals"][r], f"{ctx}: goal vector of {names[r]}"
                    assert done[0, k] == (st["marks"][r] & 1) and task[0, k] == r
                    checked += 1
                    marked += bool(st["marks"][r])
    assert checked > 1000 and marked > 200, (checked, marked)


def test_golden_shared_goal_id():
    """two nodes with one id_num: the goal entry is the LATER node's, as recipe.py:38-39 overwrites it"""
    doc = golden()
    sh = doc["shared_id"]
    recipe = shared_id_recipe(sh["nodes"])
    assert sh["states"]
    for s in sh["states"]:
        ep = doc["episodes"][s["episode"]]
        t = golden_tables(ep, ep["states"][0]["record"], graphs=[recipe], num_goals=sh["num_goals"], R=1)
        rec = np.array(ep["states"][s["state"]]["record"], dtype=np.uint32)
        got, _ = tasks.host_set_tasks(t, rec, [True], recipe_ids=ids_rows([[0]]))
        m = tasks.slot_marks(got[0], 0, False)
        assert m == s["marks"] and (m >> 2 & 1) and not (m >> 3 & 1)
        goal, done, task, _t = tasks.host_infos(t, got)
        assert goal[0, 0].tolist() == s["goals"] and s["goals"][2] == 1
        assert not goal[0, 1:].any() and task[0, 0] == 0


@pytest.mark.parametrize("k", range(4))
def test_golden_switches(k):
    """the C oracle, stepped from host_set_tasks' record, reproduces the reference's switched trajectory step for step"""
    doc = golden()
    names = doc["recipe_names"]
    ep = doc["switches"][k]
    t = golden_tables(ep, ep["initial_record"], R=len(ep["new_recipes"]))
    new = [names.index(r) for r in ep["new_recipes"]]
    before, after = np.array(ep["record_before"], dtype=np.uint32), np.array(ep["record_after"], dtype=np.uint32)
    got, refused = tasks.host_set_tasks(t, before, [True], recipe_ids=ids_rows([new]))
    assert not refused.any() and np.array_equal(got[0], after), f"{ep['set']}: the record after the switch"
    assert [tasks.slot_marks(after, r, False) for r in range(len(new))] == ep["marks_after"]
    orc, rec, A = switch_oracle(ep), got[0].copy(), t.dims.A
    completed = False
    for i, st in enumerate(ep["steps"]):
        ctx = f"{ep['set']} step {i} after the switch"
        err, _obs, rew, term, trunc = orc.step_env(rec, st["actions"])
        assert err == 0, f"{ctx}: oracle error {err}"
        assert np.array_equal(bits(rew), bits([float.fromhex(x) for x in st["rewards"]])), f"{ctx}: rewards"
        assert term.tolist() == st["terms"] and trunc.tolist() == st["truncs"], f"{ctx}: flags"
        a, b = rec.copy(), np.array(st["record"], dtype=np.uint32)
        a[soa.W_STATUS] = b[soa.W_STATUS] = 0                           # (the reference has no status word)
        assert np.array_equal(a, b), f"{ctx}: record"
        goal, done, task, tt = tasks.host_infos(t, rec)
        assert done[0].tolist() == st["recipe_done"][:A] and task[0].tolist() == st["task"][:A] == new[:A], f"{ctx}: infos"
        assert goal[0].tolist() == st["goal_vector"], f"{ctx}: goal vectors"
        assert tt[0] == ep["switch_step"] + i + 1
        completed = completed or any(st["recipe_done"])
    assert k != 0 or (completed and any(ep["marks_after"])), "the late coop switch finds a node satisfied and completes the new recipe"


def test_fresh_records_against_the_oracle():
    """host_set_tasks on a fresh world equals czo_reset_env of an oracle built with those recipe ids: all 8 x 8 recipe pairs on
    coop_test - a route that does not pass through partner.recipe_marks"""
    n = len(RECIPES)
    assert n == 8
    pairs = np.array([(a, b) for a in range(n) for b in range(n)])
    base = tables_of(len(pairs), "coop_test", "example", 2, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=30, num_layouts=3)
    orc = oracle_for(base)
    orc.reset()
    want_t = tables_of(len(pairs), "coop_test", "example", 2, pairs, "scheme3", max_steps=30, num_layouts=3)
    want = oracle_for(want_t)
    want.reset()
    got, refused = tasks.host_set_tasks(base, orc.records, np.ones(len(pairs), bool), recipe_ids=ids_rows(pairs))
    assert not refused.any()
    assert np.array_equal(got, want.records)
    assert (got[:, soa.W_RECIPES] != orc.records[:, soa.W_RECIPES]).sum() == len(pairs) - 1
    # slots >= R are forced to 0xFF whatever was passed, an id past the table refuses the env, an env not chosen stays
    ids = ids_rows(pairs)
    ids[:, 2:] = 3
    ids[5, 1] = n
    chosen = np.ones(len(pairs), bool)
    chosen[7] = False
    got2, refused2 = tasks.host_set_tasks(base, orc.records, chosen, recipe_ids=ids)
    assert refused2.tolist() == [e == 5 for e in range(len(pairs))]
    keep = np.array([e in (5, 7) for e in range(len(pairs))])
    assert np.array_equal(got2[keep], orc.records[keep]) and np.array_equal(got2[~keep], want.records[~keep])
    with pytest.raises(ValueError):
        tasks.host_set_tasks(base, orc.records, chosen)
    with pytest.raises(ValueError):
        tasks.host_set_tasks(base, orc.records, chosen, task_list=np.zeros((0, 4), np.uint8))


@pytest.fixture
def user_recipes():
    with fresh_user_registry():
        yield


def test_goal_table_of_the_default_book():
    t = tables_of(2, "coop_test", "example", 2, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=30, num_layouts=2)
    assert t.num_goals == rd.DEFAULT_NUM_GOALS == 26 and t.goal_table.shape == (len(t.book_names), soa.MAX_NODES) and t.goal_table.dtype == np.uint8
    for r, g in enumerate(t.recipe_graphs):
        n = len(g.node_list)
        assert t.goal_table[r, :n].tolist() == [node.id_num for node in g.node_list] and (t.goal_table[r, n:] == 0xFF).all()
        # the node the kernels take for goal id `id` - the `counts` bit of Recipe.flatten - is the last of node_list that carries it
        last = {node.id_num: j for j, node in enumerate(g.node_list)}
        assert [j for j in range(n) if g.flatten()[1 + j] >> 24 & 1] == sorted(last.values())
    graphs = t.recipe_graphs
    top = max(node.id_num for g in graphs for node in g.node_list)
    with pytest.raises(ValueError):
        tasks.goal_table(graphs, top)                                   # an id >= num_goals
    with pytest.raises(ValueError):
        tasks.goal_table(graphs, 256)
    assert tasks.goal_table(graphs, top + 1).shape == t.goal_table.shape


def test_goal_table_of_a_user_registry(user_recipes):
    t = tables_of(2, "coop_test", "example", 2, ["FruitFeast", "BreadSnack"], "scheme3", max_steps=30, num_layouts=2)
    assert t.recipe_nodes == soa.MAX_NODES, "the fixture book has a graph of more than 8 nodes: wide tables"
    assert t.num_goals == rd.NUM_GOALS == tasks.current_num_goals() and t.num_goals != rd.DEFAULT_NUM_GOALS
    assert t.goal_table.shape == (3, soa.MAX_NODES) and int(t.goal_table[t.goal_table != 0xFF].max()) < t.num_goals
    # wide packing: 16 bits per recipe, slots 2 and 3 in word 7
    assert tasks.pack_marks([0x8001, 0x0102, 0x4004, 0xFFFF], True) == (0x01028001, 0xFFFF4004)
    assert tasks.pack_marks([0x81, 0x12, 0x44, 0xFF], False) == (0xFF441281, 0)
    rec = np.zeros(t.dims.RW, np.uint32)
    rec[soa.W_MARKS], rec[soa.W_MARKS_HI] = 0x01028001, 0xFFFF4004
    assert [tasks.slot_marks(rec, r, True) for r in range(4)] == [0x8001, 0x0102, 0x4004, 0xFFFF]
    orc = oracle_for(t)
    orc.reset()
    got, _ = tasks.host_set_tasks(t, orc.records, [True, True], recipe_ids=ids_rows([[2, 0], [1, 1]]))
    t2 = tables_of(2, "coop_test", "example", 2, np.array([[2, 0], [1, 1]]), "scheme3", max_steps=30, num_layouts=2)
    want = oracle_for(t2)
    want.reset()
    assert np.array_equal(got, want.records)


def test_goal_ids_beyond_a_byte_leave_the_batch_without_a_goal_table():
    """the registry's id counter never goes back: a batch whose ids have outgrown the table's byte is still made, without the table"""
    with fresh_user_registry(first_id=250):
        t = tables_of(2, "coop_test", "example", 2, ["FruitFeast", "BreadSnack"], "scheme3", max_steps=30, num_layouts=2)
        assert t.num_goals == rd.NUM_GOALS > 255 and t.goal_table is None and t.recipe_table.shape[0] == 3
        with pytest.raises(ValueError):
            tasks.goal_table(t.recipe_graphs, t.num_goals)


def test_a_node_id_outside_the_goals_is_not_hidden(monkeypatch):
    """only `more than 255 goals` leaves a batch without a goal table: a node id >= num_goals is a malformed book and raises"""
    monkeypatch.setattr(tasks, "current_num_goals", lambda: 25)          # (the book's graphs carry ids up to 25)
    with pytest.raises(ValueError):
        tables_of(2, "coop_test", "example", 2, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", max_steps=30, num_layouts=2)


def test_keyed_draw():
    from oracle_binding import load_lib
    czo = load_lib()
    K, seed = 3, 5
    seen = set()
    for e in range(67):
        for ep in range(4):
            u = czo.czo_spawn_uniform(seed, e, ep << 32, tasks.TASK_KEY, 0)
            want = min(int(u * K), K - 1)
            assert tasks.task_draw(seed, e, ep, K) == want
            assert tasks.task_draw(seed, e, ep, K, uniform=lambda s, g, p, t, a, d: czo.czo_spawn_uniform(s, g, (p << 32) | t, a, d)) == want
            seen.add((ep, want))
    assert seen == {(ep, k) for ep in range(4) for k in range(K)}, "every task occurs in every episode"
    assert tasks.task_draw(seed, 9, 2, 1) == 0
    with pytest.raises(ValueError):
        tasks.task_draw(seed, 0, 0, 0)


def test_abi_and_bindings(repo_root):
    hdr = open(os.path.join(repo_root, "include", "cookingzoo.h")).read()
    assert re.search(r"^#define\s+CZ_ABI_VERSION\s+10\b", hdr, flags=re.M), "additions only: the ABI number stays"
    capture = hdr[hdr.index("STREAM CAPTURE"):]
    capture = capture[:capture.index("*/")]
    assert "cz_set_tasks_device" in capture and "cz_infos_device" in capture
    assert "whole table" in hdr[hdr.index("cz_set_tasks_device:"):], "the header says why any id of the table suits every step kernel"
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    want = {"cz_load_goal_table": (ctypes.c_int, [vp, vp, i32, i32]), "cz_num_goals": (i32, [vp]),
            "cz_set_tasks_device": (ctypes.c_int, [vp, vp, vp, vp, i32, u64]), "cz_set_tasks_refused": (i64, [vp]),
            "cz_infos_device": (ctypes.c_int, [vp, i64, i64, vp, vp, vp, vp, vp])}
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared"
        assert bound[name] == want[name], name
    assert set(NEW_SYMBOLS) <= set(_native.ADDED_SYMBOLS)
    lib = _native.lib()
    assert lib.cz_num_goals(None) == -1 and lib.cz_set_tasks_refused(None) == -1
    assert lib.cz_set_tasks_device(None, None, None, None, 0, 0) != 0 and lib.cz_infos_device(None, 0, 0, None, None, None, None, None) != 0
    assert lib.cz_load_goal_table(None, None, 0, 0) != 0
