"""The scripted partner's definition on the host (cooking_zoo_amd/partner.py), no device: against what a fresh, unmodified
`CookingAgent` returned (tests/golden/partner_ref.json.gz, tools/gen_partner_golden.py), against a second route over the object
view of `symbolic.materialize`, on hand-built records for what replay does not reach, and on the known-answer trace."""
import numpy as np
import pytest

from cooking_zoo_amd import partner, soa
from cooking_zoo_amd.cooking_book import recipe_drawer
from cooking_zoo_amd.cooking_book.recipe import Recipe, RecipeNode
from cooking_zoo_amd.cooking_world.constants import BlenderFoodStates, ChopFoodStates
from grid_common import CASES, checkpoints
from partner_common import KAT_ACTIONS, KAT_REWARD, book_of, golden, golden_layout, kat_tables, plain_partner
from vec_common import oracle_for

CUT, BLEND, COUNTER, FLOOR = (soa.STATIC_CLASSES.index(n) for n in ("Cutboard", "Blender", "Counter", "Floor"))


def test_golden_answers_exact():
    """every stored answer: action, target and walk-call count where the reference returned, RAISES exactly where it raised"""
    doc = golden()
    names = doc["recipe_names"]
    assert names == list(recipe_drawer.RECIPES)
    n, status, raises, levels = 0, set(), set(), set()
    for ep in doc["episodes"]:
        dims, layout = soa.Dims(*ep["dims"]), golden_layout(ep)
        levels.add((ep["level"], ep["scheme"]))
        for st in ep["states"]:
            rec = np.array(st["record"], dtype=np.uint32)
            for ans in st["answers"]:
                a, r = ans[0], ans[1]
                got = partner.agent_answer(dims, layout, rec, recipe_drawer.RECIPES[names[r]](), a)
                ctx = f"{ep['set']} step {st['step']} agent {a} {names[r]}: stored {ans[2:]}, host model {got}"
                if isinstance(ans[2], str):
                    assert got.status == partner.RAISES and got.action == 0 and got.target == partner.NO_TARGET, ctx
                    raises.add(ans[2])
                else:
                    action, walks, x, y = ans[2:]
                    assert got.status != partner.RAISES and got.action == action and got.walks == walks, ctx
                    assert (got.last_walk or partner.NO_TARGET) == (x, y), ctx
                    assert got.target == ((x, y) if got.status == partner.WALK else partner.NO_TARGET), ctx
                    assert (got.status == partner.WALK) == (walks > 0 and not (got.tags[-1] == "no_child")), ctx
                status.add(got.status)
                n += 1
    assert n >= 5000 and status == {partner.DONE, partner.WALK, partner.IDLE, partner.RAISES}
    assert raises >= {"IndexError", "TypeError"}
    assert levels == {("coop_test", "scheme3"), ("switch_test", "scheme1"), ("switch_test", "scheme3"), ("crowded_6x5", "scheme3"), ("dense_8x8", "scheme3")}


@pytest.mark.parametrize("name", list(CASES))
def test_second_route(name):
    """the host model against the plain model over the symbolic view, at reset and at the checkpoints of an oracle trajectory under
    the state-aware policy, every env, agent and recipe name of the book on every state - on the two levels of more than 256 cells
    (20 x 20, 32 x 32: a fill in plain Python takes milliseconds) two envs per state and every third (recipe, env, state)
    combination, which still reaches every recipe name on each of those levels"""
    tables, points = checkpoints(name, 6)
    dims = tables.dims
    book = book_of(tables)
    orc = oracle_for(tables)
    orc.reset()
    big = dims.C > 256
    seen, names_seen = set(), set()
    for k, recs in enumerate([orc.records.copy()] + list(points)):
        for e, rec in enumerate(recs[:2] if big else recs):
            layout = tables.layouts[int(rec[soa.W_LAYOUT])]
            for r, recipe in enumerate(book):
                if big and (r + e + k) % 3:
                    continue
                for a in range(dims.A):
                    got = partner.agent_answer(dims, layout, rec, recipe, a)
                    want = plain_partner(dims, layout, rec, recipe, a)
                    assert (got.action, got.target, got.status) == want, (
                        f"{name} point {k} env {e} agent {a} {tables.book_names[r]}: host model {got}, second route {want}")
                    seen.add(got.status)
                    names_seen.add(r)
    assert partner.WALK in seen
    if big:
        assert names_seen == set(range(len(book))), "the thinning left a recipe name out"


def test_host_partner_shapes_masks_and_absent():
    tables, points = checkpoints("coop_test", 6, True)
    dims, recs = tables.dims, points[-1]
    book = book_of(tables)
    assert ((recs[:, soa.W_STATUS] >> partner.SPAWN_GONE0) & 0xF).any(), "no checkpoint has a despawned agent"
    act, tg, st = partner.host_partner(dims, tables.layouts, recs, book)
    assert act.shape == st.shape == (6, 2) and tg.shape == (6, 2, 2) and act.dtype == tg.dtype == np.int32 and st.dtype == np.uint8
    gone = ((recs[:, soa.W_STATUS, None] >> (partner.SPAWN_GONE0 + np.arange(2))) & 1) != 0
    assert ((st == partner.ABSENT) == gone).all() and (act[gone] == 0).all() and (tg[gone] == -1).all()
    a1, t1, s1 = partner.host_partner(dims, tables.layouts, recs, book, agents=0b10)
    assert np.array_equal(a1[:, 1], act[:, 1]) and (a1[:, 0] == 0).all() and (s1[:, 0] == partner.IDLE).all() and (t1[:, 0] == -1).all()
    idx = np.full((6, 2), 99, np.int64)
    assert (partner.host_partner(dims, tables.layouts, recs, book, recipe_idx=idx)[2][~gone] == partner.IDLE).all(), "an index outside the table"
    unused = recs.copy()
    unused[:, soa.W_RECIPES] |= 0xFF00
    assert (partner.host_partner(dims, tables.layouts, unused, book)[2][:, 1][~gone[:, 1]] == partner.DONE).all(), "an unused recipe slot"
    for bad in (0, 4):
        with pytest.raises(ValueError):
            partner.host_partner(dims, tables.layouts, recs, book, agents=bad)
    one = partner.host_partner(dims, tables.layouts, recs[0], book)
    assert one[0].shape == (2,) and np.array_equal(one[0], act[0])


def test_rank_table_is_the_static_list_order():
    differs = set()
    for name in CASES:
        tables, _ = checkpoints(name, 6)
        for layout in tables.layouts:
            rank = partner.rank_table(layout)
            assert rank.dtype == np.uint16 and rank.shape == (layout.width * layout.height,)
            for cls, cells in layout.static_lists.items():
                assert [int(rank[c]) for c in cells] == list(range(len(cells))), f"{name} {cls}"
                if sorted(cells) != list(cells):
                    differs.add(name)
    assert "coop_test" in differs, "no list of coop_test differs from cell order"


# ---------------------------------------------------------------------------------------------------------------------------
# hand-built records
# ---------------------------------------------------------------------------------------------------------------------------

def coop_world():
    """one coop_test record at reset, its layout and dims"""
    tables, _ = checkpoints("coop_test", 6)
    orc = oracle_for(tables)
    orc.reset()
    rec = orc.records[0].copy()
    return tables, tables.layouts[int(rec[soa.W_LAYOUT])], rec


def slots_of(dims, rec, cls):
    return [s for s in range(dims.D) if soa.unpack_dyn0(rec[dims.dyn0_word0 + s])[2:] == (cls, soa.DYN_ALIVE | soa.DYN_FREE)
            or (soa.unpack_dyn0(rec[dims.dyn0_word0 + s])[2] == cls and soa.unpack_dyn0(rec[dims.dyn0_word0 + s])[3] & soa.DYN_ALIVE)]


def set_flags(dims, rec, slot, flags):
    x, y, c, f = soa.unpack_dyn0(rec[dims.dyn0_word0 + slot])
    rec[dims.dyn0_word0 + slot] = soa.pack_dyn0(x, y, c, f | flags)


def leaf(name, *conditions):
    return RecipeNode(root_type=name, id_num=0, name=name, conditions=list(conditions))


def test_completed_recipe_is_done():
    tables, layout, rec = coop_world()
    dims = tables.dims
    recipe = Recipe(leaf("Tomato", ("chop_state", ChopFoodStates.CHOPPED)), 1)
    assert partner.agent_answer(dims, layout, rec, recipe, 0).status == partner.WALK
    set_flags(dims, rec, slots_of(dims, rec, soa.TOMATO)[0], soa.DYN_CHOPPED)
    got = partner.agent_answer(dims, layout, rec, recipe, 0)
    assert (got.action, got.target, got.status, got.walks) == (0, partner.NO_TARGET, partner.DONE, 0)
    assert plain_partner(dims, layout, rec, recipe, 0) == (0, partner.NO_TARGET, partner.DONE)


def test_first_unmet_condition_wants_fresh():
    """base_agent.py:153: no appliance makes anything FRESH: 0 from the condition branch, the contains branch of a leaf idles"""
    tables, layout, rec = coop_world()
    dims = tables.dims
    for s in slots_of(dims, rec, soa.TOMATO):
        set_flags(dims, rec, s, soa.DYN_CHOPPED)
    recipe = Recipe(leaf("Tomato", ("chop_state", ChopFoodStates.FRESH)), 1)
    got = partner.agent_answer(dims, layout, rec, recipe, 0)
    assert (got.action, got.status, got.walks) == (0, partner.IDLE, 0) and got.tags[0] == "no_appliance", got
    assert plain_partner(dims, layout, rec, recipe, 0) == (0, partner.NO_TARGET, partner.IDLE)


def test_two_conditions_in_both_orders():
    """the first unmet condition in the NODE'S order chooses the appliance: the accept mask of the step kernels cannot tell"""
    tables, layout, rec = coop_world()
    dims = tables.dims
    ch, ma = ("chop_state", ChopFoodStates.CHOPPED), ("blend_state", BlenderFoodStates.MASHED)
    carrot = slots_of(dims, rec, soa.CARROT)[0]
    x, y, _o, _h = soa.unpack_agent(rec[soa.AGENT_WORD0 + 1])
    rec[soa.AGENT_WORD0 + 1] = soa.pack_agent(x, y, 1, carrot)                       # the carrot in agent 1's hands
    rec[dims.dyn0_word0 + carrot] = soa.pack_dyn0(x, y, soa.CARROT, soa.DYN_ALIVE)
    a = partner.agent_answer(dims, layout, rec, Recipe(leaf("Carrot", ch, ma), 1), 1)
    b = partner.agent_answer(dims, layout, rec, Recipe(leaf("Carrot", ma, ch), 1), 1)
    assert a.tags == b.tags == ("held_to_appliance",) and a.status == b.status == partner.WALK, (a, b)
    cells = soa.record_cells(dims, rec) & soa.CELL_TYPE_MASK
    kind = lambda ans: int(cells[ans.target[1] * dims.W + ans.target[0]])
    assert (kind(a), kind(b)) == (CUT, BLEND), (a, b)
    for recipe, want in ((Recipe(leaf("Carrot", ch, ma), 1), a), (Recipe(leaf("Carrot", ma, ch), 1), b)):
        assert plain_partner(dims, layout, rec, recipe, 1) == (want.action, want.target, want.status)
    rows = partner.partner_rows([Recipe(leaf("Carrot", ch, ma), 1), Recipe(leaf("Carrot", ma, ch), 1)])
    assert rows.shape == (2, partner.ROW_WORDS) and rows[0, 2] == (0 | 1 << 1) | (1 | 2 << 1) << 4 and rows[1, 2] == (1 | 2 << 1) | (0 | 1 << 1) << 4
    assert Recipe(leaf("Carrot", ch, ma), 1).flatten()[1] == Recipe(leaf("Carrot", ma, ch), 1).flatten()[1], "the step kernels' word tells them apart"


def test_two_walks_in_one_step():
    """an unmet condition whose walk returns 0 (the nearest Plate lies in a corner no floor touches), then the contains branch
    walks.  (A Plate has no chop_state: the condition stays unmet - a deviation, the reference raises - and the Cutboard sequence
    fetches the Plate.)"""
    tables, layout, rec = coop_world()
    dims = tables.dims
    W, H = dims.W, dims.H
    plate = RecipeNode(root_type="Plate", id_num=1, name="Plate", conditions=[("chop_state", ChopFoodStates.CHOPPED)], contains=[leaf("Lettuce")])
    recipe = Recipe(plate, 2)
    cells = soa.record_cells(dims, rec) & soa.CELL_TYPE_MASK
    assert cells[(H - 1) * W + W - 1] == COUNTER and cells[(H - 2) * W + W - 2] == FLOOR and cells[(H - 2) * W + W - 1] == COUNTER
    _x, _y, o, h = soa.unpack_agent(rec[soa.AGENT_WORD0 + 1])
    rec[soa.AGENT_WORD0 + 1] = soa.pack_agent(W - 2, H - 2, o, h)                    # agent 1 next to the corner
    p0, p1 = slots_of(dims, rec, soa.PLATE)[:2]
    rec[dims.dyn0_word0 + p0] = soa.pack_dyn0(W - 1, H - 1, soa.PLATE, soa.DYN_ALIVE | soa.DYN_FREE)       # the corner: no floor next to it
    rec[dims.dyn0_word0 + slots_of(dims, rec, soa.LETTUCE)[0]] = soa.pack_dyn0(W - 1, H - 2, soa.LETTUCE, soa.DYN_ALIVE | soa.DYN_FREE)
    got = partner.agent_answer(dims, layout, rec, recipe, 1)
    assert got.walks == 2 and got.tags == ("fetch", "to_child"), got
    assert (got.action, got.target, got.status) == (2, (W - 1, H - 2), partner.WALK), got
    assert plain_partner(dims, layout, rec, recipe, 1) == (got.action, got.target, got.status)


def test_a_node_class_without_objects_raises():
    """a node whose class is neither static nor dynamic ("Agent"): the batch has no such objects, the status is RAISES; the table
    row carries the class code 255"""
    tables, layout, rec = coop_world()
    recipe = Recipe(leaf("Agent"), 1)
    got = partner.agent_answer(tables.dims, layout, rec, recipe, 0)
    assert (got.action, got.target, got.status, got.walks) == (0, partner.NO_TARGET, partner.RAISES, 0) and got.tags == ("IndexError",)
    assert partner.partner_rows([recipe])[0, 1] & 0xFF == soa.NODE_CLS_NONE


def test_known_answer_trace():
    """a fresh decision per step from kat_c3's initial record, then the oracle's step, 30 times: the pinned actions, and the 30th
    step terminates with 19.9875"""
    tables, rec0 = kat_tables(1)
    dims = tables.dims
    orc = oracle_for(tables)
    orc.reset()
    orc.records[0] = rec0
    book = book_of(tables)
    acts = ""
    for t in range(30):
        a, _tg, st = partner.host_partner(dims, tables.layouts, orc.records, book)
        acts += str(int(a[0, 0]))
        out = orc.step(a.astype(np.int32), want_obs=False)
        if t < 29:
            assert not (orc.records[0, soa.W_STATUS] & soa.STATUS_DONE), f"the episode ended at step {t + 1}"
    assert acts == KAT_ACTIONS, acts
    assert orc.records[0, soa.W_STATUS] & soa.STATUS_TERM, "the 30th step does not terminate"
    assert float(out[1][0, 0]) == KAT_REWARD and out[2][0, 0] == 1
