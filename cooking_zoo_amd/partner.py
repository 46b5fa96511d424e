"""The scripted partner: `CookingAgent.step` of the reference, defined on records.

The reference's heuristic partner (`cooking_agents/cooking_agent.py:9-119`, `base_agent.py:128-198`) decides, from the symbolic
observation, which object to walk to, and walks there with `walk_to_location` (cooking_zoo_amd/nav.py).  Its only memory is the
`reachable` cache, and the Floor set never changes inside an episode, so the answer is a pure function of (record, recipe, agent);
this module is that function for the batched env, on the host, from records alone (it never loads the device library).
`tests/golden/partner_ref.json.gz` (tools/gen_partner_golden.py) holds what a fresh, unmodified `CookingAgent` returns.

Per agent: `action` 0..4 (the walk codes), `target` (x, y) - the location handed to the `walk_to_location` call whose result was
returned, (-1, -1) when no walk produced the answer - and `status`:

    DONE   0  every node of the recipe is marked (cooking_agent.py:14-15), or the env's recipe slot is unused; action 0
    WALK   1  the action is the result of a walk to `target` (0 at the goal, or when the goal is unreachable)
    IDLE   2  the reference returns 0 without a walk (cooking_agent.py:30, :53 falling through)
    RAISES 3  the reference raises here: no object of the node's class (IndexError, cooking_agent.py:48), a walk to the None that
              `closest` found (TypeError, base_agent.py:64), or no reachable main object while a reachable child object exists
              (AttributeError, cooking_agent.py:63); action 0, target (-1, -1)
    ABSENT 4  the agent's despawn bit is set in the status word; action 0

The steps (line numbers of the reference):

  * marks: `update_recipe_state` (recipe.py:77-104) of the asked recipe on the current record - record word 1 holds the marks of
    the env's own recipes only; the node is the unmarked one with the HIGHEST `node_list` index (base_agent.py:49-53);
  * the condition branch (cooking_agent.py:41-53): candidates are all live objects of the node's class, reachable or not, in list
    order; the best has the fewest unmet conditions, then the smallest distance to the agent, the earlier in the list on ties
    (`sorted` is stable); its first unmet condition IN THE NODE'S ORDER chooses the appliance (CHOPPED: Cutboard, MASHED: Blender,
    anything else: 0); a result of 0 - a walk that returned 0 included - falls through to the contains branch (:21);
  * `generic_sequence` (base_agent.py:155-190), tags of `Answer.tags` in brackets: the object lies directly on a reachable
    appliance: walk to it [on_appliance]; it is the held object: to the closest reachable empty appliance [held_to_appliance], or,
    none being empty, to the closest reachable Counter, empty or not [held_to_counter]; otherwise, with a reachable empty
    appliance: hands full: to the closest reachable empty Counter [drop_held], hands empty: to the object [fetch]; no empty
    appliance: to the closest reachable appliance [wait_appliance].  `closest` takes the first strict minimum in list order; None
    followed by the walk raises;
  * the contains branch (cooking_agent.py:26-39, 55-119): the main object is the reachable object of the node's class with the most
    reachable child objects that meet their node's conditions at its location, the strictly nearer on an equal count, the earlier
    in the list otherwise; the object to fetch is the nearest reachable child object that is not at the main object's location,
    children in `contains` order, objects in list order, strict `<`; none: 0 [no_child]; it is at the agent's own cell (held, or in
    the held plate): walk to the main object [to_main], else walk to it [to_child];
  * distances are square roots of sums of two squares below 2 * 32 * 32, so the integer squares order alike: integers everywhere;
  * every `reachable` query starts or ends at the agent's cell: one fill from the agent's cell over the Floor set answers all of
    them - a location is reachable iff it is the agent's cell, lies in the fill or has a 4-neighbour in the fill;
  * list orders: dynamic classes in slot order, static classes in `Layout.static_lists` order, which is not cell order (the
    statics are the record's cells of the type, ordered by the rank the layout's lists give them, then by cell).

Deviations from the reference: those of nav.py; a condition on an attribute the object's class lacks (the reference raises
AttributeError) counts as unmet, as in `cooking_book.recipe._condition_code`; a slot outside the grid or of no class is not an
object and an agent outside the grid is IDLE (no valid record has either); a despawned agent is ABSENT (the reference's own demo,
`demo_heuristic_agent_with_spawn.py`, does not ask an agent that is missing from the observations); node classes other than the 7
static and 10 dynamic ones have no objects.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from cooking_zoo_amd import nav, soa
from cooking_zoo_amd.cooking_world.constants import BlenderFoodStates, ChopFoodStates

DONE, WALK, IDLE, RAISES, ABSENT = range(5)
STATUS_NAMES = ("DONE", "WALK", "IDLE", "RAISES", "ABSENT")
NO_TARGET = (-1, -1)
SPAWN_GONE0 = 8                                                        # status word: bit 8 + a = agent a is despawned
ATTR_CHOP, ATTR_BLEND = 0, 1                                           # the attribute codes of the device's condition table
_VALUE_CODES = {"chop_state": {ChopFoodStates.FRESH.value: 0, ChopFoodStates.CHOPPED.value: 1},
                "blend_state": {BlenderFoodStates.FRESH.value: 0, BlenderFoodStates.IN_PROGRESS.value: 1, BlenderFoodStates.MASHED.value: 2}}
APPLIANCE = {(ATTR_CHOP, 1): "Cutboard", (ATTR_BLEND, 2): "Blender"}   # base_agent.py:141-147 (CHOPPED, MASHED); anything else: none

# action, target, status; walks: walk_to_location calls; last_walk: the argument of the last one; tags: the branches taken
Answer = namedtuple("Answer", "action target status walks last_walk tags")


class _Raise(Exception):
    pass


Obj = namedtuple("Obj", "cls loc slot chopped mashed held_by plate static")  # slot -1: a static object; plate: the slot of the plate it is in


def rank_table(layout):
    """uint16 [W * H]: the position of the cell's static object in `world_objects[class]` (Layout.static_lists)"""
    rank = np.zeros(layout.width * layout.height, dtype=np.uint16)
    for cells in static_lists(layout).values():
        for k, c in enumerate(cells):
            rank[c] = k
    return rank


def static_lists(layout):
    """`Layout.static_lists`; a layout without a Floor list (rebuilt from a fixture that left it out) gets the Floor cells in cell
    order, which is their creation order (parsing.py:8-17: the base grid row by row, less the cells a static object replaced)"""
    lists = dict(layout.static_lists)
    if "Floor" not in lists:
        floor = soa.STATIC_CLASSES.index("Floor")
        lists["Floor"] = [int(c) for c in np.nonzero((np.asarray(layout.cells) & soa.CELL_TYPE_MASK) == floor)[0]]
    return lists


def condition_pairs(node):
    """the node's conditions as (attribute, wanted value) integer pairs in the node's own order: attribute 0 chop_state,
    1 blend_state; value as the reference's enums number them (FRESH 0, CHOPPED 1 / IN_PROGRESS 1, MASHED 2)"""
    out = []
    for attr, value in node.conditions:
        code = _VALUE_CODES.get(attr, {}).get(getattr(value, "value", value))
        if code is None:
            raise ValueError(f"unsupported recipe condition {(attr, value)!r}")
        out.append((ATTR_CHOP if attr == "chop_state" else ATTR_BLEND, code))
    return out


ROW_WORDS, MAX_CONDS = 1 + 2 * soa.MAX_NODES, 8                       # one row of the device's partner table (cz_load_partner_table)


def partner_rows(recipes):
    """uint32 [len(recipes)][ROW_WORDS]: per recipe the node count, then per node  class | conditions << 8 | child mask << 16  and
    the conditions in the node's own order, 4 bits each: attribute | wanted value << 1"""
    out = np.zeros((len(recipes), ROW_WORDS), dtype=np.uint32)
    for r, recipe in enumerate(recipes):
        nodes = recipe.node_list
        index = {id(n): j for j, n in enumerate(nodes)}
        out[r, 0] = len(nodes)
        for j, n in enumerate(nodes):
            pairs = condition_pairs(n)
            if len(pairs) > MAX_CONDS:
                raise ValueError(f"recipe node {n.name!r} has {len(pairs)} conditions, the partner table holds {MAX_CONDS}")
            kids = 0
            for c in n.contains:
                kids |= 1 << index[id(c)]
            out[r, 1 + 2 * j] = soa.class_node_id(n.name) | (len(pairs) << 8) | (kids << 16)
            out[r, 2 + 2 * j] = sum((at | v << 1) << (4 * q) for q, (at, v) in enumerate(pairs))
    return out


class _World:
    """the objects of one record, per class in list order, and the agent's reachability"""

    def __init__(self, dims, layout, record):
        self.dims, self.W, self.H = dims, dims.W, dims.H
        rec = np.asarray(record, dtype=np.uint32)
        self.rec = rec
        self.agents = [soa.unpack_agent(rec[soa.AGENT_WORD0 + a]) for a in range(dims.A)]
        held_by = {h: a for a, (_x, _y, _o, h) in enumerate(self.agents) if h >= 0}
        self.by_class = {}
        cells = soa.record_cells(dims, rec)
        rank = rank_table(layout)
        for t, name in enumerate(soa.STATIC_CLASSES):                  # the record's cells of the type, in the layout's list order
            lst = sorted((int(rank[c]), int(c)) for c in np.nonzero((cells & soa.CELL_TYPE_MASK) == t)[0])
            self.by_class[name] = [Obj(name, (c % dims.W, c // dims.W), -1, False, False, -1, -1, True) for _r, c in lst]
        self.direct = set()                                            # cells with an object lying directly on them
        for s in range(dims.D):
            x, y, cls, flags = soa.unpack_dyn0(rec[dims.dyn0_word0 + s])
            if not flags & soa.DYN_ALIVE or cls >= len(soa.DYNAMIC_CLASSES) or x >= dims.W or y >= dims.H:
                continue                                               # (no valid record has the last three)
            plate, _seq = soa.unpack_dyn1(rec[dims.dyn1_word0 + s])
            name = soa.DYNAMIC_CLASSES[cls]
            o = Obj(name, (x, y), s, bool(flags & soa.DYN_CHOPPED), bool(flags & soa.DYN_MASHED) and cls in soa.BLENDER_FOOD,
                    held_by.get(s, -1), plate, False)
            self.by_class.setdefault(name, []).append(o)
            if o.held_by < 0 and plate < 0:
                self.direct.add((x, y))
        self.floor = nav.floor_set(dims, rec)
        self._fields = {}

    def objects(self, name):
        return self.by_class.get(name, [])

    def field(self, g):
        if g not in self._fields:
            self._fields[g] = nav.flood(self.floor, g[0], g[1])
        return self._fields[g]


def meets(o, attr, value):
    """getattr(obj, attr) == value, an attribute the class lacks meeting nothing"""
    if o.static or o.cls == "Plate":
        return False
    if attr == ATTR_CHOP:
        return value == (1 if o.chopped else 0)
    if o.cls not in ("Carrot", "Banana"):
        return False
    return value == (2 if o.mashed else 0)


def recipe_marks(world, recipe):
    """bit j = node j marked: recipe.py:77-104 on the record's objects"""
    nodes = recipe.node_list
    index = {id(n): j for j, n in enumerate(nodes)}
    marks, locs = 0, {}
    for j in range(len(nodes) - 1, -1, -1):
        n = nodes[j]
        locs[j] = set()
        kids = [index[id(c)] for c in n.contains]
        if not all(marks >> k & 1 for k in kids):
            continue
        pairs = condition_pairs(n)
        for o in world.objects(n.name):
            if all(meets(o, at, v) for at, v in pairs) and all(o.loc in locs[k] for k in kids):
                locs[j].add(o.loc)
                marks |= 1 << j
    return marks


def _d2(p, q):
    return (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2


def agent_answer(dims, layout, record, recipe, a):
    """the Answer of agent `a` asked for `recipe` (a cooking_book Recipe) on `record`; the despawn bit is not looked at"""
    w = _World(dims, layout, record)
    ax, ay, _o, held_slot = w.agents[a]
    L = (ax, ay)
    W, H = dims.W, dims.H
    if not (ax < W and ay < H):
        return Answer(0, NO_TARGET, IDLE, 0, None, ("off_grid",))
    fill = w.field(L) >= 0                                             # the agent's cell and every Floor cell a path from it reaches

    def reachable(loc):
        x, y = loc
        if not (0 <= x < W and 0 <= y < H):
            return False
        if loc == L or fill[x, y]:
            return True
        return any(0 <= x + dx < W and 0 <= y + dy < H and fill[x + dx, y + dy] for _c, dx, dy in nav.DELTAS)

    walks, tags = [], []

    def walk(loc, tag):
        tags.append(tag)
        if loc is None:
            raise _Raise("TypeError")                                  # base_agent.py:64
        walks.append(loc)
        return nav.first_move(w.field(loc), ax, ay, loc[0], loc[1])[0]

    def closest(origin, locs):                                         # base_agent.py:128-138; every origin is the agent's cell
        best, bd = None, None
        for loc in locs:
            if reachable(loc) and (bd is None or _d2(origin, loc) < bd):
                best, bd = loc, _d2(origin, loc)
        return best

    def generic_sequence(appliance, o):                                # base_agent.py:155-190
        apps = [p for p in w.objects(appliance) if reachable(p.loc)]
        on = not o.static and o.held_by < 0 and o.plate < 0
        for p in apps:
            if on and p.loc == o.loc:
                return walk(o.loc, "on_appliance")
        empty = [p.loc for p in apps if p.loc not in w.direct]
        if not o.static and o.slot == held_slot:
            if empty:
                return walk(closest(o.loc, empty), "held_to_appliance")
            return walk(closest(o.loc, [c.loc for c in w.objects("Counter") if reachable(c.loc)]), "held_to_counter")
        if empty:
            if held_slot >= 0:
                return walk(closest(L, [c.loc for c in w.objects("Counter") if reachable(c.loc) and c.loc not in w.direct]), "drop_held")
            return walk(o.loc, "fetch")
        return walk(closest(L, [p.loc for p in apps]), "wait_appliance")

    def condition_action(node):                                        # cooking_agent.py:41-53
        pairs = condition_pairs(node)
        best, bk = None, None
        for o in w.objects(node.name):
            k = (sum(not meets(o, at, v) for at, v in pairs), _d2(L, o.loc))
            if bk is None or k < bk:
                best, bk = o, k
        if best is None:
            raise _Raise("IndexError")                                 # cooking_agent.py:48
        for at, v in pairs:
            if not meets(best, at, v):
                appliance = APPLIANCE.get((at, v))
                if appliance is None:
                    tags.append("no_appliance")                        # base_agent.py:153
                    return 0
                return generic_sequence(appliance, best)
        tags.append("conditions_met")
        return 0

    def contains_action(node):                                         # cooking_agent.py:26-39
        kids = [(c, condition_pairs(c), [o for o in w.objects(c.name) if reachable(o.loc)]) for c in node.contains]
        main, bc = None, -1
        for m in w.objects(node.name):                                 # get_location_with_most_objects, :96-119
            if not reachable(m.loc):
                continue
            count = sum(1 for _c, pairs, objs in kids for o in objs if o.loc == m.loc and all(meets(o, at, v) for at, v in pairs))
            if count > bc or (count == bc and _d2(L, m.loc) < _d2(L, main.loc)):
                main, bc = m, count
        child, bd = None, None
        for _c, _pairs, objs in kids:                                  # get_best_contains_obj, :55-72
            for o in objs:
                if main is None:
                    raise _Raise("AttributeError")                     # :63, node_world_object is None
                if o.loc != main.loc and (bd is None or _d2(L, o.loc) < bd):
                    child, bd = o, _d2(L, o.loc)
        if child is None:
            tags.append("no_child")
            return 0, False
        if child.loc == L:
            tags.append("child_underfoot" if child.static else "child_held" if child.slot == held_slot else "child_in_held_plate")
            return walk(main.loc, "to_main"), True
        return walk(child.loc, "to_child"), True

    marks = recipe_marks(w, recipe)
    node = None
    for j in range(len(recipe.node_list) - 1, -1, -1):
        if not marks >> j & 1:
            node = recipe.node_list[j]
            break
    if node is None:
        return Answer(0, NO_TARGET, DONE, 0, None, ("done",))
    try:
        action = condition_action(node)
        walked = bool(walks)
        if not action:
            action, walked = contains_action(node)
    except _Raise as e:
        return Answer(0, NO_TARGET, RAISES, len(walks), walks[-1] if walks else None, tuple(tags) + (str(e),))
    last = walks[-1] if walks else None
    if walked:
        return Answer(int(action), last, WALK, len(walks), last, tuple(tags))
    return Answer(0, NO_TARGET, IDLE, len(walks), last, tuple(tags))


def host_partner(dims, layouts, records, recipes, agents=None, recipe_idx=None):
    """records uint32 [n][RW] (or one record); `layouts`: the layout pool (record word 2 indexes it); `recipes`: the loaded recipe
    table, a list of cooking_book Recipes; `agents`: bit a = agent a is driven (None: all); `recipe_idx` int [n][A]: indices
    into `recipes` (None: the env's own recipe of slot a, record word 5; 0xFF: DONE; an index outside the table: IDLE)
    -> actions int32 [n][A], targets int32 [n][A][2], status uint8 [n][A]; an agent that is not driven gets 0, (-1, -1), IDLE"""
    recs = np.asarray(records, dtype=np.uint32)
    single = recs.ndim == 1
    recs = recs.reshape(-1, recs.shape[-1])
    n, A = recs.shape[0], dims.A
    mask = (1 << A) - 1 if agents is None else int(agents)
    if mask == 0 or mask >> A:
        raise ValueError(f"agents is {mask:#x}: no bit, or a bit at or above the {A} agents")
    idx = None if recipe_idx is None else np.asarray(recipe_idx, dtype=np.int64).reshape(n, A)
    actions, targets = np.zeros((n, A), np.int32), np.full((n, A, 2), -1, np.int32)
    status = np.full((n, A), IDLE, np.uint8)
    for i, rec in enumerate(recs):
        layout = layouts[int(rec[soa.W_LAYOUT])]
        for a in range(A):
            if not mask >> a & 1:
                continue
            if int(rec[soa.W_STATUS]) >> (SPAWN_GONE0 + a) & 1:
                status[i, a] = ABSENT
                continue
            if idx is None:
                r = int(rec[soa.W_RECIPES]) >> (8 * a) & 0xFF
                if r == 0xFF:
                    status[i, a] = DONE
                    continue
            else:
                r = int(idx[i, a])
            if not 0 <= r < len(recipes):
                continue
            ans = agent_answer(dims, layout, rec, recipes[r], a)
            actions[i, a], targets[i, a], status[i, a] = ans.action, ans.target, ans.status
    if single:
        return actions[0], targets[0], status[0]
    return actions, targets, status
