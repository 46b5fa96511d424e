"""Helpers of the scripted partner's tests (host and GPU): the fixture computed from the unmodified reference, the recipes of a
batch, recipe overrides that cover the book, the second, independent route to the answers - a plain model over the object view of
`symbolic.materialize` with Python lists and `sorted` -, the known-answer world, and sentinel-filled device buffers of the outputs.
Nothing here touches the device library."""
import functools
import gzip
import json
import os

import numpy as np

from cooking_zoo_amd import nav, partner, soa
from cooking_zoo_amd.cooking_world import symbolic
from cooking_zoo_amd.cooking_world.constants import BlenderFoodStates, ChopFoodStates
from cooking_zoo_amd.cooking_world.layout import Layout
from vec_common import GUARD

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_ACTIONS = "312442214141113331242131124444"
KAT_REWARD = 19.9875


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/partner_ref.json.gz (tools/gen_partner_golden.py); do not write to it"""
    with gzip.open(os.path.join(HERE, "golden", "partner_ref.json.gz")) as f:
        return json.load(f)


def golden_layout(ep):
    """what the host model needs of the episode's layout: the grid size and the static lists (cells from the first record)"""
    dims = soa.Dims(*ep["dims"])
    cells = soa.record_cells(dims, np.array(ep["states"][0]["record"], dtype=np.uint32)) & soa.CELL_TYPE_MASK
    return Layout(dims.W, dims.H, cells, {k: list(v) for k, v in ep["static_lists"].items()}, [], [], [])


def book_of(tables):
    """the loaded recipe table as cooking_book Recipes, in table order"""
    return list(tables.recipe_graphs)


def override_indices(n, A, R, shift):
    """int32 [n][A] recipe indices that cover the whole table over envs and agents; `shift` moves the pattern"""
    return ((np.arange(n)[:, None] + 3 * np.arange(A)[None, :] + shift) % R).astype(np.int32)


@functools.lru_cache(maxsize=None)
def kat_tables(n):
    """the world of golden set kat_c3 (coop_test, one agent, TomatoLettuceSalad, all dishes end the episode) as a one-layout pool"""
    from cooking_zoo_amd.vec_env import BatchTables
    from golden_io import GoldenSet, layout_from_episode
    gs = GoldenSet("kat_c3")
    ep = gs.episodes[0]
    t = BatchTables(n, gs.cfg["level"], gs.cfg["meta_file"], 1, 400, gs.cfg["recipes"], bool(gs.cfg["end_condition_all_dishes"]),
                    gs.cfg["action_scheme"], gs.cfg.get("reward_scheme"), layouts=[layout_from_episode(ep)])
    return t, np.array(ep.states[0], dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# the second route: the reference's functions restated over the object view, with lists and sorted
# ---------------------------------------------------------------------------------------------------------------------------

class Raised(Exception):
    pass


def plain_partner(dims, layout, record, recipe, a):
    """(action, target, status) of agent `a` by the second route"""
    view = symbolic.materialize(dims, layout, record)
    if "Floor" not in layout.static_lists:                               # (a layout rebuilt without its Floor list: cell order)
        cells = soa.record_cells(dims, np.asarray(record, dtype=np.uint32)) & soa.CELL_TYPE_MASK
        view["Floor"] = [symbolic._make("Floor", location=(int(c) % dims.W, int(c) // dims.W), content=[]) for c in np.nonzero(cells == 0)[0]]
    me = view["Agent"][a]
    here = tuple(me.location)
    floor = {tuple(o.location) for o in view["Floor"]}
    seen, todo = {here}, [here]
    while todo:                                                          # every cell a path from the agent can stand on
        x, y = todo.pop()
        for _c, dx, dy in nav.DELTAS:
            nx = (x + dx, y + dy)
            if nx in floor and nx not in seen:
                seen.add(nx)
                todo.append(nx)

    def reachable(loc):
        loc = tuple(loc)
        return loc in seen or any((loc[0] + dx, loc[1] + dy) in seen for _c, dx, dy in nav.DELTAS)

    def dist(loc):
        return ((loc[0] - here[0]) ** 2 + (loc[1] - here[1]) ** 2) ** 0.5

    def has(o, cond):
        attr, value = cond
        return getattr(o, attr, None) == value                           # (an attribute the class lacks meets nothing)

    walks = []

    def walk(loc):
        if loc is None:
            raise Raised("walk to None")
        walks.append(tuple(loc))
        field = nav.flood(nav.floor_set(dims, np.asarray(record, dtype=np.uint32)), loc[0], loc[1])
        return nav.first_move(field, here[0], here[1], loc[0], loc[1])[0]

    def closest(locs):
        best = None
        for loc in locs:
            if reachable(loc) and (best is None or dist(loc) < dist(best)):
                best = loc
        return best

    # update_recipe_state
    nodes = recipe.node_list
    found = {}
    for n in reversed(nodes):
        found[id(n)] = []
        if all(found.get(id(c)) for c in n.contains):
            found[id(n)] = [o for o in view.get(n.name, []) if all(has(o, c) for c in n.conditions)
                            and all(any(tuple(k.location) == tuple(o.location) for k in found[id(c)]) for c in n.contains)]
    open_nodes = [n for n in nodes if not found[id(n)]]
    if not open_nodes:
        return 0, partner.NO_TARGET, partner.DONE
    node = open_nodes[-1]
    try:
        ranked = sorted(view.get(node.name, []), key=lambda o: (sum(not has(o, c) for c in node.conditions), dist(o.location)))
        if not ranked:
            raise Raised("no object of the class")
        obj, action = ranked[0], 0
        unmet = [c for c in node.conditions if not has(obj, c)]
        name = {ChopFoodStates.CHOPPED: "Cutboard", BlenderFoodStates.MASHED: "Blender"}.get(unmet[0][1]) if unmet else None
        if name:
            apps = [p for p in view.get(name, []) if reachable(p.location)]
            counters = [c for c in view.get("Counter", []) if reachable(c.location)]
            free = [p.location for p in apps if not p.content]
            if any(obj in p.content for p in apps):
                action = walk(obj.location)
            elif obj is me.holding:
                action = walk(closest(free) if free else closest([c.location for c in counters]))
            elif free:
                action = walk(closest([c.location for c in counters if not c.content])) if me.holding is not None else walk(obj.location)
            else:
                action = walk(closest([p.location for p in apps]))
        if action:
            return action, walks[-1], partner.WALK
        kids = [(c, [o for o in view.get(c.name, []) if reachable(o.location)]) for c in node.contains]
        mains = [m for m in view.get(node.name, []) if reachable(m.location)]

        def count(m):
            return sum(1 for c, objs in kids for o in objs if tuple(o.location) == tuple(m.location) and all(has(o, k) for k in c.conditions))

        main = sorted(mains, key=lambda m: (-count(m), dist(m.location)))[0] if mains else None
        pool = [o for _c, objs in kids for o in objs]
        if pool and main is None:
            raise Raised("no main object")
        pool = sorted((o for o in pool if tuple(o.location) != tuple(main.location)), key=lambda o: dist(o.location)) if pool else []
        if not pool:
            return 0, partner.NO_TARGET, partner.IDLE
        action = walk(main.location if tuple(pool[0].location) == here else pool[0].location)
        return action, walks[-1], partner.WALK
    except Raised:
        return 0, partner.NO_TARGET, partner.RAISES


# ---------------------------------------------------------------------------------------------------------------------------
# sentinel-filled device buffers of the three outputs
# ---------------------------------------------------------------------------------------------------------------------------

OUTPUTS = ("action", "target", "status")
OUTPUT_SUBSETS = [tuple(f for k, f in enumerate(OUTPUTS) if m >> k & 1) for m in range(1, 8)]      # the 7 non-empty ones
SENT = dict(action=0x5A5A5A5A, target=0x6B6B6B6B, status=0xEE)                 # no walk code, no coordinate or -1, no status


class PartnerBufs:
    """the three outputs laid out for n envs, each with GUARD 32-bit words behind it, all filled with their sentinels"""

    def __init__(self, env, n):
        A = env.num_agents
        self.n, self.A = n, A
        self.shape = dict(action=(n, A), target=(n, A, 2), status=(n, A))
        self.dtype = dict(action=np.int32, target=np.int32, status=np.uint8)
        self.size = {f: int(np.prod(s)) for f, s in self.shape.items()}
        self.guard = {f: GUARD * 4 // np.dtype(self.dtype[f]).itemsize for f in OUTPUTS}
        self.buf = {f: env.alloc((self.size[f] + self.guard[f],), self.dtype[f]) for f in OUTPUTS}
        self.fill()

    def fill(self):
        for f in OUTPUTS:
            self.buf[f].from_host(np.full(self.size[f] + self.guard[f], SENT[f], dtype=self.dtype[f]))

    def args(self, outputs):
        return {("d_" + f): self.buf[f] for f in outputs}

    def read(self, f):
        got = self.buf[f].to_host()
        return got[:self.size[f]].reshape(self.shape[f]), got[self.size[f]:]

    def check(self, ctx, outputs, want, agents=None):
        """a named buffer holds `want` = (actions, targets, status) for the driven agents and its sentinel for the others, its guard
        is untouched; a buffer the call did not name keeps its sentinel everywhere"""
        mask = (1 << self.A) - 1 if agents is None else agents
        driven = np.array([bool(mask >> a & 1) for a in range(self.A)])
        for f, w in zip(OUTPUTS, want):
            body, guard = self.read(f)
            sent = np.array(SENT[f]).astype(self.dtype[f])
            if f not in outputs:
                assert (body == sent).all() and (guard == sent).all(), f"{ctx}: {f} was not named and was written"
                continue
            assert (guard == sent).all(), f"{ctx}: {f}: a store went behind the last element"
            assert (body[:, ~driven] == sent).all(), f"{ctx}: {f}: an entry of an agent that is not driven was written"
            w = np.asarray(w).reshape(body.shape)
            bad = np.argwhere(body[:, driven] != w[:, driven])
            assert not len(bad), (f"{ctx}: {f} differs from the host model at (env, driven agent..) {bad[:6].tolist()}: got "
                                  f"{body[:, driven][tuple(bad[0])]}, want {w[:, driven][tuple(bad[0])]}")
