"""Helpers of the task tests (host and GPU): the fixture computed from the unmodified reference, device-free tables over a golden
episode, the oracle of a switched trajectory, the host model of one device call, and sentinel-filled device buffers of the five
outputs of `infos_device`.  Nothing here touches the device library."""
import contextlib
import functools
import gzip
import json
import os
import types

import numpy as np

from cooking_zoo_amd import soa, tasks
from cooking_zoo_amd.cooking_book.recipe import Recipe, RecipeNode
from cooking_zoo_amd.cooking_book.recipe_drawer import RECIPES
from cooking_zoo_amd.cooking_world.constants import ChopFoodStates
from cooking_zoo_amd.cooking_world.layout import Layout
from vec_common import GUARD

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/tasks_ref.json.gz (tools/gen_tasks_golden.py); do not write to it"""
    with gzip.open(os.path.join(HERE, "golden", "tasks_ref.json.gz")) as f:
        return json.load(f)


def golden_tables(ep, first_record, graphs=None, num_goals=None, R=None):
    """what the host model reads of a `BatchTables`, over one golden episode: its dims, a one-layout pool (the grid and the static
    lists; cells from `first_record`), the book (`graphs`: the default one), R recipe slots (the agents' number unless given)"""
    dims = soa.Dims(*ep["dims"])
    cells = soa.record_cells(dims, np.array(first_record, dtype=np.uint32)) & soa.CELL_TYPE_MASK
    layout = Layout(dims.W, dims.H, cells, {k: list(v) for k, v in ep["static_lists"].items()}, [], [], [])
    graphs = [RECIPES[n]() for n in golden()["recipe_names"]] if graphs is None else graphs
    G = golden()["num_goals"] if num_goals is None else num_goals
    return types.SimpleNamespace(dims=dims, layouts=[layout], recipe_graphs=graphs, recipe_nodes=soa.NARROW_NODES, num_agents=dims.A,
                                 num_recipes=dims.A if R is None else R, num_goals=G, goal_table=tasks.goal_table(graphs, G), env_id_base=0)


@contextlib.contextmanager
def fresh_user_registry(first_id=0):
    """the fixture recipes (host_common.register_fixture_recipes) in a registry whose id counter starts at `first_id`, as in a fresh
    process: the counter is process-global and never goes back, so deep into a test session its ids no longer fit the byte a goal
    table has for them.  Afterwards the registry is empty and the counter stands behind the ids it gave - consistent for whoever
    registers next."""
    from cooking_zoo_amd.cooking_book import recipe_drawer as rd
    from host_common import register_fixture_recipes
    assert not rd.RECIPE_STORE
    rd.NUM_GOALS, rd._user_ids = int(first_id), iter(range(int(first_id), 1 << 30))     # (the module has no call for this, as the reference has none)
    register_fixture_recipes()
    try:
        yield
    finally:
        rd.RECIPE_STORE.clear()


def shared_id_recipe(nodes):
    """the hand-built recipe of the golden's `shared_id` part from its stored node list: [name, id_num, conditions, children]"""
    values = {"CHOPPED": ChopFoodStates.CHOPPED}
    made = [None] * len(nodes)
    for j in range(len(nodes) - 1, -1, -1):                              # children follow their parent in node_list
        name, id_num, conds, kids = nodes[j]
        made[j] = RecipeNode(root_type=name, id_num=id_num, name=name, conditions=[(a, values[v]) for a, v in conds],
                             contains=[made[k] for k in kids])
    return Recipe(made[0], 1 + max(n[1] for n in nodes), "SharedId")


def switch_oracle(ep):
    """the C oracle of one switched trajectory: the episode's level as a one-layout pool, auto-reset off"""
    from cooking_zoo_amd.cooking_world.engine.load_level import load_meta_file
    from golden_io import recipe_table
    from oracle_binding import Oracle
    dims = soa.Dims(*ep["dims"])
    off, cells = [0], []
    for name in soa.STATIC_CLASSES:
        cells += [y * dims.W + x for x, y in ep["statics"].get(name, [])]
        off.append(len(cells))
    lay = (np.array(ep["initial_record"], dtype=np.uint32), np.asarray(off, dtype=np.int32), np.asarray(cells, dtype=np.int16))
    return Oracle(dims, load_meta_file(ep["meta"]), recipe_table(), [lay], scheme=3 if ep["scheme"] == "scheme3" else 1,
                  max_steps=ep["max_steps"], end_condition_all=ep["all_dishes"], num_recipes=len(ep["new_recipes"]))


def ids_rows(rows):
    """recipe ids per env, any width up to 4 -> uint8 [n][4], 0xFF in the slots not given"""
    rows = np.asarray(rows, dtype=np.int64)
    out = np.full((rows.shape[0], 4), 0xFF, dtype=np.uint8)
    out[:, :rows.shape[1]] = rows
    return out


def task_list_draws(tables, records, task_list, seed):
    """the row of `task_list` every env of `records` (the whole batch of `tables`) draws: int [n]"""
    return np.array([tasks.task_draw(seed, tables.env_id_base + e, int(r[soa.W_EPISODE]), len(task_list)) for e, r in enumerate(records)])


# ---------------------------------------------------------------------------------------------------------------------------
# sentinel-filled device buffers of the five outputs
# ---------------------------------------------------------------------------------------------------------------------------

OUTPUTS = ("goal8", "goal32", "recipe_done", "task", "t")
OUTPUT_SUBSETS = [tuple(f for k, f in enumerate(OUTPUTS) if m >> k & 1) for m in range(1, 32)]      # the 31 non-empty ones
SENT = dict(goal8=0xA7, goal32=0x7FC0BEEF, recipe_done=0xB9, task=0x5A5A5A5A, t=0x6B6B6B6B)      # no 0 / 1, no index, no step count
DTYPE = dict(goal8=np.uint8, goal32=np.uint32, recipe_done=np.uint8, task=np.int32, t=np.int32)   # (goal32: the floats' bits)


class InfoBufs:
    """the five outputs laid out for n envs, each with GUARD 32-bit words in front of it and behind it, all filled with sentinels"""

    def __init__(self, env, n):
        A, G = env.num_agents, env.num_goals
        self.n = n
        self.shape = dict(goal8=(n, A, G), goal32=(n, A, G), recipe_done=(n, A), task=(n, A), t=(n,))
        self.size = {f: int(np.prod(s)) for f, s in self.shape.items()}
        self.guard = {f: GUARD * 4 // np.dtype(DTYPE[f]).itemsize for f in OUTPUTS}
        self.buf = {f: env.alloc((self.size[f] + 2 * self.guard[f],), DTYPE[f]) for f in OUTPUTS}
        self.fill()

    def fill(self):
        for f in OUTPUTS:
            self.buf[f].from_host(np.full(self.size[f] + 2 * self.guard[f], SENT[f], dtype=DTYPE[f]))

    def args(self, outputs):
        """keyword arguments of `infos_device`: the body of every named buffer (a raw device address behind the front guard)"""
        return {("d_" + f): int(self.buf[f].ptr) + GUARD * 4 for f in outputs}

    def check(self, ctx, outputs, want):
        """a named buffer holds `want` = (goal uint8, done, task, t) - goal32 the same as 0.0 / 1.0 - between untouched guards; a
        buffer the call did not name keeps its sentinel everywhere"""
        goal, done, task, t = want
        expect = dict(goal8=goal, goal32=np.asarray(goal, dtype=np.float32).view(np.uint32), recipe_done=done, task=task, t=t)
        for f in OUTPUTS:
            got = self.buf[f].to_host()
            g = self.guard[f]
            front, body, back = got[:g], got[g:g + self.size[f]].reshape(self.shape[f]), got[g + self.size[f]:]
            sent = np.array(SENT[f]).astype(DTYPE[f])
            assert (front == sent).all() and (back == sent).all(), f"{ctx}: {f}: a store went outside the rows"
            if f not in outputs:
                assert (body == sent).all(), f"{ctx}: {f} was not named and was written"
                continue
            w = np.asarray(expect[f]).reshape(body.shape)
            bad = np.argwhere(body != w)
            assert not len(bad), f"{ctx}: {f} differs from the host model at {bad[:6].tolist()}: got {body[tuple(bad[0])]}, want {w[tuple(bad[0])]}"
