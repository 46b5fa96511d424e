"""Tasks on records: which recipe an env plays, and the goal vector, `recipe_done` and `task` the reference reports for it.

The reference fixes an env's recipes in its constructor and rebuilds their graphs at every `reset()` (cooking_env.py:197-201:
`recipe_graphs = [RECIPES[name]() ...]`, `update_recipe_state(world)` on each, `recipe_mapping = dict(zip(agents, graphs))`).  Its
`infos` carry `recipe_done` and `task` for every agent at every step (cooking_env.py:317-331), and the `"full"` observation returns
`goal_vector = recipe_mapping[agent].goals_completed(num_goals)` (cooking_env.py:277, recipe.py:36-40).  This module is the definition
of both for the batched env, on the host, from records alone (it never creates a device handle): `host_set_tasks` is those lines of
`reset()` applied to fresh graphs of OTHER names on the record's current world, `host_infos` reads the task state back.
`tests/golden/tasks_ref.json.gz` (tools/gen_tasks_golden.py) holds what the unmodified reference computes.

  * goal table: `goal_table(graphs, num_goals)[r][j]` is `node_list[j].id_num` of recipe r, 0xFF past its last node; `num_goals`
    follows cooking_env.py:100-105 (`current_num_goals`): NUM_GOALS with a user registry, else DEFAULT_NUM_GOALS (26);
  * goal vector of agent a: of the env's recipe slot a (`recipe_mapping`, cooking_env.py:201); `g[id] = not marked` for the LAST
    node of `node_list` that carries `id` (later nodes overwrite earlier ones, recipe.py:38-39: the node whose `counts` bit
    `Recipe.flatten` sets), 0 for ids no node of the recipe carries; `recipe_done[a]` is the root's mark, `task[a]` the recipe's
    index in `book_names`, `t` the record's step counter;
  * marks: record word 1 holds bits 8 r + j (node j of recipe slot r) while every graph of the book has at most 8 nodes, else 16
    bits per recipe: slots 0, 1 in word 1 and slots 2, 3 in word 7;
  * keyed draw: `task_draw(seed, env_global, episode, K) = min(int(u * K), K - 1)` with u the project's one counter-based stream
    (`cz_spawn_uniform`) at t = 0 under agent key 0x200, draw 0 - a key nobody else uses (spawn draws: agents 0..3; the layout
    generator: 0x100).

Deviations from the reference: none in the values; a recipe id outside the table in a used slot is refused (the env stays as it
was) where the reference raises KeyError when the name is looked up.
"""
from __future__ import annotations

import numpy as np

from cooking_zoo_amd import partner, soa
from cooking_zoo_amd.cooking_book import recipe_drawer

TASK_KEY = 0x200                     # the `agent` word of the keyed stream under which tasks are drawn
NO_NODE = 0xFF                       # goal table: past the recipe's last node; recipe ids: an unused slot
MAX_GOALS = 255


def current_num_goals():
    """cooking_env.py:100-105: a non-empty user registry counts its own ids"""
    return int(recipe_drawer.NUM_GOALS if recipe_drawer.RECIPE_STORE else recipe_drawer.DEFAULT_NUM_GOALS)


def goal_table(graphs, num_goals):
    """uint8 [len(graphs)][soa.MAX_NODES]: the goal id of every node, NO_NODE past the last one.  ValueError for more than 255 goals
    or an id outside [0, num_goals) (the reference raises IndexError there when the Recipe is made, recipe.py:34)"""
    num_goals = int(num_goals)
    if not 1 <= num_goals <= MAX_GOALS:
        raise ValueError(f"num_goals is {num_goals}, not in 1..{MAX_GOALS}")
    out = np.full((len(graphs), soa.MAX_NODES), NO_NODE, dtype=np.uint8)
    for r, g in enumerate(graphs):
        for j, node in enumerate(g.node_list):
            if not 0 <= int(node.id_num) < num_goals:
                raise ValueError(f"recipe {r} node {j} ({node.name!r}) has goal id {node.id_num}, not below num_goals = {num_goals}")
            out[r, j] = int(node.id_num)
    return out


def task_draw(seed, env_global, episode, K, uniform=None):
    """the row of a K-row task list that env `env_global` plays in episode `episode`.  `uniform(seed, env_global, episode, t, agent,
    draw)`: the keyed stream, by default the library's own host mirror cz_spawn_uniform"""
    if K < 1:
        raise ValueError("task_draw: K < 1")
    if uniform is None:
        from cooking_zoo_amd import _native
        uniform = _native.lib().cz_spawn_uniform
    u = float(uniform(int(seed), int(env_global), int(episode), 0, TASK_KEY, 0))
    return min(int(u * K), int(K) - 1)


def is_wide(tables):
    return tables.recipe_nodes != soa.NARROW_NODES


def pack_marks(marks, wide):
    """marks of the recipe slots 0..3 (a sequence of ints) -> (record word 1, record word 7)"""
    lo = hi = 0
    for r, m in enumerate(marks):
        if not wide:
            lo |= (int(m) & 0xFF) << (8 * r)
        elif r < 2:
            lo |= (int(m) & 0xFFFF) << (16 * r)
        else:
            hi |= (int(m) & 0xFFFF) << (16 * (r - 2))
    return lo, hi


def slot_marks(record, r, wide):
    """the node marks of recipe slot r of one record: bit j = node j"""
    if not wide:
        return (int(record[soa.W_MARKS]) >> (8 * r)) & 0xFF
    return (int(record[soa.W_MARKS if r < 2 else soa.W_MARKS_HI]) >> (16 * (r & 1))) & 0xFFFF


def _rows(records):
    recs = np.array(records, dtype=np.uint32)
    return recs.reshape(-1, recs.shape[-1])


def host_set_tasks(tables, records, chosen, recipe_ids=None, task_list=None, seed=0, env_begin=0):
    """cooking_env.py:197-201 with fresh graphs of other names, for the chosen records: -> (new records uint32 [n][RW], refused bool
    [n]).  `records` are envs [env_begin, env_begin + n) of `tables`' batch; `chosen` bool [n]; the new ids of env e are
    `recipe_ids[e]` (uint8 [n][4]) or, without them, row `task_draw(seed, env_id_base + env_begin + e, record's episode, K)` of
    `task_list` (uint8 [K][4]).  A chosen env with an id outside the table in one of its R used slots is refused and stays word for
    word as it was.  Otherwise word 5 becomes the new ids (slots >= R forced to 0xFF) and every recipe's marks are evaluated from
    scratch on the record's current world (partner.recipe_marks); everything else - t, status, episode, pool word, running returns,
    cells, objects - is untouched."""
    recs = _rows(records)
    n, R, wide = recs.shape[0], int(tables.num_recipes), is_wide(tables)
    chosen = np.asarray(chosen, dtype=bool).reshape(n)
    if recipe_ids is None and task_list is None:
        raise ValueError("host_set_tasks: neither recipe ids nor a task list")
    ids = None if recipe_ids is None else np.asarray(recipe_ids, dtype=np.uint8).reshape(n, 4)
    tl = None if task_list is None else np.asarray(task_list, dtype=np.uint8).reshape(-1, 4)
    if ids is None and len(tl) < 1:
        raise ValueError("host_set_tasks: a task list with K < 1")
    graphs = tables.recipe_graphs
    refused = np.zeros(n, dtype=bool)
    for e in np.nonzero(chosen)[0]:
        rec = recs[e]
        if ids is not None:
            new = ids[e].copy()
        else:
            new = tl[task_draw(seed, tables.env_id_base + env_begin + int(e), int(rec[soa.W_EPISODE]), len(tl))].copy()
        new[R:] = NO_NODE
        if (new[:R] >= len(graphs)).any():
            refused[e] = True
            continue
        world = partner._World(tables.dims, tables.layouts[int(rec[soa.W_LAYOUT])], rec)
        lo, hi = pack_marks([partner.recipe_marks(world, graphs[int(new[r])]) for r in range(R)], wide)
        rec[soa.W_RECIPES] = int(new[0]) | int(new[1]) << 8 | int(new[2]) << 16 | int(new[3]) << 24
        rec[soa.W_MARKS] = lo
        if wide:
            rec[soa.W_MARKS_HI] = hi
    return recs, refused


def host_infos(tables, records):
    """-> goal uint8 [n][A][G], done uint8 [n][A], task int32 [n][A], t int32 [n] of `records` (see the module text)"""
    recs = _rows(records)
    n, A, G, wide = recs.shape[0], int(tables.num_agents), int(tables.num_goals), is_wide(tables)
    goal, done = np.zeros((n, A, G), dtype=np.uint8), np.zeros((n, A), dtype=np.uint8)
    task = np.zeros((n, A), dtype=np.int32)
    for e, rec in enumerate(recs):
        for a in range(A):
            r = (int(rec[soa.W_RECIPES]) >> (8 * a)) & 0xFF
            task[e, a] = r
            marks = slot_marks(rec, a, wide)
            done[e, a] = marks & 1
            if r >= len(tables.goal_table):                            # (an unused slot, 0xFF: a recipe without nodes)
                continue
            for j in range(soa.MAX_NODES):
                gid = int(tables.goal_table[r, j])
                if gid != NO_NODE:
                    goal[e, a, gid] = 0 if marks >> j & 1 else 1       # (a later node of the same id overwrites: recipe.py:38-39)
    return goal, done, task, recs[:, soa.W_T].astype(np.int32)
