"""Shortest-path navigation: `BaseAgent.walk_to_location` and `reachable` of the reference, defined on records.

The reference's scripted partner (`cooking_agents/base_agent.py:62-126`) walks by a breadth-first search from the agent's cell
over the `observation["Floor"]` tiles, the goal cell admitted whatever it is; every node is expanded in the order of the walk
codes 0:(0,0) 1:(-1,0) 2:(+1,0) 3:(0,+1) 4:(0,-1), and the first move of the first path found is returned.  That path is the
lexicographically smallest shortest path in move codes, so one flood fill from the GOAL answers every start:

    F = the cells of type Floor (a walkable Block is not in observation["Floor"]: objects are keyed by class name);
    field[g] = 0; for c in F, field[c] = the breadth-first distance from g, every cell entered being in F; every other cell
    is unreachable (UNREACHABLE = 0xFFFF);
    start s == g: action 0, steps 0;
    otherwise among the neighbours n = s + delta of codes 1, 2, 3, 4 that lie in the grid and have a finite field[n] (they are in
    F or are g), the smallest field[n] wins, the first code on ties: action = the code, steps = field[n] + 1;
    no such neighbour: action 0, steps -1.

`reachable(a, b)` of the reference is `steps >= 0`.  This module is the definition for the batched env, on the host, from records
alone (it never loads the device library); `k_navigate` (csrc/cz_query.h, `CookingVecEnv.navigate_device`) computes the same
on the device.  `tests/golden/nav_ref.json.gz` (tools/gen_nav_golden.py) holds what the unmodified reference returns.

Deviations from the reference:
  * a target with a coordinate outside [0, W) x [0, H) is "no target": action 0, steps -1, field all unreachable ((-1, -1) is the
    padding value) - the reference would walk towards an off-grid goal next to a floor tile;
  * a despawned agent is routed from its stored location;
  * the reference's `reachable` cache can answer from a stale world; there is no cache here.
An agent whose stored location lies outside the grid (no valid record has one) gets action 0, steps -1.

`walkable_blocks=True` (CZ_NAV_WALKABLE_BLOCKS) adds the Blocks whose walkable bit is set to F - cells `world_step` lets an agent
enter; the default is what `BaseAgent` sees.

Memory layout: targets int32 [n][A][T][2] (x, y); actions and steps int32 [n][A][T] (with T = 1 the actions are the [n][A] array a
step takes: the walk codes are the same in both action schemes); field uint16 [n][A][T][W * H], cell (x, y) at x * H + y as in
the grid observation.
"""
from __future__ import annotations

import numpy as np

from cooking_zoo_amd import soa

MAX_TARGETS = 8
UNREACHABLE = 0xFFFF
WALKABLE_BLOCKS = 1                                                    # the flag bit of cz_navigate_device
DELTAS = ((1, -1, 0), (2, 1, 0), (3, 0, 1), (4, 0, -1))               # code, dx, dy: base_agent.py:26-32


def floor_set(dims, record, walkable_blocks=False):
    """bool [W][H]: the cells a path may cross"""
    cells = soa.record_cells(dims, np.asarray(record, dtype=np.uint32)).astype(np.uint32)
    ty = cells & soa.CELL_TYPE_MASK
    ok = ty == soa.STATIC_CLASSES.index("Floor")
    if walkable_blocks:
        ok |= (ty == soa.STATIC_CLASSES.index("Block")) & ((cells & soa.CELL_WALK) != 0)
    return np.ascontiguousarray(ok.reshape(dims.H, dims.W).T)


def flood(floor, gx, gy):
    """int32 [W][H]: field of the goal (gx, gy) over `floor`, -1 where unreachable; all -1 for a goal outside the grid"""
    W, H = floor.shape
    field = np.full((W, H), -1, dtype=np.int32)
    if not (0 <= gx < W and 0 <= gy < H):
        return field
    field[gx, gy] = 0
    frontier, d = [(gx, gy)], 0
    while frontier:
        d += 1
        nxt = []
        for x, y in frontier:
            for _code, dx, dy in DELTAS:
                nx, ny = x + dx, y + dy
                if 0 <= nx < W and 0 <= ny < H and floor[nx, ny] and field[nx, ny] < 0:
                    field[nx, ny] = d
                    nxt.append((nx, ny))
        frontier = nxt
    return field


def first_move(field, sx, sy, gx, gy):
    """(action, steps) of the start (sx, sy) on the field of the goal (gx, gy)"""
    W, H = field.shape
    if not (0 <= gx < W and 0 <= gy < H) or not (0 <= sx < W and 0 <= sy < H):
        return 0, -1
    if (sx, sy) == (gx, gy):
        return 0, 0
    best = (0, -1)
    for code, dx, dy in DELTAS:
        nx, ny = sx + dx, sy + dy
        if 0 <= nx < W and 0 <= ny < H and field[nx, ny] >= 0 and (best[1] < 0 or field[nx, ny] + 1 < best[1]):
            best = (code, int(field[nx, ny]) + 1)
    return best


def host_navigate(dims, records, targets, walkable_blocks=False):
    """records uint32 [n][RW] (or one record), targets int [n][A][T][2] (or [A][T][2]) -> actions int32 [n][A][T], steps int32
    [n][A][T], field uint16 [n][A][T][W * H]"""
    recs = np.asarray(records, dtype=np.uint32)
    single = recs.ndim == 1
    recs = recs.reshape(-1, recs.shape[-1])
    tg = np.asarray(targets, dtype=np.int64)
    tg = tg.reshape((recs.shape[0], dims.A, -1, 2))
    n, A, T = tg.shape[:3]
    if not 1 <= T <= MAX_TARGETS:
        raise ValueError(f"T is {T}, not in 1..{MAX_TARGETS}")
    actions, steps = np.zeros((n, A, T), dtype=np.int32), np.zeros((n, A, T), dtype=np.int32)
    field = np.empty((n, A, T, dims.C), dtype=np.uint16)
    for i, rec in enumerate(recs):
        floor = floor_set(dims, rec, walkable_blocks)
        fields = {}
        for a in range(A):
            sx, sy, _o, _h = soa.unpack_agent(rec[soa.AGENT_WORD0 + a])
            for t in range(T):
                gx, gy = int(tg[i, a, t, 0]), int(tg[i, a, t, 1])
                if (gx, gy) not in fields:
                    fields[gx, gy] = flood(floor, gx, gy)
                f = fields[gx, gy]
                actions[i, a, t], steps[i, a, t] = first_move(f, sx, sy, gx, gy)
                field[i, a, t] = np.where(f < 0, UNREACHABLE, f).astype(np.uint16).reshape(-1)
    if single:
        return actions[0], steps[0], field[0]
    return actions, steps, field
