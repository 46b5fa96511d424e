"""The navigation call's definition on the host (cooking_zoo_amd/nav.py), no device: against what the unmodified reference's
`BaseAgent.walk_to_location` / `reachable` returned (tests/golden/nav_ref.json.gz, tools/gen_nav_golden.py), against a second
route that searches from the start the way the reference does, and the properties of the field."""
import numpy as np
import pytest

from cooking_zoo_amd import nav, soa
from grid_common import CASES, checkpoints
from nav_common import PADDING, all_cell_targets, draw_targets, golden, golden_answers, second_route

SMALL = [name for name, case in CASES.items() if case[5] == 0]


def all_goals(dims, rec, walkable_blocks=False):
    """(actions, steps) int32 [A][W][H] and field uint16 [A][W * H (goal)][W * H] of one record, every cell as the goal"""
    acts, steps, fields = [], [], []
    for tg, idx in all_cell_targets(dims, 1):
        a, s, f = nav.host_navigate(dims, rec, tg[0], walkable_blocks)
        keep = [k for k, i in enumerate(idx) if i >= 0]
        assert (a[:, len(keep):] == 0).all() and (s[:, len(keep):] == -1).all() and (f[:, len(keep):] == nav.UNREACHABLE).all(), "padding"
        acts.append(a[:, keep]), steps.append(s[:, keep]), fields.append(f[:, keep])
    shape = (dims.A, dims.W, dims.H)
    return np.concatenate(acts, 1).reshape(shape), np.concatenate(steps, 1).reshape(shape), np.concatenate(fields, 1)


def test_golden_answers_exact():
    """host_navigate of the stored record = what the reference returned, every stored state, agent and goal"""
    doc = golden()
    levels, n_states, codes, blocks = set(), 0, set(), set()
    for ep in doc["episodes"]:
        dims = soa.Dims(*ep["dims"])
        levels.add(ep["level"])
        for st in ep["states"]:
            rec = np.array(st["record"], dtype=np.uint32)
            want_act, want_reach = golden_answers(ep, st)
            act, steps, _f = all_goals(dims, rec)
            ctx = f"{ep['set']} seed {ep['seed']} step {st['step']}"
            bad = np.argwhere(act != want_act)
            assert not len(bad), f"{ctx}: actions differ at (agent, x, y) {bad[:6].tolist()}: {act[tuple(bad[0])]} for {want_act[tuple(bad[0])]}"
            bad = np.argwhere((steps >= 0) != want_reach)
            assert not len(bad), f"{ctx}: reachability differs at (agent, x, y) {bad[:6].tolist()}"
            codes |= set(np.unique(want_act).tolist())
            if ep["level"] == "switch_test":
                blocks.add(bool(st["open_blocks"]))
            n_states += 1
    assert levels == {"coop_test", "switch_test", "crowded_6x5", "dense_8x8"} and n_states >= 20
    assert codes == {0, 1, 2, 3, 4} and blocks == {False, True}


@pytest.mark.parametrize("name", list(CASES))
def test_second_route(name):
    """the flood fill from the goal against the queue search from the start over the Floor objects of the symbolic view: the same
    steps and actions, both flag values - every cell as the goal on the small levels, drawn targets on the others"""
    tables, points = checkpoints(name, 6)
    dims = tables.dims
    for k, recs in enumerate(points):
        for wb in (False, True):
            if name in SMALL:
                chunks = [tg for tg, _idx in all_cell_targets(dims, len(recs))] if k % 2 == int(wb) else []
            else:
                chunks = [draw_targets(dims, recs, 8, 100 + k)]
            for tg in chunks:
                act, steps, _f = nav.host_navigate(dims, recs, tg, wb)
                for e, rec in enumerate(recs):
                    a2, s2 = second_route(dims, tables.layouts[int(rec[soa.W_LAYOUT])], rec, tg[e], wb)
                    assert np.array_equal(act[e], a2) and np.array_equal(steps[e], s2), (
                        f"{name} checkpoint {k} env {e} walkable_blocks={wb}: targets {tg[e].tolist()}: host_navigate {act[e].tolist()} "
                        f"{steps[e].tolist()}, second route {a2.tolist()} {s2.tolist()}")


@pytest.mark.parametrize("name", ["coop_test", "switch_test", "dense_8x8"])
def test_field_properties(name):
    tables, points = checkpoints(name, 6)
    dims = tables.dims
    W, H = dims.W, dims.H
    rec = points[-1][2]
    floor = nav.floor_set(dims, rec)
    act, steps, field = all_goals(dims, rec)
    f = field.reshape(dims.A, W, H, W, H).astype(np.int64)                       # [agent][goal x][goal y][x][y]
    f[f == nav.UNREACHABLE] = -1
    assert np.array_equal(f[0], f[-1]), "the field depends on the goal and the cells alone"
    f = f[0]
    cells = [(x, y) for x in range(W) for y in range(H)]
    for g in cells:
        assert f[g][g] == 0
        for c in cells:
            if c != g and not floor[c]:
                assert f[g][c] == -1, f"goal {g}: the cell {c} is not Floor and has a distance"
            if floor[c] and floor[g]:
                assert f[g][c] == f[c][g], f"field of {g} at {c} is {f[g][c]}, field of {c} at {g} is {f[c][g]}"
            for _code, dx, dy in nav.DELTAS:
                n = (c[0] + dx, c[1] + dy)
                if 0 <= n[0] < W and 0 <= n[1] < H and floor[c] and floor[n]:
                    assert (f[g][c] < 0) == (f[g][n] < 0) and abs(f[g][c] - f[g][n]) <= 1, f"goal {g}: neighbours {c} and {n}"
    for a in range(dims.A):
        sx, sy, _o, _h = soa.unpack_agent(rec[soa.AGENT_WORD0 + a])
        for g in cells:
            near = [int(f[g][sx + dx, sy + dy]) for _c, dx, dy in nav.DELTAS if 0 <= sx + dx < W and 0 <= sy + dy < H]
            finite = [v for v in near if v >= 0]
            if g == (sx, sy):
                assert (act[a][g], steps[a][g]) == (0, 0)
            else:
                assert (steps[a][g] == -1) == (not finite), f"agent {a} at {(sx, sy)}, goal {g}: steps {steps[a][g]}, neighbours {near}"
                assert steps[a][g] == (min(finite) + 1 if finite else -1) and (act[a][g] == 0) == (not finite)
    assert (steps == -1).any() and (steps > 0).any()


def test_padding_and_off_grid_targets():
    tables, points = checkpoints("crowded_6x5", 6)
    dims = tables.dims
    recs = points[0]
    off = [PADDING, (dims.W, 0), (0, dims.H), (-1, 0), (0, -1), (dims.W + 250, 3), (2 ** 31 - 1, -2 ** 31), (256, 256)]
    tg = np.broadcast_to(np.array(off, dtype=np.int64), (len(recs), dims.A, 8, 2))
    act, steps, field = nav.host_navigate(dims, recs, tg)
    assert act.shape == steps.shape == (6, dims.A, 8) and field.shape == (6, dims.A, 8, dims.C)
    assert act.dtype == steps.dtype == np.int32 and field.dtype == np.uint16
    assert (act == 0).all() and (steps == -1).all() and (field == nav.UNREACHABLE).all()
    a1, s1, f1 = nav.host_navigate(dims, recs[0], tg[0])                        # one record
    assert a1.shape == (dims.A, 8) and f1.shape == (dims.A, 8, dims.C)
    for bad_T in (0, 9):
        with pytest.raises(ValueError):
            nav.host_navigate(dims, recs, np.zeros((len(recs), dims.A, bad_T, 2), np.int64))


def test_walkable_blocks_change_results_only_while_the_block_is_open():
    tables, points = checkpoints("switch_test", 6, points=8)
    dims = tables.dims
    seen = set()
    for recs in points:
        for rec in recs:
            cells = soa.record_cells(dims, rec)
            is_open = bool((((cells & soa.CELL_TYPE_MASK) == soa.STATIC_CLASSES.index("Block")) & ((cells & soa.CELL_WALK) != 0)).any())
            plain, wide = all_goals(dims, rec), all_goals(dims, rec, True)
            same = all(np.array_equal(p, w) for p, w in zip(plain, wide))
            assert is_open or same, "walkable_blocks changed a result while every Block is closed"
            assert same != is_open, "an open Block changes no result on switch_test"
            seen.add(is_open)
    assert seen == {False, True}, "the checkpoints do not show the Block both closed and open"
    for name in ("coop_test", "dense_8x8"):                                      # no Block: nothing changes
        t2, p2 = checkpoints(name, 6)
        assert all(np.array_equal(p, w) for p, w in zip(all_goals(t2.dims, p2[-1][0]), all_goals(t2.dims, p2[-1][0], True)))
