"""The grid observation's definition on the host (cooking_zoo_amd/grid.py), no device: against words computed from the
unmodified reference's live objects (tests/golden/grid_ref.json.gz, tools/gen_grid_golden.py), against its own expansion, and
against a second route over `symbolic.materialize`'s object view on oracle trajectories - with a coverage condition over all
of this module's states."""
import glob
import gzip
import json
import os

import numpy as np
import pytest

from cooking_zoo_amd import grid, soa
from cooking_zoo_amd.cooking_world import symbolic
from grid_common import CASES, Coverage, checkpoints, view_bits

HERE = os.path.dirname(os.path.abspath(__file__))
LEVEL_DIR = os.path.join(os.path.dirname(HERE), "cooking_zoo_amd", "utils", "level")
# the oracle trajectories of this module: (case, envs, despawn / respawn on)
RUNS = [("coop_test", 6, True), ("crowded_6x5", 6, True), ("switch_test", 6, False), ("dense_16x16", 4, False), ("large_16x16", 4, False),
        ("limit_8x31", 3, False)]
# Channels no state can set, by the definition itself: the reference's Bread vector is the literal (1, 0, 0) (world_objects.py:747-748)
CONSTANT_ZERO = ["Bread.zero1", "Bread.zero2"]
# Channels of classes that occur in no level file of the repository: none - every class of the reference does
ABSENT_CLASS_CHANNELS = []


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(HERE, "golden", "grid_ref.json.gz")) as f:
        return json.load(f)


def test_class_table(golden):
    table = [tuple(t) for t in golden["class_table"]]
    assert [n for n, _ in table] == grid.REF_CLASSES
    assert dict(table) == symbolic.STATE_LENGTH
    off = 0
    for name, n in table:
        assert grid.CLASS_OFFSET[name] == off
        assert [c.split(".")[0] for c in grid.REF_CHANNELS[off:off + n]] == [name] * n
        off += n
    assert off == len(grid.REF_CHANNELS) == 32 == symbolic.GRAPH_REPRESENTATION_LENGTH
    assert golden["channels"] == grid.channels(True) and len(grid.channels(True)) == 48 and grid.channels(False) == grid.REF_CHANNELS
    assert len(set(grid.channels(True))) == 48


def test_golden_words_exact(golden):
    """host_bits of the stored record = the words the reference's live objects gave, every stored state, as integers"""
    levels, n_states = set(), 0
    for ep in golden["episodes"]:
        dims = soa.Dims(*ep["dims"])
        levels.add((ep["level"], ep["scheme"]))
        for st in ep["states"]:
            rec = np.array(st["record"], dtype=np.uint32)
            want = np.array(st["bits"], dtype=np.uint32).reshape(dims.W, dims.H, 2)
            got = grid.host_bits(dims, rec, extended=True)
            bad = np.argwhere(got != want)
            assert not len(bad), f"{ep['set']} seed {ep['seed']} step {st['step']}: words differ at (x, y, word) {bad[:6].tolist()}"
            assert np.array_equal(grid.host_bits(dims, rec), want[..., :1])
            n_states += 1
    assert n_states >= 24
    assert ("crowded_6x5", "scheme3") in levels and ("switch_test", "scheme1") in levels        # non-square; scheme1 with Switch and Block
    ones = Coverage()
    for ep in golden["episodes"]:
        for st in ep["states"]:
            ones.add(st["bits"])
    missing = ones.never(1)
    assert "object.in_plate" not in missing and "Banana.mashed" not in missing and "agent.despawned" in missing, missing


def test_expand_bit_by_bit():
    tables, recs = checkpoints("crowded_6x5", 6, True)
    for extended in (False, True):
        bits = grid.host_bits(tables.dims, recs[-1], extended)
        C = 48 if extended else 32
        assert bits.shape == (6, tables.dims.W, tables.dims.H, (C + 31) // 32) and bits.dtype == np.uint32
        for dtype in (np.uint8, np.float32):
            g = grid.expand(bits, dtype)
            assert g.shape == bits.shape[:-1] + (C,) and g.dtype == dtype and g.flags.c_contiguous
            for c in range(C):
                assert np.array_equal(g[..., c] != 0, (bits[..., c >> 5] >> np.uint32(c & 31)) & 1 != 0), f"channel {c}"
            assert set(np.unique(g).tolist()) <= {0, 1}
    assert not (grid.host_bits(tables.dims, recs[-1], True)[..., 1] >> 16).any(), "bits of the second word behind channel 47"
    assert grid.agent_xy(tables.dims, recs[-1]).shape == (6, 4, 2)


def level_classes(levels=None):
    """class names that occur in the level files (all of the repository's, or the named ones): objects by name, Floor and
    Counter as the map's own characters, and the agents"""
    paths = glob.glob(os.path.join(LEVEL_DIR, "*.json")) if levels is None else [os.path.join(LEVEL_DIR, l + ".json") for l in levels]
    names = {"Agent"}
    for path in paths:
        text = open(path).read()
        names |= {n for n in symbolic.STATE_LENGTH if f'"{n}"' in text}
        rows = json.loads(text)["LEVEL_LAYOUT"]
        names |= {n for ch, n in (("-", "Counter"), (" ", "Floor")) if ch in rows}
    return names


def test_second_route_and_coverage(golden):
    cov = Coverage()
    for ep in golden["episodes"]:
        for st in ep["states"]:
            cov.add(st["bits"])
    oracle = Coverage()
    for name, n, spawn in RUNS:
        tables, points = checkpoints(name, n, spawn, points=8)
        dims = tables.dims
        for recs in points:
            got = grid.host_bits(dims, recs, extended=True)
            for e, rec in enumerate(recs):
                want = view_bits(dims, tables.layouts[int(rec[soa.W_LAYOUT])], rec)
                bad = np.argwhere(got[e] != want)
                assert not len(bad), f"{name} env {e}: host_bits and the object view differ at (x, y, word) {bad[:6].tolist()}"
            oracle.add(got)
            assert np.array_equal(grid.agent_xy(dims, recs)[..., 0], recs[:, soa.AGENT_WORD0:soa.AGENT_WORD0 + dims.A] & 0xFF)
    cov.ones |= oracle.ones
    cov.zeros |= oracle.zeros
    present = level_classes()
    for ch in ABSENT_CLASS_CHANNELS:
        assert ch.split(".")[0] not in present, f"{ch}: its class occurs in a level file"
    allowed = set(ABSENT_CLASS_CHANNELS) | set(CONSTANT_ZERO)
    # the oracle's trajectories alone meet the condition
    assert set(oracle.never(1)) <= allowed, f"channels never set on the oracle's states: {sorted(set(oracle.never(1)) - allowed)}"
    assert not oracle.never(0), f"channels never clear: {oracle.never(0)}"
    assert set(cov.never(1)) == set(CONSTANT_ZERO) | set(ABSENT_CLASS_CHANNELS)
    used = level_classes([CASES[name][0] for name, _n, _s in RUNS])
    assert not [ch for ch in ABSENT_CLASS_CHANNELS if ch.split(".")[0] in used]
