"""Level instantiation from keyed draws, host side: `load_level.instantiate` under `level_program.KeyedDraws` - the model of
cz_generate_layouts - against the layouts the unmodified reference parser (parsing.py:5-151) gives under the same stream
(tests/golden/layouts_keyed_ref.json), and the level-program compiler the device reads its levels from."""
import copy
import json

import numpy as np
import pytest

from cooking_zoo_amd import soa, spawn
from cooking_zoo_amd.cooking_world.engine import level_program as lp
from cooking_zoo_amd.cooking_world.engine import load_level as ll
from layout_keyed_common import CASES, CASE_IDS, assert_matches_reference, case_tables


def test_keyed_draws_are_the_spawn_stream():
    for seed, slot, gen in [(0, 0, 0), (3, 5, 1), ((1 << 64) - 1, 65534, (1 << 32) - 1), (12345678901234567, 77, 9)]:
        rng = lp.KeyedDraws(seed, slot, gen)
        for n in range(40):
            assert rng.random() == float(spawn.uniform(seed, slot, gen, lp.LAYOUT_TAG, n))
        u = float(spawn.uniform(seed, slot, gen, lp.LAYOUT_TAG, 40))
        assert rng.sample(list(range(100, 117)), 1) == [100 + int(u * 17)] and rng.n == 41
    assert not 0 <= lp.LAYOUT_TAG <= 3                                   # never an agent's despawn / respawn stream


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_model_matches_reference(case):
    level, meta, A, dims = case_tables(case)
    for ref in case["draws"]:
        lay, n = lp.keyed_layout(level, meta, A, dims, ref["seed"], ref["slot"], ref["generation"])
        assert lay is not None
        assert n == ref["n_draws"], "the model consumed a different number of draws than the reference"
        assert_matches_reference(lay, ref)


def test_fixture_covers_what_it_should():
    levels = {c["level"] for c in CASES}
    assert {"coop_test", "coexistence_test", "switch_test", "large_16x16", "crowded_6x5", "dense_8x8", "limit_32x8"} <= levels
    assert any("OPTIONAL" in json.dumps(ll.load_level_file(c["level"])) for c in CASES)
    assert any(case_tables(c)[3].huge for c in CASES)
    assert max(d["n_draws"] for c in CASES for d in c["draws"]) > 1000        # the rejection loops of a large level


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_level_program_round_trips(case):
    level, meta, A, dims = case_tables(case)
    prog = lp.compile_level(level, meta, A, dims)
    assert prog.dtype == np.uint32 and prog[lp.H_WORDS] == prog.size
    lev2, meta2, A2, dims2 = lp.decode_program(prog)
    assert lev2 == lp.normalize_level(level)
    assert list(meta2.items()) == list(meta.items()) and A2 == A and dims2 == dims.as_tuple()
    # ... and the decoded level instantiates to the same layouts
    for ref in case["draws"][:2]:
        a, na = lp.keyed_layout(level, meta, A, dims, ref["seed"], ref["slot"], ref["generation"])
        b, nb = lp.keyed_layout(lev2, meta2, A2, dims, ref["seed"], ref["slot"], ref["generation"])
        assert a.key() == b.key() and na == nb


def _coop():
    case = next(c for c in CASES if c["level"] == "coop_test" and c["num_agents"] == 2)
    level, meta, A, dims = case_tables(case)
    return copy.deepcopy(level), dict(meta), A, dims


def test_compiler_refuses_what_the_reference_raises_on():
    level, meta, A, dims = _coop()
    spec = list(level["STATIC_OBJECTS"][0].values())[0]
    for axis, lim in (("X_POSITION", dims.W), ("Y_POSITION", dims.H)):
        for bad in (-1, lim + 1):
            lv = copy.deepcopy(level)
            list(lv["STATIC_OBJECTS"][0].values())[0][axis] = spec[axis] + [bad]
            with pytest.raises(ValueError, match="out of bounds"):
                lp.compile_level(lv, meta, A, dims)
        # the far edge itself passes the reference's test (`>`, parsing.py:34): such a candidate only never fits
        lv = copy.deepcopy(level)
        list(lv["STATIC_OBJECTS"][0].values())[0][axis] = spec[axis] + [lim]
        lp.compile_level(lv, meta, A, dims)
        lay, _ = lp.keyed_layout(lv, meta, A, dims, 1, 0, 0)
        assert lay is not None
    for section, name in (("STATIC_OBJECTS", "Oven"), ("DYNAMIC_OBJECTS", "Pizza"), ("STATIC_OBJECTS", "Tomato"), ("DYNAMIC_OBJECTS", "Blender")):
        lv = copy.deepcopy(level)
        lv[section].append({name: {"COUNT": 1, "X_POSITION": [1], "Y_POSITION": [1]}})
        with pytest.raises(ValueError, match="unknown"):
            lp.compile_level(lv, meta, A, dims)
    lv = copy.deepcopy(level)
    lv["DYNAMIC_OBJECTS"].append({"Onion": {"COUNT": 1, "X_POSITION": [1], "Y_POSITION": [0]}})
    m2 = {k: v for k, v in meta.items() if k != "Onion"}
    with pytest.raises(ValueError):                                         # a class the meta file does not list (KeyError in the reference)
        lp.compile_level(lv, m2, A, soa.Dims(dims.W, dims.H, dims.D, A, lp.feature_length(m2)))
    with pytest.raises(ValueError, match="grid"):
        lp.compile_level(level, meta, A, soa.Dims(dims.W + 1, dims.H, dims.D, A, dims.F))


def failure_cases():
    """(name, level, meta, A, dims) whose every draw fails the way the reference raises"""
    level, meta, A, dims = _coop()
    out = []
    m0 = dict(meta)
    m0["Blender"] = 0                                                       # "Too many Blender objects loaded"
    out.append(("meta cap 0", level, m0, A, soa.Dims(dims.W, dims.H, dims.D, A, lp.feature_length(m0))))
    nofree = copy.deepcopy(level)                                           # no Counter anywhere: 10 001 tries, then ValueError
    nofree["LEVEL_LAYOUT"] = "\n".join(" " * dims.W for _ in range(dims.H))
    out.append(("no free Counter", nofree, meta, A, dims))
    case = next(c for c in CASES if c["level"] == "switch_test")
    lv, ms, As, ds = case_tables(case)
    lv = copy.deepcopy(lv)
    lv["STATIC_OBJECTS"].append({"Switch": {"COUNT": 1, "X_POSITION": [3], "Y_POSITION": [2]}})
    ms = dict(ms)
    ms["Switch"] = 2
    out.append(("second Switch", lv, ms, As, soa.Dims(ds.W, ds.H, ds.D, As, lp.feature_length(ms))))
    return out


@pytest.mark.parametrize("which", [0, 1, 2], ids=["meta-cap-0", "no-free-counter", "second-switch"])
def test_failed_draws_leave_the_slot_unchanged(which):
    name, level, meta, A, dims = failure_cases()[which]
    lp.compile_level(level, meta, A, dims)                                  # nothing a compiler could know
    lay, n = lp.keyed_layout(level, meta, A, dims, 5, 3, 1)
    assert lay is None, name
    if which == 1:
        assert n >= 2 * (lp.MAX_TRIES_OBJECT + 1)
    previous = ["held before"] * 4
    lays, failed = lp.keyed_layouts([level], meta, A, dims, [0] * 8, 5, 1, 2, 4, previous)
    assert failed == 4 and lays == previous


def test_more_slots_than_the_batch_has_is_a_failed_draw():
    level, meta, A, dims = _coop()
    small = soa.Dims(dims.W, dims.H, 4, A, dims.F)
    assert lp.keyed_layout(level, meta, A, small, 1, 0, 0)[0] is None
    assert lp.keyed_layout(level, meta, A, dims, 1, 0, 0)[0] is not None
