"""GPU: k_generate_layouts (csrc/cz_generate.h) on every shipped level at every agent count and on every branch that refuses a draw.

tests/test_gpu_layout_generate.py redraws a few slots of ten levels and reads them back through reset / cz_get_state / cz_observe,
where a descriptor word that points at the wrong halfword of the image can encode the same float on a fresh world.  Here every case
of tests/golden/layouts_keyed_stress_ref.json.gz - the 15 shipped levels at 1 .. Agent-count agents and the six stress levels of
tests/levels/, one per way a draw can fail - redraws the middle half of a prefilled pool, once per generation, and reads BOTH pool
tables back as the device holds them (cz_diag_read_layout_pool): every slot of the range must equal Layout.init_record /
obs_descriptor of the host model byte for byte, a slot whose draw failed and every slot outside the range what it held before, and
cz_generate_failures the model's count.  The model itself is pinned to the unmodified reference parser by that fixture
(tests/test_layout_keyed.py); the fixture's keys lie inside the ranges drawn here and are compared once more on the way.

A failed draw costs the host model 10 001 attempts in Python, so the model's draws are computed once per (level, meta, agents,
key) and shared by the tests that need them; nothing of them is changed afterwards.

Vacuity: FLOORS holds, per case, what the HOST MODEL ALONE must have gone through in the slots drawn - failed and successful
draws of the level's failure kind in the same launches, layouts with a rejection streak of at least 64 and of at least 128 (the
second and third round of the kernel's 64-attempt loop), positions drawn on the far edge, static objects their OPTIONAL test left
out.  Each floor is about half of what the model gives under SEED (profiles/r17/README.md has the measured values)."""
import ctypes as C
import faulthandler
import random

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from cooking_zoo_amd.cooking_world.engine import level_program as lp
from cooking_zoo_amd.cooking_world.engine import load_level as ll
from layout_keyed_common import (FOUR, KINDS, SHIPPED, STRESS, STRESS_CASES, STRESS_IDS, assert_matches_reference, case_files, case_tables,
                                 failure_kind, host_update, read_pool, reference_misfit)
from vec_common import bits

pytestmark = pytest.mark.gpu

SEED = 1717                                    # tools/gen_golden.py STRESS_SEED: the fixture's keys are among the slots drawn here
SAMPLE = 32                                    # slots read back through reset + cz_observe as well, next to a twin env


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after five minutes, also when it hangs inside a HIP call"""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def prefilled(n, level, meta, agents, *, pool, max_dyn=None):
    """test_gpu_layout_generate.prefilled - a batch whose whole pool holds ONE fixed, valid, recognisable layout per level, the
    host loader's draw under Random(99) - for levels whose draw can fail as well: the first draw of that stream that succeeds,
    fits the batch and has one Switch at the most (that module's helper would raise on stress_agent_timeout with 3 agents)"""
    from cooking_zoo_amd.vec_env import CookingVecEnv
    levels = [level] if isinstance(level, str) else list(level)
    m = ll.load_meta_file(meta)
    fixed = []
    for name in levels:
        lv, rng = ll.load_level_file(name), random.Random(99)
        D = max_dyn or max(ll.level_max_dyn(ll.load_level_file(l)) for l in levels)
        for _ in range(100):
            try:
                lay = ll.instantiate(lv, m, agents, rng)
                lay.obs_descriptor(m, soa.Dims(lay.width, lay.height, D, agents, lp.feature_length(m)))
                if lay.slots_used <= D:
                    break
            except ValueError:
                continue
        fixed.append([lay] * pool)
    return CookingVecEnv(n, level, meta, agents, 30, FOUR[:max(agents, 1)], action_scheme="scheme3", layouts=fixed, max_dyn=max_dyn,
                         auto_reset=True)


# ------------------------------------------------------------------------------------------------ the host model, computed once
_DRAWS = {}


def model_draw(level_file, meta_file, level, meta, A, seed, slot, generation):
    """-> (Layout or None, the ValueError's message or None, stats of load_level.instantiate): one keyed draw of the host model
    before the batch's own limits (slots, Counter features) are applied.  Shared; never modified."""
    key = (level_file, meta_file, A, seed, slot, generation)
    if key not in _DRAWS:
        stats = {}
        try:
            _DRAWS[key] = (ll.instantiate(level, meta, A, lp.KeyedDraws(seed, slot, generation), stats), None, stats)
        except ValueError as exc:
            _DRAWS[key] = (None, str(exc), stats)
    return _DRAWS[key]


def model_rows(lay, meta, dims, slot):
    """-> (init record, descriptor, None) or (None, None, message): what enters a batch of `dims`"""
    try:
        return lay.init_record(dims, slot), lay.obs_descriptor(meta, dims), None
    except ValueError as exc:
        return None, None, str(exc)


def pool_shape(dims):
    """-> (pool slots, generations, first, count): 256 slots and 3 generations, 128 and 2 from 16 x 16 cells upwards (the host
    model takes 2 - 4 ms per layout there); the middle half is drawn"""
    L, gens = (128, (1, 2)) if dims.W >= 16 and dims.H >= 16 else (256, (1, 2, 3))
    return L, gens, L // 4, L // 2


def read_tables(env, first, count):
    """rows [first, first + count) of the pool's two tables as the device holds them"""
    L = _native.lib()
    L.cz_diag_read_layout_pool.restype = C.c_int
    L.cz_diag_read_layout_pool.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    recs = np.zeros((count, env.dims.RW), dtype=np.uint32)
    desc = np.zeros((count, env.dims.F), dtype=np.uint32)
    _native.check(env._h, L.cz_diag_read_layout_pool(env._h, first, count, recs.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p)))
    return recs, desc


def assert_rows(got, want, what, first, count):
    if not np.array_equal(got, want):
        s = int(np.nonzero((got != want).any(axis=1))[0][0])
        w = int(np.nonzero(got[s] != want[s])[0][0])
        where = "inside" if first <= s < first + count else "OUTSIDE"
        raise AssertionError(f"{what} of slot {s} ({where} the range drawn) differs from word {w} on: {got[s, w]:#x}, expected {want[s, w]:#x}")


def new_coverage():
    return {"failed": {k: 0 for k in KINDS}, "ok": 0, "streak64": 0, "streak128": 0, "far_edge": 0, "static_optional_stops": 0}


def expect_generation(files, levels, meta, A, dims, level_of_slot, generation, first, count, recs, desc, lays, cov, failed_slots=None):
    """apply the host model's draws of slots [first, first + count) under (SEED, generation) to the expected tables and layouts"""
    failed = 0
    for s in range(first, first + count):
        li = int(level_of_slot[s])
        lay, msg, stats = model_draw(files[li][0], files[li][1], levels[li], meta, A, SEED, s, generation)
        cov["streak64"] += stats["max_streak"] >= 64
        cov["streak128"] += stats["max_streak"] >= 128
        cov["far_edge"] += stats["far_edge"]
        cov["static_optional_stops"] += stats["static_optional_stops"]
        r = d = None
        if lay is not None:
            r, d, msg = model_rows(lay, meta, dims, s)
        if msg is not None:
            cov["failed"][failure_kind(msg)] += 1
            failed += 1
            if failed_slots is not None:
                failed_slots.append(s)
            continue                                                        # a failed draw: the slot keeps what it held
        cov["ok"] += 1
        recs[s], desc[s], lays[s] = r, d, lay
    return failed


# ------------------------------------------------------------------------------------------------ floors (host model alone)
# (level, agents) -> conditions on the coverage of the slots drawn; "kinds": failure kind -> floors of (failed, successful) draws.
# Cases not listed must not fail at all.  Values: profiles/r17/README.md.
FLOORS = {}
for _level, _agents, _floors in [
        ("dense_8x8", 4, {"streak64": 100, "streak128": 30}),
        ("large_16x16", 4, {"streak64": 20, "streak128": 1}),
        ("huge_objs_16x16", 3, {"streak64": 22, "streak128": 1}),
        ("coexistence_test", 2, {"static_optional_stops": 160}),
        ("stress_object_timeout", 3, {"kinds": {"object time-out": (35, 150)}, "streak64": 35, "streak128": 35, "far_edge": 100000,
                                      "static_optional_stops": 110}),
        ("stress_agent_timeout", 2, {"far_edge": 400, "static_optional_stops": 100}),
        ("stress_second_switch", 3, {"kinds": {"second Switch": (40, 150)}, "static_optional_stops": 150}),
        ("stress_counter_overflow", 3, {"kinds": {"Counter overflow": (60, 130)}, "far_edge": 70, "static_optional_stops": 150}),
        ("stress_slots", 3, {"kinds": {"slots": (45, 140)}}),
        ("stress_meta_cap", 3, {"kinds": {"meta cap": (50, 140)}, "far_edge": 100, "static_optional_stops": 190})]:
    for _a in range(1, _agents + 1):
        FLOORS[_level, _a] = _floors
# the third agent's only Floor candidate is one the first two may stand on: no failure at 1 or 2 agents, half of the draws at 3
FLOORS["stress_agent_timeout", 3] = {"kinds": {"agent time-out": (100, 90)}, "streak64": 100, "streak128": 100, "far_edge": 75000,
                                     "static_optional_stops": 100}


def floors_of(case):
    return FLOORS.get((case["level"], case["num_agents"]), {})


def assert_floors(case, cov, padded=False):
    fl = floors_of(case)
    allowed = set(fl.get("kinds", {}))
    for kind, n in cov["failed"].items():
        assert n == 0 or kind in allowed, f"{n} draws failed by {kind!r}, which this case does not provide for"
    for kind, (n_failed, n_ok) in fl.get("kinds", {}).items():
        if padded and kind == "slots":
            assert cov["failed"][kind] == 0                               # (the padded record has room for every loaf)
            continue
        assert cov["failed"][kind] >= n_failed, f"vacuous: {cov['failed'][kind]} draws failed by {kind!r}, floor {n_failed}"
        assert cov["ok"] >= n_ok, f"vacuous: {cov['ok']} draws succeeded next to them, floor {n_ok}"
    for name in ("streak64", "streak128", "far_edge", "static_optional_stops"):
        assert cov[name] >= fl.get(name, 0), f"vacuous: {name} {cov[name]}, floor {fl[name]}"


def run_case(case, max_dyn=None, instance=None):
    level, meta, A, dims = case_tables(case, max_dyn)
    files = [case_files(case)]
    L, gens, first, count = pool_shape(dims)
    pad = dims.D if (max_dyn or case.get("max_dyn")) else None
    env = prefilled(SAMPLE, files[0][0], files[0][1], A, pool=L, max_dyn=pad)
    twin = prefilled(SAMPLE, files[0][0], files[0][1], A, pool=L, max_dyn=pad)
    assert env.dims.as_tuple() == dims.as_tuple()
    if instance is not None:
        assert _native.lib().cz_diag_instance(env._h) == instance
    recs, desc = read_tables(env, 0, L)
    assert np.array_equal(recs, env._lay_records) and np.array_equal(desc, env._lay_desc), "the read-back of the prefill"
    lays = list(env.layouts)
    los = np.zeros(L, dtype=np.uint8)
    cov, failed = new_coverage(), 0
    for g in gens:
        env.generate_layouts(first, count, g, seed=SEED, mirror=False)
        failed += expect_generation(files, [level], meta, A, dims, los, g, first, count, recs, desc, lays, cov)
        got_recs, got_desc = read_tables(env, 0, L)
        assert_rows(got_recs, recs, f"generation {g}: record", first, count)
        assert_rows(got_desc, desc, f"generation {g}: descriptor", first, count)
        assert env.generate_failures() == failed
    assert_floors(case, cov, padded=max_dyn is not None)
    assert sum(l is not lays[0] for l in lays) >= count // 2, "the generated part must differ from the prefill"
    # the fixture's keys that lie in the range drawn: the model the device was held against is the reference's draw
    for ref in case["draws"]:
        if ref["seed"] == SEED and ref["generation"] in gens and first <= ref["slot"] < first + count:
            lay, msg, _ = model_draw(files[0][0], files[0][1], level, meta, A, SEED, ref["slot"], ref["generation"])
            if "raises" in ref:
                assert lay is None and failure_kind(msg) == failure_kind(ref["message"])
            elif lay is None:
                assert failure_kind(msg) == reference_misfit(ref, meta, dims) == "second Switch"
            else:
                assert_matches_reference(lay, ref)
    # the old read path, on a sample: reset + cz_get_state + cz_observe next to a twin fed over cz_update_layouts
    slots = np.arange(first, first + SAMPLE)
    host_update(twin, first, lays[first:first + SAMPLE])
    rg, og = read_pool(env, slots)
    rt, ot = read_pool(twin, slots)
    assert np.array_equal(rg, rt) and np.array_equal(bits(og), bits(ot)), "records / observations of the sample"
    env.resolve_layouts()
    assert [l.key() for l in env.layouts] == [l.key() for l in lays]
    env.close(); twin.close()
    return cov


@pytest.mark.parametrize("case", STRESS_CASES, ids=STRESS_IDS)
def test_every_slot_drawn_equals_the_model_in_both_tables(case):
    run_case(case)


STRESS_A3 = [c for c in STRESS_CASES if c["stress"] and c["num_agents"] == 3]


@pytest.mark.parametrize("max_dyn,instance", [(65, 1), (129, 2)])
@pytest.mark.parametrize("case", STRESS_A3, ids=[c["level"] for c in STRESS_A3])
def test_stress_levels_padded_onto_the_larger_instances(case, max_dyn, instance):
    """the record is longer and the huge instance keeps another LDS image, so the descriptor's halfword bases differ"""
    run_case(case, max_dyn, instance)


def test_mixed_batch_fails_only_in_the_failing_levels_slice():
    """two levels that never fail around one whose second, OPTIONAL Switch refuses a quarter of its draws: one launch per generation
    over the middle of the pool, which cuts through all three slices"""
    stress = next(c for c in STRESS_CASES if c["level"] == "stress_second_switch")
    files = [("coop_test", "example"), (case_files(stress)[0], "example"), ("coexistence_test", "example")]
    names = [f[0] for f in files]
    n_slice, A = 64, 2
    env = prefilled(SAMPLE, names, "example", A, pool=n_slice)
    twin = prefilled(SAMPLE, names, "example", A, pool=n_slice)
    assert env.pool_slices == [(0, 64), (64, 64), (128, 64)]
    L, first, count = 3 * n_slice, 24, 144
    los, levels, meta, dims = env.level_of_slot(), env.level_objects, env.meta, env.dims
    recs, desc = read_tables(env, 0, L)
    assert np.array_equal(recs, env._lay_records) and np.array_equal(desc, env._lay_desc)
    lays, cov, failed, failed_slots = list(env.layouts), new_coverage(), 0, []
    for g in (1, 2, 3):
        env.generate_layouts(first, count, g, seed=SEED, mirror=False)
        failed += expect_generation(files, levels, meta, A, dims, los, g, first, count, recs, desc, lays, cov, failed_slots)
        got_recs, got_desc = read_tables(env, 0, L)
        assert_rows(got_recs, recs, f"generation {g}: record", first, count)
        assert_rows(got_desc, desc, f"generation {g}: descriptor", first, count)
        assert env.generate_failures() == failed
    assert all(64 <= s < 128 for s in failed_slots)
    assert cov["failed"] == {**{k: 0 for k in KINDS}, "second Switch": failed}
    assert failed >= MIXED_FLOOR[0] and 3 * n_slice - failed >= MIXED_FLOOR[1], f"vacuous: {failed} draws of the middle slice failed"
    slots = np.concatenate([np.arange(56, 72), np.arange(120, 136)])          # both borders between slices
    host_update(twin, 56, lays[56:72])
    host_update(twin, 120, lays[120:136])
    rg, og = read_pool(env, slots)
    rt, ot = read_pool(twin, slots)
    assert np.array_equal(rg, rt) and np.array_equal(bits(og), bits(ot))
    env.close(); twin.close()


MIXED_FLOOR = (17, 78)                                                     # (failed, successful) draws of the middle slice


def test_zz_the_floors_cover_every_level_agent_count_and_failure_kind():
    """the coverage table the cases above assert: every case of the fixture is one of them, every shipped level at every agent
    count, every stress level at 1 .. 3 agents, and each of the six failure kinds with floors above zero on both sides"""
    cases = {(c["level"], c["num_agents"]) for c in STRESS_CASES}
    assert cases == {(l, a) for l, n in SHIPPED.items() for a in range(1, n + 1)} | {(l, a) for l in STRESS for a in (1, 2, 3)}
    assert set(FLOORS) <= cases
    mixed = {k for fl in FLOORS.values() for k, (nf, nk) in fl.get("kinds", {}).items() if nf > 0 and nk > 0}
    assert mixed == set(KINDS), mixed
    for name in ("streak64", "streak128", "far_edge", "static_optional_stops"):
        assert sum(fl.get(name, 0) > 0 for fl in FLOORS.values()) >= 3, name
    assert min(MIXED_FLOOR) > 0
