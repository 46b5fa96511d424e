"""GPU: reset() of chosen envs on the device (cz_reset_device / CookingVecEnv.reset_device; cooking_env.py:178-210, rows :271,352-373).
Everything is compared exactly: records as bytes (running-return words stripped), float64 rows as uint64, float32 rows as uint32
against np.float32 of the oracle's rows, codes decoded through obs_table().  Every output buffer is pre-filled with a sentinel and the
float32 buffer is guarded.  What a chosen env must become comes from the oracle alone, in one of two ways: episode word + 1,
czo_next_layout_group, czo_reset_env (`oracle_reset`), or the reset pass of an auto_reset = 1 oracle's czo_step_env on a record whose
done bit is set (`oracle_reset_pass`)."""
import ctypes as C
import functools

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from fuzz_policy import BumperActions
from oracle_binding import VecOracle
from vec_common import (ALL_FORMS, COOP, FORM_SUBSETS, INSTANCE_CASES, SENT8, SENT64, SENTINEL, TWO, Bufs, CallerStream, check_rows, env_of,
                        instance, oracle_reset, strip, tables_of, want32)

pytestmark = pytest.mark.gpu

SEED = 3                            # the mixed run's seed: `sensitive` holds for it on the oracle alone


def make(n, auto_reset=False, tables=None, **cfg):
    return env_of(tables or tables_of(n, **cfg), auto_reset)


def oracle_reset_pass(orc, auto, e):
    """the second way: the done bit set on the record, and an auto_reset = 1 oracle's step does its reset pass on it"""
    rec = orc.records[e]
    rec[soa.W_STATUS] |= 1
    err, obs, rew, term, trunc = auto.oracle.step_env(rec, np.zeros(orc.dims.A, dtype=np.int32), env_local=e)
    assert err == 0 and not rew.any() and not term.any() and not trunc.any()
    return obs


class Script:
    """A run on the oracle alone (no device): per step the actions, the mask of the reset call behind the step, the explicit layout
    ids (or None), the records after the step and after the reset, and the float64 rows of every env that restarted."""

    def __init__(self, tables, steps, seed, p_chosen=0.1, p_done=None, null_mask=False, explicit=False, groups=(1, 0), way=1):
        n, L = tables.num_envs, len(tables.layouts)
        self.null_mask = null_mask
        self.orc = orc = VecOracle.from_vec_env(tables, auto_reset=0)
        auto = VecOracle.from_vec_env(tables, auto_reset=1)
        for o in (orc, auto):
            o.set_layout_group(*groups)
        self.obs0 = orc.reset()
        self.rec0 = orc.records.copy()
        pol = BumperActions(tables.dims, tables.scheme_class.CODE, np.random.default_rng(seed))
        rng = np.random.default_rng(seed + 1000)
        self.steps = []
        self.count = dict(chosen_done=0, chosen_live=0, unchosen_done=0, unchosen_live=0, refused=0, finished=0)
        for t in range(steps):
            acts = pol.act(orc.records)
            before = (orc.records[:, soa.W_STATUS] & 1) != 0
            obs, rew, term, trunc = orc.step(acts)
            pol.observe_result(orc.records)
            done = (orc.records[:, soa.W_STATUS] & 1) != 0
            self.count["finished"] += int((done & ~before).sum())
            stepped = orc.records.copy()
            # (a mask byte counts when it is not 0: any value; finished envs may be chosen at a rate of their own, so that both kinds turn up)
            p = np.where(done, p_chosen if p_done is None else p_done, p_chosen)
            mask = done.astype(np.uint8) if null_mask else (rng.random(n) < p).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
            ids = None
            if explicit:      # valid ids of the whole pool (outside the env's slice too), -1 = the keyed draw, L and L + 7 = refused
                ids = rng.choice(np.array(list(range(L)) + [-1, -1, -5, L, L + 7], dtype=np.int32), size=n).astype(np.int32)
            chosen = mask != 0
            refused = chosen & (ids >= L) if explicit else np.zeros(n, dtype=bool)
            self.count["chosen_done"] += int((chosen & done).sum()); self.count["chosen_live"] += int((chosen & ~done).sum())
            self.count["unchosen_done"] += int((~chosen & done).sum()); self.count["unchosen_live"] += int((~chosen & ~done).sum())
            self.count["refused"] += int(refused.sum())
            rows = {}
            for e in np.nonzero(chosen & ~refused)[0]:
                lay = int(ids[e]) if explicit and ids[e] >= 0 else -1
                if way == 2 and lay < 0:
                    rows[int(e)] = oracle_reset_pass(orc, auto, int(e))
                else:
                    rows[int(e)] = oracle_reset(orc, int(e), lay, *groups)
            self.steps.append(dict(acts=acts, obs=obs, mask=mask, ids=ids, stepped=stepped, rows=rows, refused=refused, after=orc.records.copy()))

    def sensitive(self, n):
        return all(self.count[k] >= n for k in ("chosen_done", "chosen_live", "unchosen_done", "unchosen_live"))


@functools.lru_cache(maxsize=None)
def coop_script(kind):
    """the scripts of the coop_test runs, made once and shared (read-only) by the tests that replay them"""
    t = tables_of(37, **COOP)
    if kind == "mixed":
        return Script(t, 40, SEED, p_chosen=0.08, p_done=0.25)
    if kind == "null":
        return Script(t, 40, SEED, null_mask=True, way=2)
    if kind == "explicit":
        return Script(t, 16, SEED, p_chosen=0.6, explicit=True)
    raise KeyError(kind)


def replay(env, script, forms=ALL_FORMS, prepare=None, calls=None):
    """the script on the device: step (float64 rows for everyone; codes and float32 rows keep their sentinel), then reset_device.
    `calls`: the steps whose reset call is made, a range - the steps in front of it must choose nobody, those behind it are left out"""
    b = Bufs(env)
    env.reset(return_obs=False)
    assert np.array_equal(strip(env.get_state()), script.rec0)
    if prepare:
        prepare()
    for t, s in enumerate(script.steps if calls is None else script.steps[:calls[-1] + 1]):
        b.fill()
        b.act.from_host(s["acts"])
        env.step_device(b.act, b.obs, b.rew, b.term, b.trunc)
        if calls is not None and t not in calls:
            assert not s["mask"].any() and not script.null_mask      # (without its call the records are still the script's)
            continue
        b.mask.from_host(s["mask"])
        if s["ids"] is not None:
            b.ids.from_host(s["ids"])
        before = b.read()
        assert np.array_equal(before[0], s["obs"].view(np.uint64)), f"step {t}: the step's own rows"
        assert np.array_equal(strip(env.get_state()), s["stepped"]), f"step {t}: records after the step"
        env.reset_device(None if script.null_mask else b.mask, b.ids if s["ids"] is not None else None,
                         b.obs if "obs" in forms else None, b.rows32.buf if "obs32" in forms else None, b.codes if "codes" in forms else None)
        check_rows(f"call {t}", env, before, b.read(), s["rows"], forms)
        assert np.array_equal(strip(env.get_state()), s["after"]), f"call {t}: records"
    return b


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2, 3: the coop_test runs
# ---------------------------------------------------------------------------------------------------------------------------

def test_mixed_run_all_three_forms():
    s = coop_script("mixed")
    assert s.sensitive(37), s.count                 # (the oracle alone: each of the four kinds of env at least N times)
    env = make(37, **COOP)
    replay(env, s)
    assert env.reset_device_refused() == 0
    env.close()


MIXED_CALLS = range(1, 25)          # the mixed script's calls 1..24: in each of them somebody is chosen (call 0 chooses nobody)


@pytest.mark.parametrize("forms", FORM_SUBSETS, ids="+".join)
def test_every_subset_of_forms(forms):
    """k_reset_where's rows come from one writer shared with the other off-step kernels: each form alone, each pair - float32 rows
    from the image observe built, the float64 table staged or not - and all three; a buffer the call does not name keeps its sentinel"""
    s = coop_script("mixed")
    kinds = np.zeros(4, dtype=int)                  # (the oracle alone) per call somebody chosen and somebody left alone ...
    for t in MIXED_CALLS:
        chosen, done = s.steps[t]["mask"] != 0, (s.steps[t]["stepped"][:, soa.W_STATUS] & 1) != 0
        assert chosen.any() and not chosen.all() and sorted(s.steps[t]["rows"]) == np.nonzero(chosen)[0].tolist(), t
        kinds += [(chosen & done).sum(), (chosen & ~done).sum(), (~chosen & done).sum(), (~chosen & ~done).sum()]
    assert (kinds >= 20).all(), kinds               # ... and over the calls each of the four kinds of env, often
    env = make(37, **COOP)
    replay(env, s, forms, calls=MIXED_CALLS)
    assert env.reset_device_refused() == 0
    env.close()


def test_null_mask_resets_exactly_the_done_envs():
    s = coop_script("null")
    assert s.count["chosen_done"] >= 37 and s.count["chosen_live"] == 0 and s.count["unchosen_done"] == 0, s.count
    env = make(37, **COOP)
    replay(env, s)
    assert not (env.get_state()[:, soa.W_STATUS] & 1).any()
    env.close()


def test_explicit_layouts_and_refused_ids():
    s = coop_script("explicit")
    L = 3
    ids = np.concatenate([st["ids"][st["mask"] != 0] for st in s.steps])
    assert s.count["refused"] >= 10 and (ids == L).any() and (ids == L + 7).any() and (ids < 0).any() and all((ids == k).any() for k in range(L))
    env = make(37, **COOP)
    b = replay(env, s)
    assert env.reset_device_refused() == s.count["refused"]
    # a further call adds to the counter, and refused envs are byte-identical before and after (running returns included)
    recs = env.get_state()
    b.fill()
    b.mask.from_host(np.ones(37, dtype=np.uint8))
    b.ids.from_host(np.where(np.arange(37) % 2 == 0, L, L + 7).astype(np.int32))
    env.reset_device(b.mask, b.ids, b.obs, b.rows32.buf, b.codes)
    assert env.reset_device_refused() == s.count["refused"] + 37
    assert np.array_equal(env.get_state(), recs)
    obs, codes, r32 = b.read()
    assert (obs == SENT64).all() and (codes == SENT8).all() and (r32 == SENTINEL).all()
    env.close()


def test_explicit_ids_reach_outside_the_envs_pool_slice():
    """two levels, two pool slices: an explicit id of the other level's slice is taken, as cz_reset takes it (same grid, other world)"""
    cfg = dict(COOP, level=["coop_test", "switch_test"])
    t = tables_of(9, **cfg)
    orc = VecOracle.from_vec_env(t, auto_reset=0)
    orc.reset()
    env = make(9, tables=t)
    env.reset(return_obs=False)
    b = Bufs(env)
    (b0, c0), (b1, c1) = t.pool_slices
    ids = np.array([(b1 + e % c1) if t.env_level[e] == 0 else (b0 + e % c0) for e in range(9)], dtype=np.int32)
    b.mask.from_host(np.ones(9, dtype=np.uint8)); b.ids.from_host(ids)
    before = b.read()
    env.reset_device(b.mask, b.ids, b.obs, b.rows32.buf, b.codes)
    rows = {e: oracle_reset(orc, e, int(ids[e])) for e in range(9)}
    check_rows("other slice", env, before, b.read(), rows)
    recs = strip(env.get_state())
    assert np.array_equal(recs, orc.records) and np.array_equal(recs[:, soa.W_LAYOUT], ids.astype(np.uint32))
    assert env.reset_device_refused() == 0
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4, 5: masks at their ends, statistics
# ---------------------------------------------------------------------------------------------------------------------------

def run_some(envs, orc, pol, steps):
    """-> how many env-steps were live ones (a finished env is frozen: auto_reset is off)"""
    live = 0
    for _ in range(steps):
        acts = pol.act(orc.records)
        live += int(((orc.records[:, soa.W_STATUS] & 1) == 0).sum())
        for env, b in envs:
            b.act.from_host(acts)
            env.step_device(b.act, b.obs, b.rew, b.term, b.trunc)
        orc.step(acts)
        pol.observe_result(orc.records)
    return live


def host_reset(envs, orc, lo, count):
    """cz_reset of envs [lo, lo + count) to the layouts they are on (no episode bump), so that the batch holds episodes of two ages"""
    ids = orc.records[lo:lo + count, soa.W_LAYOUT].astype(np.int32)
    for env, _ in envs:
        env.reset(layout_ids=ids, return_obs=False, env_begin=lo, env_count=count)
    for e in range(lo, lo + count):
        assert orc.oracle.lib.czo_reset_env(C.byref(orc.oracle.ctx), C.c_int64(e), C.c_uint32(int(ids[e - lo])),
                                            orc.records[e].ctypes.data_as(C.c_void_p), None) == 0


def test_empty_and_full_masks():
    t = tables_of(37, **COOP)
    env, orc = make(37, tables=t), VecOracle.from_vec_env(t, auto_reset=0)
    env.reset(return_obs=False); orc.reset()
    b = Bufs(env)
    pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(1))
    run_some([(env, b)], orc, pol, 7)
    host_reset([(env, b)], orc, 0, 18)
    run_some([(env, b)], orc, pol, 7)
    done = (orc.records[:, soa.W_STATUS] & 1) != 0
    assert done.any() and not done.all()
    recs, st = env.get_state(), env.stats()
    b.fill()
    before = b.read()
    b.mask.from_host(np.zeros(37, dtype=np.uint8))
    env.reset_device(b.mask, None, b.obs, b.rows32.buf, b.codes)
    assert np.array_equal(env.get_state(), recs) and env.stats() == st
    assert all(np.array_equal(x, y) for x, y in zip(b.read(), before))
    b.mask.from_host(np.full(37, 255, dtype=np.uint8))
    env.reset_device(b.mask, None, b.obs, b.rows32.buf, b.codes)
    rows = {e: oracle_reset(orc, e) for e in range(37)}
    check_rows("full mask", env, before, b.read(), rows)
    recs = strip(env.get_state())
    assert np.array_equal(recs, orc.records) and not recs[:, soa.W_T].any() and not (recs[:, soa.W_STATUS] & 1).any()
    env.close()


def test_statistics_equal_host_resets_of_the_same_set():
    t = tables_of(37, **COOP)
    env, twin, orc = make(37, tables=t), make(37, tables=t), VecOracle.from_vec_env(t, auto_reset=0)
    env.reset(return_obs=False); twin.reset(return_obs=False); orc.reset()
    b, bt = Bufs(env), Bufs(twin)
    pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(2))
    envs = [(env, b), (twin, bt)]
    live = run_some(envs, orc, pol, 7)
    host_reset(envs, orc, 0, 18)
    live += run_some(envs, orc, pol, 7)
    done = (orc.records[:, soa.W_STATUS] & 1) != 0
    chosen = np.random.default_rng(3).random(37) < 0.5
    assert (chosen & done).any() and (chosen & ~done).any() and (~chosen & done).any() and (~chosen & ~done).any()
    ids = np.full(37, -1, dtype=np.int32)
    for e in np.nonzero(chosen)[0]:
        oracle_reset(orc, int(e))
        ids[e] = orc.records[e, soa.W_LAYOUT]
    b.mask.from_host(chosen.astype(np.uint8)); b.ids.from_host(ids)
    env.reset_device(b.mask, b.ids)
    for e in np.nonzero(chosen)[0]:
        twin.reset(layout_ids=[int(ids[e])], return_obs=False, env_begin=int(e), env_count=1)
    st = env.stats()
    assert st == twin.stats() and st["env_steps"] == live and st["episodes"] == int(done.sum())      # aborted episodes: steps stay, none is counted
    live += run_some(envs, orc, pol, 10)
    st = env.stats()
    assert st == twin.stats() and st["env_steps"] == live
    assert np.array_equal(strip(env.get_state()), orc.records)
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6: every instance and agent count
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level,meta,agents,recipes,scheme,inst", INSTANCE_CASES)
def test_every_instance_and_agent_count(level, meta, agents, recipes, scheme, inst):
    """the mixed run, short, on every kernel instance and agent count; the calls name all three buffers, or - by the agent count - the
    float32 rows alone (the image is then built without the float64 encode) or the codes alone"""
    forms = {1: ("obs32",), 3: ("codes",)}.get(agents, ALL_FORMS) if level == "dense_8x8" else ALL_FORMS
    t = tables_of(9, level, meta, agents, recipes, scheme, 6, 3)
    s = Script(t, 12, 7, p_chosen=0.4)
    assert all(s.count[k] > 0 for k in ("chosen_done", "chosen_live", "unchosen_done", "unchosen_live")), s.count
    env = make(9, tables=t)
    assert instance(env) == inst
    replay(env, s, forms)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7, 8: layout group, despawn / respawn
# ---------------------------------------------------------------------------------------------------------------------------

def test_keyed_draw_lands_in_the_active_layout_group():
    cfg = dict(COOP, num_layouts=8)
    t = tables_of(37, **cfg)
    s = Script(t, 14, 5, groups=(2, 1))
    lay = np.concatenate([st["after"][sorted(st["rows"]), soa.W_LAYOUT] for st in s.steps])
    assert len(lay) >= 37 and ((lay >= 4) & (lay < 8)).all() and len(set(lay.tolist())) == 4      # (the oracle: the active half, all of it)
    env = make(37, tables=t)
    replay(env, s, forms=("obs",), prepare=lambda: env.set_layout_group(2, 1))
    env.close()


def test_despawn_respawn_on():
    from cooking_zoo_amd.spawn import decode_status, grace_bits
    t = tables_of(37, agent_despawn_rate=0.1, agent_respawn_rate=0.3, grace_period=3, spawn_seed=4, **COOP)
    env = make(37, tables=t)
    env.set_spawn_rates(0.1, 0.3, 3)
    s = Script(t, 14, 9, p_chosen=0.3)
    assert s.orc.oracle.ctx.spawn and s.count["chosen_live"] >= 37
    for st in s.steps:                                         # a restarted world: everybody present, the grace period running
        for e in st["rows"]:
            active, grace = decode_status(st["after"][e:e + 1, soa.W_STATUS], 2, grace_bits(3, 2))
            assert active.all() and (grace == 3).all() and not st["after"][e, soa.W_STATUS] & 0xFFF
    b = replay(env, s)
    orc = s.orc                                                # 10 more steps, nobody reset: still the oracle's with set_spawn
    orc_records = orc.records.copy()
    pol = BumperActions(t.dims, t.scheme_class.CODE, np.random.default_rng(10))
    try:
        for k in range(10):
            acts = pol.act(orc.records)
            b.act.from_host(acts)
            env.step_device(b.act, b.obs, b.rew, b.term, b.trunc)
            obs, rew, term, trunc = orc.step(acts)
            pol.observe_result(orc.records)
            assert np.array_equal(b.obs.to_host(), obs.view(np.uint64)) and np.array_equal(b.trunc.to_host(), trunc), f"step {k} behind the resets"
            assert np.array_equal(strip(env.get_state()), orc.records), f"step {k} behind the resets"
    finally:
        orc.records[:] = orc_records
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9: inside a capture
# ---------------------------------------------------------------------------------------------------------------------------

def test_reset_device_inside_a_callers_capture():
    n, K, R = 256, 4, 50
    cfg = dict(COOP, num_layouts=8)
    t = tables_of(n, **cfg)
    env, ref = make(n, tables=t), make(n, tables=t)
    be, br = Bufs(env), Bufs(ref)
    L = _native.lib()

    def loop(e, b, k):
        for _ in range(k):
            _native.check(e._h, L.cz_probe_policy(e._h, b.obs.ptr, None, b.act.ptr))
            e.step_device(b.act, b.obs, b.rew, b.term, b.trunc)
            e.reset_device(None, None, b.obs, b.rows32.buf, b.codes)

    for e, b in ((env, be), (ref, br)):
        e.reset(return_obs=False)
        e.observe_device(b.obs)
    cs = CallerStream(env)
    with cs.capture():
        loop(env, be, K)                                        # K x [policy, step, reset of the finished envs]: captured, not executed
    assert env._steps == 0 and env.captured_steps == K         # (and the resets are no steps)
    assert np.array_equal(env.get_state(), ref.get_state()), "capturing must not have stepped or reset anything"
    cs.replay(R)
    cs.sync()
    loop(ref, br, K * R)
    ref.sync()
    assert ref._steps == K * R
    assert np.array_equal(env.get_state(), ref.get_state())
    for x, y in zip(be.read() + (be.act.to_host(), be.rew.to_host().view(np.uint64), be.term.to_host(), be.trunc.to_host()),
                    br.read() + (br.act.to_host(), br.rew.to_host().view(np.uint64), br.term.to_host(), br.trunc.to_host())):
        assert np.array_equal(x, y)
    st = env.stats()
    assert st == ref.stats() and st["episodes"] >= n and st["env_steps"] == n * K * R      # no env-step went to a reset pass
    assert not (env.get_state()[:, soa.W_STATUS] & 1).any()
    cs.close()
    env.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 10: shards
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mixed", "explicit"])
def test_three_unequal_shards_equal_one_handle(kind):
    from cooking_zoo_amd.sharded import ShardedVecEnv
    s = coop_script(kind)
    n, A = 37, 2
    many = ShardedVecEnv(n, COOP["level"], COOP["meta"], A, COOP["max_steps"], TWO, action_scheme="scheme3", num_layouts=3, auto_reset=False,
                         device_ids=[0, 0, 0])
    assert sorted(c for _, c in many.ranges) == [12, 12, 13]
    F, Fp = many.F, many.codes_pitch
    act, rew, term, trunc = many.alloc((A,), np.int32), many.alloc((A,), np.float64), many.alloc((A,), np.uint8), many.alloc((A,), np.uint8)
    obs, r32, codes = many.alloc((A, F), np.uint64), many.alloc((A, F), np.uint32), many.alloc((A, Fp), np.uint8)
    mask, ids = many.alloc((), np.uint8), many.alloc((), np.int32)
    many.reset(return_obs=False)
    table = many.obs_table()
    for t, st in enumerate(s.steps):
        r32.from_host(np.full((n, A, F), SENTINEL, dtype=np.uint32)); codes.from_host(np.full((n, A, Fp), SENT8, dtype=np.uint8))
        act.from_host(st["acts"])
        many.step_device(act, obs, rew, term, trunc)
        mask.from_host(st["mask"])
        if st["ids"] is not None:
            ids.from_host(st["ids"])
        many.reset_device(mask, ids if st["ids"] is not None else None, obs, r32, codes)
        assert np.array_equal(strip(many.get_state()), st["after"]), f"call {t}: records"
        g64, g32, gc = obs.to_host(), r32.to_host(), codes.to_host()
        want = st["obs"].copy()
        for e, o in st["rows"].items():
            want[e] = o
            assert np.array_equal(g32[e], want32(o)) and np.array_equal(table[gc[e][:, :F]].view(np.uint64), o.view(np.uint64)), (t, e)
        rest = [e for e in range(n) if e not in st["rows"]]
        assert np.array_equal(g64, want.view(np.uint64)) and (g32[rest] == SENTINEL).all() and (gc[rest] == SENT8).all(), f"call {t}"
    assert many.reset_device_refused() == s.count["refused"]
    many.close()
