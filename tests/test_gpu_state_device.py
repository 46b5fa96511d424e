"""GPU: save, restore and fork of env states on the device (cz_save_device / cz_restore_device; CookingVecEnv.save_device,
restore_device, fork_device).  Everything is compared exactly: records as bytes against the oracle's (running-return words apart:
those against a numpy sum of the oracle's rewards in step order), float64 rows as uint64, float32 rows as uint32 against np.float32
of the oracle's rows, codes decoded through obs_table().  Every output buffer is pre-filled with a sentinel and the float32 buffer is
guarded.  What a restored env must be comes from the oracle alone: its record e set to the saved row, its rows the oracle's observe
of that record (`Twin.restore`); the statistics follow the numpy model of tests/host_common.py."""
import ctypes as C

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from fuzz_policy import BumperActions
from oracle_binding import VecOracle
from host_common import env_steps, row_ok, steps_correction
from vec_common import (ALL_FORMS, COOP, FORM_SUBSETS, INSTANCE_CASES, SENT8, SENT64, SENTINEL, TWO, Bufs, CallerStream, check_rows, env_of,
                        instance, strip, tables_of)

pytestmark = pytest.mark.gpu

RET = slice(soa.RET_WORD0, soa.RET_WORD0 + 8)
ARCH_SENT = 0xA5C3F00D              # an archive word nobody wrote (as a layout id, a recipe id or a pool word it would be refused)
DONE = soa.STATUS_DONE


def make(n, auto_reset, tables):
    return env_of(tables, auto_reset)


class Twin:
    """The oracle's batch and what the device keeps beside it: the running returns (record words 12..19: the rewards of the episode
    added in step order), the per-env statistics words, and the episodes that ended since the last collect."""

    def __init__(self, tables, auto_reset, seed):
        self.t, self.n, self.A, self.auto = tables, tables.num_envs, tables.dims.A, bool(auto_reset)
        self.orc = VecOracle.from_vec_env(tables, auto_reset=int(auto_reset))
        self.pol = BumperActions(tables.dims, tables.scheme_class.CODE, np.random.default_rng(seed))
        self.ret, self.fin = np.zeros((self.n, 4)), np.zeros((self.n, 4))
        self.su, self.lensum = np.zeros(self.n, np.int32), np.zeros(self.n, np.int64)
        self.episodes = self.taken = self.passes = 0
        self.last = {}                       # env -> [episode word, length, returns, finished since the last collect]
        self.orc.reset()

    def records(self):
        r = self.orc.records.copy()
        r[:, RET] = self.ret.view(np.uint32)
        return r

    def done(self):
        return (self.orc.records[:, soa.W_STATUS] & DONE) != 0

    def act(self):
        return self.pol.act(self.orc.records)

    def step(self, acts):
        stepped = ~self.done()                                 # (a finished env is frozen, or takes its reset pass: no step either way)
        obs, rew, term, trunc = self.orc.step(acts)
        self.pol.observe_result(self.orc.records)
        after = self.orc.records
        ended = stepped & self.done()
        self.ret[stepped, :self.A] += rew[stepped]
        for e in np.nonzero(ended)[0]:
            self.last[int(e)] = [int(after[e, soa.W_EPISODE]), int(after[e, soa.W_T]), self.ret[e].copy(), self.last.get(int(e), [0] * 4)[3] + 1]
        self.fin[ended] += self.ret[ended]
        self.ret[ended] = 0.0
        self.lensum[ended] += after[ended, soa.W_T]
        self.episodes += int(ended.sum()); self.taken += int(stepped.sum())
        self.passes += int((~stepped).sum()) if self.auto else 0
        return obs.copy(), rew.copy(), term.copy(), trunc.copy()

    def host_reset(self, env, lo, count):
        """cz_reset of envs [lo, lo + count) to the layouts they are on: the batch then holds episodes of two ages"""
        ids = self.orc.records[lo:lo + count, soa.W_LAYOUT].astype(np.int32)
        env.reset(layout_ids=ids, return_obs=False, env_begin=lo, env_count=count)
        for e in range(lo, lo + count):
            rec = self.orc.records[e]
            if not rec[soa.W_STATUS] & DONE:
                self.su[e] += np.int32(rec[soa.W_T])
            assert self.orc.oracle.lib.czo_reset_env(C.byref(self.orc.oracle.ctx), C.c_int64(e), C.c_uint32(int(ids[e - lo])),
                                                     rec.ctypes.data_as(C.c_void_p), None) == 0
            self.ret[e] = 0.0

    def restore(self, archive, slots=None):
        """env e becomes row slots[e] of `archive` (whole records, uint32 [capacity][RW]) -> (the oracle's rows of the restored
        envs, how many envs were refused)"""
        t, rows, refused = self.t, {}, 0
        for e in range(self.n):
            s = e if slots is None else int(slots[e])
            if s < 0:
                continue
            if s >= len(archive) or not row_ok(archive[s], t.dims, len(t.layouts), len(t.book_names), t.num_recipes):
                refused += 1
                continue
            row, old = archive[s], self.orc.records[e]
            self.su[e] += steps_correction(old[soa.W_STATUS], old[soa.W_T], row[soa.W_STATUS], row[soa.W_T])
            self.orc.records[e] = strip(row[None])[0]
            self.ret[e] = row[RET].copy().view(np.float64)
            rows[e] = self.orc.oracle.observe(self.orc.records[e])
        return rows, refused

    def stats(self):
        """what cz_get_stats must return of the counters a restore can touch (return_sum: env e in chain e, then the binary tree)"""
        level = np.zeros((256, 4))
        level[:self.n] += self.fin
        while level.shape[0] > 1:
            level = level[:level.shape[0] // 2] + level[level.shape[0] // 2:]
        rec = self.orc.records
        return dict(env_steps=env_steps(self.su, self.lensum, rec[:, soa.W_STATUS], rec[:, soa.W_T]), episodes=self.episodes,
                    length_sum=int(self.lensum.sum()), return_sum=[float(v) for v in level[0]])


def assert_state(env, tw, ctx):
    got = env.get_state()
    assert np.array_equal(strip(got), tw.orc.records), f"{ctx}: records"
    assert np.array_equal(got[:, RET], tw.ret.view(np.uint32)), f"{ctx}: running returns"


def assert_stats(env, tw, ctx):
    got, want = env.stats(), tw.stats()
    assert want["env_steps"] == tw.taken, f"{ctx}: the model itself"
    for k in ("env_steps", "episodes", "length_sum"):
        assert got[k] == want[k], f"{ctx}: {k} {got[k]}, the model gives {want[k]}"
    assert np.array_equal(np.array(got["return_sum"]).view(np.uint64), np.array(want["return_sum"]).view(np.uint64)), f"{ctx}: return_sum"


def step_both(env, b, tw, ctx, acts=None):
    """one step on the device and on the oracle, compared -> (actions, the device's outputs and records)"""
    acts = tw.act() if acts is None else acts
    b.act.from_host(acts)
    env.step_device(b.act, b.obs, b.rew, b.term, b.trunc)
    obs, rew, term, trunc = tw.step(acts)
    got = (b.obs.to_host(), b.rew.to_host().view(np.uint64), b.term.to_host(), b.trunc.to_host(), env.get_state())
    assert np.array_equal(got[0], obs.view(np.uint64)), f"{ctx}: rows"
    assert np.array_equal(got[1], rew.view(np.uint64)) and np.array_equal(got[2], term) and np.array_equal(got[3], trunc), f"{ctx}: rewards / flags"
    assert_state(env, tw, ctx)
    return acts, got


def start(n, auto_reset, seed, tables=None, **cfg):
    t = tables or tables_of(n, **cfg)
    env, tw = make(n, auto_reset=auto_reset, tables=t), Twin(t, auto_reset, seed)
    env.reset(return_obs=False)
    assert_state(env, tw, "reset")
    return t, env, tw, Bufs(env)


def archive_of(env, rows):
    a = env.alloc((rows, env.dims.RW), np.uint32)
    a.from_host(np.full((rows, env.dims.RW), ARCH_SENT, dtype=np.uint32))
    return a


def restore_both(env, b, tw, ctx, arch, slots=None, forms=ALL_FORMS, d_slot=None, fork=False, host_archive=None, capacity=None):
    """restore_device (or fork_device) with sentinel-filled outputs, against Twin.restore -> the oracle's rows"""
    b.fill()
    before = b.read()
    host_archive = tw.records() if fork else (arch.to_host() if host_archive is None else host_archive)
    if capacity is not None:
        host_archive = host_archive[:capacity]
    outs = (b.obs if "obs" in forms else None, b.rows32.buf if "obs32" in forms else None, b.codes if "codes" in forms else None)
    if slots is not None:
        d_slot = d_slot or env.alloc((env.num_envs,), np.int32)
        d_slot.from_host(np.asarray(slots, dtype=np.int32))
    refused0 = env.restore_device_refused()
    if fork:
        env.fork_device(d_slot, *outs)
    else:
        env.restore_device(arch, d_slot, *outs, capacity=capacity)
    rows, refused = tw.restore(host_archive, slots)
    check_rows(ctx, env, before, b.read(), rows, forms)
    assert_state(env, tw, ctx)
    assert env.restore_device_refused() - refused0 == refused, f"{ctx}: refused"
    return rows


def mixed_ages(env, b, tw):
    """7 steps, a host reset of envs [0, 18), 7 steps: with 12-step episodes and auto-reset off the batch then holds finished envs
    and envs in mid-episode"""
    for k in range(7):
        step_both(env, b, tw, f"step {k}")
    tw.host_reset(env, 0, 18)
    for k in range(7, 14):
        step_both(env, b, tw, f"step {k}")
    done = tw.done()
    assert done.sum() >= 8 and (~done).sum() >= 8
    return done


# ---------------------------------------------------------------------------------------------------------------------------
# 1: round trip
# ---------------------------------------------------------------------------------------------------------------------------

def test_round_trip_replays_the_same_stretch():
    t, env, tw, b = start(37, True, 1, **COOP)
    arch = archive_of(env, 37)
    for k in range(10):
        step_both(env, b, tw, f"step {k}")
    env.save_device(arch)
    saved = arch.to_host()
    assert np.array_equal(saved, tw.records()), "the archive is the batch, running returns included"
    assert np.array_equal(env.get_state(), saved), "a save changes nothing of the handle"
    ended0, passes0, first = tw.episodes, tw.passes, []
    for k in range(12):
        first.append(step_both(env, b, tw, f"first pass, step {k}"))
    assert tw.episodes - ended0 >= 37 and tw.passes - passes0 >= 37      # (the oracle: episode ends and reset passes lie inside the stretch)
    rows = restore_both(env, b, tw, "restore", arch)
    assert len(rows) == 37 and np.array_equal(env.get_state(), saved)
    for k, (acts, want) in enumerate(first):
        _, got = step_both(env, b, tw, f"second pass, step {k}", acts)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), f"second pass, step {k}: not the first pass"
    assert_stats(env, tw, "after both passes")
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2, 3: slot maps, forks
# ---------------------------------------------------------------------------------------------------------------------------

def test_fork_with_a_slot_map():
    t, env, tw, b = start(37, False, 2, **COOP)
    arch, d_slot = archive_of(env, 13), env.alloc((37,), np.int32)       # 11 rows and two behind them that nobody may write
    want = np.full((13, env.dims.RW), ARCH_SENT, dtype=np.uint32)

    def save(pairs):
        slots = np.full(37, -1, dtype=np.int32)
        for e, s in pairs:
            slots[e] = s
        d_slot.from_host(slots)
        env.save_device(arch, d_slot, capacity=11)
        recs = tw.records()
        for e, s in pairs:
            if s < 11:
                want[s] = recs[e]
        assert np.array_equal(arch.to_host(), want)

    for k in range(7):
        step_both(env, b, tw, f"step {k}")
    save([(31, 0), (2, 1), (17, 2), (36, 3), (9, 4), (20, 5), (5, 11), (6, 18)])        # (slots 11 and 18: past the archive, nothing written)
    tw.host_reset(env, 0, 18)
    for k in range(7, 14):
        step_both(env, b, tw, f"step {k}")
    save([(35, 6), (0, 7), (22, 8), (13, 9), (28, 10)])
    done = tw.done()
    rng = np.random.default_rng(5)
    slots = np.where(rng.random(37) < 0.33, -1, rng.integers(0, 11, 37)).astype(np.int32)
    chosen, shared = slots >= 0, np.bincount(slots[slots >= 0], minlength=11)
    row_done = (want[:11, soa.W_STATUS] & DONE) != 0
    # (the oracle alone) all four kinds of env, rows that several envs take, finished and running rows
    assert (chosen & done).sum() >= 3 and (chosen & ~done).sum() >= 3 and (~chosen & done).sum() >= 2 and (~chosen & ~done).sum() >= 2
    assert (shared >= 2).sum() >= 3 and row_done[slots[chosen]].any() and (~row_done[slots[chosen]]).any()
    rows = restore_both(env, b, tw, "fork", arch, slots, d_slot=d_slot, capacity=11)
    assert sorted(rows) == np.nonzero(chosen)[0].tolist()
    assert np.array_equal(env.get_state()[chosen], want[slots[chosen]]), "a restored record is its row, word for word"
    assert env.restore_device_refused() == 0
    for k in range(10):
        step_both(env, b, tw, f"step {k} behind the fork")
    assert_stats(env, tw, "behind the fork")
    env.close()


def test_fork_device_with_overlapping_sources_and_destinations():
    t, env, tw, b = start(37, False, 3, **COOP)
    mixed_ages(env, b, tw)
    src = ((np.arange(37) * 7 + 3) % 37).astype(np.int32)
    assert sorted(src.tolist()) == list(range(37)) and (src != np.arange(37)).sum() == 36      # every source is a destination as well
    pre = env.get_state()
    rows = restore_both(env, b, tw, "fork_device", None, src, fork=True)
    assert len(rows) == 37 and np.array_equal(env.get_state(), pre[src]), "the gather from the records before the call"
    src[::3] = -1                                               # ... and with envs that keep their state, float32 rows alone
    pre = env.get_state()
    restore_both(env, b, tw, "fork_device, some kept", None, src, forms=("obs32",), fork=True)
    assert np.array_equal(env.get_state(), np.where((src >= 0)[:, None], pre[np.maximum(src, 0)], pre))
    for k in range(5):
        step_both(env, b, tw, f"step {k} behind the forks")
    assert_stats(env, tw, "behind the forks")
    env.close()


@pytest.mark.parametrize("forms", FORM_SUBSETS, ids="+".join)
def test_every_subset_of_forms(forms):
    """k_restore_where's rows come from one writer shared with the other off-step kernels: each form alone, each pair - float32 rows
    from the image observe built, the float64 table staged or not - and all three; a buffer the call does not name keeps its sentinel"""
    t, env, tw, b = start(37, False, 6, **COOP)
    done = mixed_ages(env, b, tw)
    arch = archive_of(env, 37)
    env.save_device(arch)
    row_done = done.copy()
    for k in range(14, 16):
        step_both(env, b, tw, f"step {k}")
    slots = ((np.arange(37) * 7 + 3) % 37).astype(np.int32)
    slots[::3] = -1
    chosen, done = slots >= 0, tw.done()
    # (the oracle alone) envs that are chosen and envs that are left alone, finished and running ones of each; rows of both kinds
    assert min((chosen & done).sum(), (chosen & ~done).sum(), (~chosen & done).sum(), (~chosen & ~done).sum()) >= 3
    assert row_done[slots[chosen]].any() and (~row_done[slots[chosen]]).any()
    rows = restore_both(env, b, tw, "restore", arch, slots, forms)
    assert sorted(rows) == np.nonzero(chosen)[0].tolist() and env.restore_device_refused() == 0
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4: refusals
# ---------------------------------------------------------------------------------------------------------------------------

def test_refused_slots_and_rows():
    t, env, tw, b = start(37, False, 4, **COOP)
    mixed_ages(env, b, tw)
    d, L, n_recipes = env.dims, len(t.layouts), len(t.book_names)
    recs = tw.records()
    rows = np.stack([recs[30], recs[4], recs[30], recs[4], recs[30], recs[4], recs[12], recs[33]])      # capacity 8
    rows[2, soa.W_LAYOUT] = L                                                                           # each of rows 2..5: one defect
    rows[3, soa.W_RECIPES] = (rows[3, soa.W_RECIPES] & ~np.uint32(0xFF00)) | np.uint32(n_recipes << 8)
    rows[4, soa.W_POOL] = 1 | (L << 16)
    rows[5, d.dyn0_word0 + d.D - 1] &= ~np.uint32(soa.DYN_ALIVE << 24)
    rows[5, d.dyn1_word0 + d.D - 1] = 1
    for s in range(8):                                          # the same input cz_set_state takes or rejects on the host
        if s in (2, 3, 4, 5):
            with pytest.raises(_native.NativeError, match="cz_set_state: record 0"):
                env.set_state(rows[s], env_begin=0)
        assert row_ok(rows[s], d, L, n_recipes, t.num_recipes) == (s not in (2, 3, 4, 5))
    assert_state(env, tw, "the host's refusals")
    arch = archive_of(env, 8)
    arch.from_host(rows)
    slots = np.array([[0, 2, 8, 3, -1, 4, 1, 5, 15, 6, 7][e % 11] for e in range(37)], dtype=np.int32)
    before = env.get_state()
    restored = restore_both(env, b, tw, "refusals", arch, slots)
    bad = np.isin(slots, (2, 3, 4, 5, 8, 15))
    assert env.restore_device_refused() == int(bad.sum()) == 21
    assert sorted(restored) == np.nonzero((slots >= 0) & ~bad)[0].tolist() and len(restored) == 13
    after = env.get_state()
    assert np.array_equal(after[bad | (slots < 0)], before[bad | (slots < 0)]), "refused and unchosen envs: byte-identical"
    assert np.array_equal(after[(slots >= 0) & ~bad], rows[slots[(slots >= 0) & ~bad]])
    assert_stats(env, tw, "refusals")
    # without slots the archive needs a row per env: refused on the host, nothing launched, nothing counted
    for call in (lambda: env.save_device(arch), lambda: env.restore_device(arch, None, b.obs, b.rows32.buf, b.codes)):
        with pytest.raises(_native.NativeError, match=r"capacity 8 < 37 envs"):
            call()
    assert np.array_equal(env.get_state(), after) and np.array_equal(arch.to_host(), rows) and env.restore_device_refused() == 21
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5: every instance and agent count
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level,meta,agents,recipes,scheme,inst", INSTANCE_CASES)
def test_every_instance_and_agent_count(level, meta, agents, recipes, scheme, inst):
    """save / step / fork / step, short, on every kernel instance and agent count; the calls name all three buffers, or - by the
    agent count - the float32 rows alone (the image is then built without the float64 encode) or the codes alone"""
    forms = {1: ("obs32",), 3: ("codes",)}.get(agents, ALL_FORMS) if level == "dense_8x8" else ALL_FORMS
    t, env, tw, b = start(9, False, 7, tables=tables_of(9, level, meta, agents, recipes, scheme, 6, 3))
    assert instance(env) == inst
    arch = archive_of(env, 9)
    for k in range(4):
        step_both(env, b, tw, f"step {k}")
    env.save_device(arch)
    assert np.array_equal(arch.to_host(), tw.records())
    for k in range(4, 8):
        step_both(env, b, tw, f"step {k}")
    assert tw.done().any()                                                   # (6-step episodes: finished envs take rows of running ones)
    restore_both(env, b, tw, "restore", arch, [0, -1, 1, 1, 8, -1, 3, 2, 9], forms)      # (slot 9: past the archive)
    assert env.restore_device_refused() == 1
    restore_both(env, b, tw, "fork", None, [(e * 4 + 1) % 9 if e % 4 else -1 for e in range(9)], forms, fork=True)
    for k in range(8, 12):
        step_both(env, b, tw, f"step {k}")
    assert_stats(env, tw, "at the end")
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6: despawn / respawn
# ---------------------------------------------------------------------------------------------------------------------------

def test_despawn_respawn_on():
    from cooking_zoo_amd.spawn import decode_status, grace_bits
    tables = tables_of(37, agent_despawn_rate=0.1, agent_respawn_rate=0.3, grace_period=3, spawn_seed=4, **COOP)
    t, env, tw, b = start(37, True, 9, tables=tables)
    env.set_spawn_rates(0.1, 0.3, 3)
    assert tw.orc.oracle.ctx.spawn
    for k in range(8):
        step_both(env, b, tw, f"step {k}")
    src = ((np.arange(37) * 7 + 3) % 37).astype(np.int32)
    src[::5] = -1
    status = tw.orc.records[:, soa.W_STATUS].copy()
    active, grace = decode_status(status[src[src >= 0]], 2, grace_bits(3, 2))
    assert (~active).sum() >= 3 and (grace > 0).sum() >= 3, "the sources carry despawn bits and countdowns"      # (the oracle alone)
    restore_both(env, b, tw, "fork", None, src, fork=True)
    assert np.array_equal(env.get_state()[src >= 0, soa.W_STATUS], status[src[src >= 0]])
    for k in range(10):
        step_both(env, b, tw, f"step {k} behind the fork")
    assert_stats(env, tw, "behind the fork")
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7: statistics and episode records
# ---------------------------------------------------------------------------------------------------------------------------

def assert_finished(env, tw, ctx):
    got = env.finished_episodes()
    assert got["env"].tolist() == sorted(tw.last), f"{ctx}: which envs finished an episode"
    for r in got:
        episode, length, ret, finished = tw.last[int(r["env"])]
        assert (int(r["episode"]), int(r["length"]), int(r["finished"])) == (episode, length, finished), f"{ctx}: env {r['env']}"
        assert np.array_equal(np.array(r["ret"]).view(np.uint64), ret.view(np.uint64)), f"{ctx}: return of env {r['env']}"
    tw.last = {}


def test_statistics_and_episode_records():
    t, env, tw, b = start(37, True, 11, **COOP)
    arch = archive_of(env, 74)
    ident = env.alloc((37,), np.int32)
    for k in range(8):
        step_both(env, b, tw, f"step {k}")
    ident.from_host(np.arange(37, dtype=np.int32))
    env.save_device(arch, ident)                                # rows 0..36: episodes in flight, 8 steps old
    for k in range(8, 12):
        step_both(env, b, tw, f"step {k}")
    ident.from_host(np.arange(37, 74, dtype=np.int32))
    env.save_device(arch, ident)                                # rows 37..73: finished episodes (12-step episodes), a few younger ones
    rows = arch.to_host()
    row_done = (rows[:, soa.W_STATUS] & DONE) != 0
    assert (~row_done[:37]).all() and row_done[37:].sum() >= 20
    assert_stats(env, tw, "before the restores")
    assert_finished(env, tw, "before the restores")
    rng, kinds, inherited = np.random.default_rng(12), set(), 0
    for call in range(4):
        slots = np.where(rng.random(37) < 0.6, rng.integers(0, 74, 37), -1).astype(np.int32)
        dest_done = tw.done()
        kinds |= {(bool(dest_done[e]), bool(row_done[slots[e]])) for e in range(37) if slots[e] >= 0}
        restore_both(env, b, tw, f"restore {call}", arch, slots, forms=("obs32",), d_slot=ident, host_archive=rows)
        assert_stats(env, tw, f"restore {call}")                # no episode counted, env_steps still the steps taken
        assert len(env.finished_episodes()) == 0, "an episode cut short by a restore leaves no record"
        since = np.zeros(37, np.int64)                          # steps since the restore, per env
        for k in range(3):
            before_t = tw.orc.records[:, soa.W_T].copy()
            step_both(env, b, tw, f"restore {call}, step {k}")
            since += 1
            for e, (_, length, _, _) in tw.last.items():
                inherited += int(length > since[e] and before_t[e] + 1 == length)
        assert_stats(env, tw, f"restore {call}, steps")
        assert_finished(env, tw, f"restore {call}, steps")
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}, kinds
    assert inherited >= 10, "restored episodes ended with lengths that reach back before the restore"
    for k in range(14):
        step_both(env, b, tw, f"last stretch, step {k}")
    assert_stats(env, tw, "at the end")
    assert_finished(env, tw, "at the end")
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8: inside a capture
# ---------------------------------------------------------------------------------------------------------------------------

def test_save_and_restore_inside_a_callers_capture():
    n, K = 64, 3
    t = tables_of(n, **dict(COOP, num_layouts=8))
    env, ref = make(n, auto_reset=True, tables=t), make(n, auto_reset=True, tables=t)
    be, br = Bufs(env), Bufs(ref)
    ae, ar = archive_of(env, n), archive_of(ref, n)
    L = _native.lib()

    def loop(e, b, arch):
        e.save_device(arch)
        for _ in range(K):
            _native.check(e._h, L.cz_probe_policy(e._h, b.obs.ptr, None, b.act.ptr))
            e.step_device(b.act, b.obs, b.rew, b.term, b.trunc)
        e.restore_device(arch, None, b.obs, b.rows32.buf, b.codes)
        _native.check(e._h, L.cz_probe_policy(e._h, b.obs.ptr, None, b.act.ptr))
        e.step_device(b.act, b.obs, b.rew, b.term, b.trunc)

    for e, b in ((env, be), (ref, br)):
        e.reset(return_obs=False)
        e.observe_device(b.obs)
    cs = CallerStream(env)
    with cs.capture():
        loop(env, be, ae)                                       # [save, K x (policy, step), restore, policy, step]: captured, not executed
    assert env._steps == 0 and env.captured_steps == K + 1     # (save and restore are no steps)
    assert np.array_equal(env.get_state(), ref.get_state()), "capturing must not have run anything"
    assert (ae.to_host() == ARCH_SENT).all()
    cs.replay(2)
    cs.sync()
    for _ in range(2):
        loop(ref, br, ar)
    ref.sync()
    assert ref._steps == 2 * (K + 1)
    state = env.get_state()
    assert np.array_equal(state, ref.get_state()) and (state[:, soa.W_T] == 2).all()        # (each replay ends one step behind what it saved)
    assert np.array_equal(ae.to_host(), ar.to_host())
    for x, y in zip(be.read() + (be.act.to_host(), be.rew.to_host().view(np.uint64), be.term.to_host(), be.trunc.to_host()),
                    br.read() + (br.act.to_host(), br.rew.to_host().view(np.uint64), br.term.to_host(), br.trunc.to_host())):
        assert np.array_equal(x, y)
    st = env.stats()
    assert st == ref.stats() and st["env_steps"] == n * 2 * (K + 1)
    assert env.restore_device_refused() == 0
    cs.close()
    env.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9: shards
# ---------------------------------------------------------------------------------------------------------------------------

def test_three_unequal_shards_equal_one_handle():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n, A = 37, 2
    t, one, tw, b = start(n, False, 13, **COOP)
    many = ShardedVecEnv(n, COOP["level"], COOP["meta"], A, COOP["max_steps"], TWO, action_scheme="scheme3", num_layouts=3, auto_reset=False,
                         device_ids=[0, 0, 0])
    assert sorted(c for _, c in many.ranges) == [12, 12, 13]
    F, Fp, RW = many.F, many.codes_pitch, one.dims.RW
    act, rew, term, trunc = many.alloc((A,), np.int32), many.alloc((A,), np.float64), many.alloc((A,), np.uint8), many.alloc((A,), np.uint8)
    obs, r32, codes = many.alloc((A, F), np.uint64), many.alloc((A, F), np.uint32), many.alloc((A, Fp), np.uint8)
    arch, src = many.alloc((RW,), np.uint32), many.alloc((), np.int32)
    many.reset(return_obs=False)

    def steps(k0, k1):
        for k in range(k0, k1):
            acts, _ = step_both(one, b, tw, f"step {k}")
            act.from_host(acts)
            many.step_device(act, obs, rew, term, trunc)
            assert np.array_equal(many.get_state(), one.get_state()), f"step {k}: the shards"

    def compare(ctx, rows):
        got, want = (obs.to_host(), codes.to_host(), r32.to_host()), b.read()
        assert np.array_equal(many.get_state(), one.get_state()), f"{ctx}: records"
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), f"{ctx}: rows"
        assert many.restore_device_refused() == one.restore_device_refused()

    def sentinels():
        obs.from_host(np.full((n, A, F), SENT64, dtype=np.uint64)); codes.from_host(np.full((n, A, Fp), SENT8, dtype=np.uint8))
        r32.from_host(np.full((n, A, F), SENTINEL, dtype=np.uint32))

    steps(0, 7)
    many.save_device(arch)
    saved = arch.to_host()
    assert np.array_equal(saved, tw.records())
    steps(7, 14)
    assert tw.done().sum() >= 30                                # (12-step episodes, auto-reset off: the restore un-freezes finished envs)
    one_arch = archive_of(one, n)
    one_arch.from_host(saved)
    sentinels()
    many.restore_device(arch, None, obs, r32, codes)
    compare("identity restore", restore_both(one, b, tw, "identity restore", one_arch))
    steps(14, 17)
    # a fork inside every shard: local indices for the shards, the same envs by their global index for the one handle
    local = np.concatenate([np.where(np.arange(c) % 4 == 3, -1, (np.arange(c) * 5 + 1) % c) for _, c in many.ranges]).astype(np.int32)
    base = np.concatenate([np.full(c, lo) for lo, c in many.ranges])
    assert (local >= 0).sum() >= 24 and len(local) == n
    src.from_host(local)
    sentinels()
    many.fork_device(src, obs, r32, codes)
    compare("shard-local fork", restore_both(one, b, tw, "shard-local fork", None, np.where(local >= 0, local + base, -1), fork=True))
    steps(17, 22)
    assert many.stats()["env_steps"] == one.stats()["env_steps"] == tw.taken
    many.close(); one.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 10: a batch of two levels
# ---------------------------------------------------------------------------------------------------------------------------

def test_a_record_of_another_level_keeps_its_recipes_and_pool_slice():
    cfg = dict(COOP, level=["coop_test", "switch_test"], num_layouts=4)
    t, env, tw, b = start(9, True, 15, **cfg)
    (b0, c0), (b1, c1) = t.pool_slices
    assert c0 >= 2 and c1 >= 2 and set(t.env_level.tolist()) == {0, 1}
    for k in range(3):
        step_both(env, b, tw, f"step {k}")
    src = np.array([e + 1 if e % 3 == 0 else -1 for e in range(9)], dtype=np.int32)         # consecutive envs: the other level
    took = np.nonzero(src >= 0)[0]
    assert (t.env_level[took] != t.env_level[src[took]]).all()
    pre = tw.records()
    assert (pre[took, soa.W_POOL] != pre[src[took], soa.W_POOL]).all()
    restore_both(env, b, tw, "fork across levels", None, src, fork=True)
    got = env.get_state()
    for w in (soa.W_RECIPES, soa.W_POOL, soa.W_LAYOUT):
        assert np.array_equal(got[took, w], pre[src[took], w])
    episode = got[took, soa.W_EPISODE].copy()
    for k in range(3, 14):                                      # 12-step episodes: the forks finish and restart inside this stretch
        step_both(env, b, tw, f"step {k}")
    now = tw.orc.records
    assert (now[took, soa.W_EPISODE] > episode).all() and np.array_equal(now[took, soa.W_POOL], pre[src[took], soa.W_POOL])
    for e in took:                                              # (the oracle: the auto-reset drew inside the record's slice)
        base, count = (b0, c0) if t.env_level[src[e]] == 0 else (b1, c1)
        assert base <= now[e, soa.W_LAYOUT] < base + count
    assert_stats(env, tw, "at the end")
    env.close()
