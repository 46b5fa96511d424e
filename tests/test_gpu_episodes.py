"""GPU: the per-env episode records (cz_episodes_collect / CookingVecEnv.collect_episodes, finished_episodes; the `episode` entries
of the reference's `infos`, cooking_env.py:248,264,329).  What every collect must report comes from the numpy model of
episodes_common.py, which walks the oracle's per-step rewards, flags and records; everything compares exactly - returns as uint64,
the packed list byte for byte - and every output array is pre-filled with a sentinel and guarded behind its end.  The conditions
that keep a test from passing vacuously (episodes ended, both ways to end, agents gone, several episodes inside one launch) are
asserted on the model's run, never on the device's."""
import functools

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from episodes_common import EP, Collector, EpisodeModel, same_entries
from fuzz_policy import BumperActions
from host_common import register_fixture_recipes
from oracle_binding import VecOracle
from vec_common import (COOP as COOP12, TWO, CallerStream, env_of as make, instance, last_lean, last_mode, oracle_reset, strip,
                        tables_of)

pytestmark = pytest.mark.gpu

WIDE = ["FruitFeast", "PickyBanana", "BreadSnack", "FruitFeast"]
COOP = dict(COOP12, max_steps=5)
STEP, ROLLOUT_ACTIONS, STEP_CODES, STEP_F32, ROLLOUT_F32 = 0, 2, 3, 6, 7       # StepMode, cz_kernels.h
EP_BLOCK = 256                                                                # k_episodes_collect's block size (cz_api.hip)


class Run:
    """one handle, its oracle twin, the model, the policy and the step buffers"""

    def __init__(self, tables, auto_reset=True, seed=0, capacity=None):
        self.t, self.env = tables, make(tables, auto_reset)
        self.orc = VecOracle.from_vec_env(tables, auto_reset=int(auto_reset))
        self.model = EpisodeModel(tables.num_envs, tables.num_agents, tables.recipe_nodes == 16, tables.env_id_base)
        self.pol = BumperActions(tables.dims, tables.scheme_class.CODE, np.random.default_rng(seed))
        env, n, A = self.env, tables.num_envs, tables.num_agents
        self.act, self.rew = env.alloc((n, A), np.int32), env.alloc((n, A), np.float64)
        self.term, self.trunc = env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)
        self.col = Collector(env, capacity)
        env.reset(return_obs=False); self.orc.reset()
        self.steps = 0

    def oracle_step(self, acts):
        """the oracle's step and the model's; -> (rewards, terminations, truncations)"""
        before = self.orc.records.copy()
        _, rew, term, trunc = self.orc.step(acts, want_obs=False)
        self.model.step(before, self.orc.records, rew)
        self.steps += 1
        return rew, term, trunc

    def step(self, launch=None, acts=None):
        """one step on both sides; `launch(env, run)` issues the device's (default: step_device without observations)"""
        acts = self.pol.act(self.orc.records) if acts is None else acts
        self.act.from_host(acts)
        if launch is None:
            self.env.step_device(self.act, None, self.rew, self.term, self.trunc)
        else:
            launch(self.env, self)
        rew, term, trunc = self.oracle_step(acts)
        self.pol.observe_result(self.orc.records)
        assert np.array_equal(self.rew.to_host().view(np.uint64), rew.view(np.uint64)), f"step {self.steps}: rewards"
        assert np.array_equal(self.trunc.to_host(), trunc) and np.array_equal(self.term.to_host(), term), f"step {self.steps}: flags"

    def close(self):
        assert np.array_equal(strip(self.env.get_state()), self.orc.records), "records at the end of the run"
        self.env.close()


# ---------------------------------------------------------------------------------------------------------------------------
# every kernel family writes the row
# ---------------------------------------------------------------------------------------------------------------------------

def launch_obs64(env, r):
    if not hasattr(r, "obs"):
        r.obs = env.alloc((env.num_envs, env.num_agents, env.F), np.float64)
    env.step_device(r.act, r.obs, r.rew, r.term, r.trunc)


def launch_codes_set(env, r):
    if not hasattr(r, "codes"):
        r.codes = env.alloc((env.num_envs, env.num_agents, env.codes_pitch), np.uint8)
        env.set_compact_output(r.codes)
    env.step_device(r.act, None, r.rew, r.term, r.trunc)


def launch_f32_set(env, r):
    if not hasattr(r, "obs32"):
        r.obs32 = env.alloc((env.num_envs, env.num_agents, env.F), np.float32)
        env.set_f32_output(r.obs32)
    env.step_device(r.act, None, r.rew, r.term, r.trunc)


def launch_codes_call(env, r):
    if not hasattr(r, "codes"):
        r.codes = env.alloc((env.num_envs, env.num_agents, env.codes_pitch), np.uint8)
    env.step_device_compact(r.act, r.codes, r.rew, r.term, r.trunc)


def launch_f32_call(env, r):
    if not hasattr(r, "obs32"):
        r.obs32 = env.alloc((env.num_envs, env.num_agents, env.F), np.float32)
    env.step_device_f32(r.act, r.obs32, r.rew, r.term, r.trunc)


# (name, level, meta, agents, recipes, scheme, max_steps, launch, kernel instance, lean, mode)
FAMILIES = [
    ("lean-2", "coop_test", "example", 2, TWO, "scheme3", 5, launch_obs64, 0, 1, STEP),
    ("lean-1", "coop_test", "example", 1, ["TomatoLettuceSalad"], "scheme3", 3, launch_obs64, 0, 1, STEP),
    ("lean-4", "crowded_6x5", "crowded_6x5", 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], "scheme1", 7,
     launch_obs64, 0, 1, STEP),
    ("codes-set", "coop_test", "example", 2, TWO, "scheme3", 4, launch_codes_set, 0, 0, STEP_CODES),
    ("f32-set", "coop_test", "example", 2, TWO, "scheme3", 6, launch_f32_set, 0, 0, STEP_F32),
    ("codes-call", "crowded_6x5", "crowded_6x5", 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], "scheme3", 5,
     launch_codes_call, 0, 0, STEP_CODES),
    ("f32-call", "dense_8x8", "dense_8x8", 1, ["TomatoSalad"], "scheme1", 4, launch_f32_call, 0, 0, STEP_F32),
    ("wide", "crowded_6x5", "crowded_6x5", 4, WIDE, "scheme3", 6, launch_obs64, 0, 0, STEP),
    ("large", "dense_16x16", "dense_16x16", 2, ["TomatoLettuceOnionSalad", "MashedCarrotBanana"], "scheme1", 4, launch_obs64, 1, 0, STEP),
    ("huge", "huge_20x20", "huge_20x20", 3, ["TomatoLettuceSalad", "MashedCarrotBanana", "TomatoSalad"], "scheme1", 5, launch_obs64, 2, 0, STEP),
]


@pytest.mark.parametrize("name,level,meta,agents,recipes,scheme,max_steps,launch,inst,lean,mode", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_kernel_family_writes_the_row(name, level, meta, agents, recipes, scheme, max_steps, launch, inst, lean, mode):
    """N = 11: one full workgroup and a partial one (8 envs per workgroup; the huge instance: two full ones and a partial one)"""
    if name == "wide":                                                  # the user recipes of test_custom_recipes.py: a graph of 10 nodes
        from cooking_zoo_amd.cooking_book import recipe_drawer as rd
        assert not rd.RECIPE_STORE
        register_fixture_recipes()
    try:
        t = tables_of(11, level, meta, agents, recipes, scheme, max_steps, 3)
    finally:
        if name == "wide":
            rd.RECIPE_STORE.clear()
    assert (t.recipe_nodes == 16) == (name == "wide")
    r = Run(t, seed=len(name))
    assert instance(r.env) == inst
    for k in range(3 * (max_steps + 1) + 2):
        r.step(launch)
        assert (last_lean(r.env), last_mode(r.env)) == (lean, mode), f"{name}: the launch took another kernel"
        r.col.collect(r.model.collect(), f"{name} step {k}")
    assert len(r.model.emitted) >= 3 * 11 and {int(e["episode"]) for e in r.model.emitted} >= {0, 1, 2}
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# fused rollouts
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["rollout_actions", "rollout_f32"])
def test_fused_rollout_finishes_several_episodes_per_launch(form):
    """T > 2 (max_steps + 1): every env finishes more than one episode inside a launch - `finished` counts them, the entry is the last"""
    n, A, ms, T = 11, 2, 4, 13
    t = tables_of(n, **dict(COOP, max_steps=ms))
    r = Run(t, seed=5)
    env = r.env
    d_acts, d_rew = env.alloc((T, n, A), np.int32), env.alloc((T, n, A), np.float64)
    d_obs32 = env.alloc((T, n, A, env.F), np.float32) if form == "rollout_f32" else None
    several = 0
    for launch in range(3):
        if form == "rollout_actions":
            acts = []
            for _ in range(T):
                acts.append(r.pol.act(r.orc.records))
                rew_last = r.oracle_step(acts[-1])[0]
                r.pol.observe_result(r.orc.records)
            d_acts.from_host(np.stack(acts).astype(np.int32))
            env.rollout_actions(d_acts, T, None, d_rew)
            assert last_mode(env) == ROLLOUT_ACTIONS
        else:
            trial = r.orc.records.copy()
            err, _, _, _, _, acts = r.orc.oracle.rollout(trial, T, 77, launch * T, want_obs=False, want_actions=True)
            assert err == 0
            for k in range(T):
                rew_last = r.oracle_step(acts[k])[0]
            env.rollout_f32(T, 77, launch * T, d_obs32, d_rew)
            assert last_mode(env) == ROLLOUT_F32
        assert np.array_equal(d_rew.to_host()[-1].view(np.uint64), rew_last.view(np.uint64)), f"launch {launch}: the last step's rewards"
        want = r.model.collect()
        assert len(want) == n and (want["finished"] >= 2).all()
        several += int((want["finished"] >= 3).sum())
        r.col.collect(want, f"{form} launch {launch}")
    assert several > 0
    r.close()


def test_fused_rollout_episodes_span_launches():
    """T = 4 with max_steps = 6: an episode runs through two launches, its return is carried from one to the next"""
    n, A, T = 11, 2, 4
    t = tables_of(n, **dict(COOP, max_steps=6))
    r = Run(t, seed=6)
    d_acts = r.env.alloc((T, n, A), np.int32)
    sizes = []
    for launch in range(9):
        acts = []
        for _ in range(T):
            acts.append(r.pol.act(r.orc.records))
            r.oracle_step(acts[-1])
            r.pol.observe_result(r.orc.records)
        d_acts.from_host(np.stack(acts).astype(np.int32))
        r.env.rollout_actions(d_acts, T)
        want = r.model.collect()
        sizes.append(len(want))
        assert (want["finished"] == 1).all()
        r.col.collect(want, f"launch {launch}")
    assert sizes.count(0) >= 3 and sizes.count(n) >= 3                  # launches in which nobody finishes, and in which everybody does
    assert all(int(e["length"]) == 6 and e["ret"][0] != 0.0 for e in r.model.emitted)      # (6 steps: never inside one launch of 4)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# both ways to end
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def kat_tables(n, max_steps, wide):
    """the world of golden set kat_c3 (coop_test, one agent, TomatoLettuceSalad; its 30 recorded actions complete the recipe) as a
    one-layout pool.  wide: a second recipe, the 10-node FruitFeast of test_custom_recipes.py, beside it (nobody cooks it; the episode
    ends with the first dish) - the book then has wide tables, and the root marks are bit 0 of 16-bit fields"""
    from cooking_zoo_amd.cooking_book import recipe_drawer as rd
    from cooking_zoo_amd.vec_env import BatchTables
    from golden_io import GoldenSet, layout_from_episode
    gs = GoldenSet("kat_c3")
    ep = gs.episodes[0]
    if wide:
        assert not rd.RECIPE_STORE
        register_fixture_recipes()
        for name in gs.cfg["recipes"]:                                  # (a user store replaces the default book: the dish goes in too)
            rd.register_recipe(rd.RECIPES[name](), name)
    try:
        t = BatchTables(n, gs.cfg["level"], gs.cfg["meta_file"], 1, max_steps, gs.cfg["recipes"] + (["FruitFeast"] if wide else []),
                        bool(gs.cfg["end_condition_all_dishes"]) and not wide, gs.cfg["action_scheme"], gs.cfg.get("reward_scheme"),
                        layouts=[layout_from_episode(ep)])
    finally:
        if wide:
            rd.RECIPE_STORE.clear()
    assert t.recipe_nodes == (16 if wide else 8)
    return t, np.asarray(ep.actions, dtype=np.int32)


def kat_actions(r, trace, ptr, delay):
    """every env walks the golden trace from the start of each of its episodes; in its first episode env e first waits delay[e] steps
    (action 0), so the envs are staggered - and the ones that wait too long are cut off by max_steps before the dish is served"""
    n = len(ptr)
    acts = np.zeros((n, 1), dtype=np.int32)
    done = (r.orc.records[:, soa.W_STATUS] & soa.STATUS_DONE) != 0
    for e in range(n):
        if done[e]:
            ptr[e] = 0                                                # (this step is the env's reset pass: its action is not used)
        elif delay[e] > 0:
            delay[e] -= 1
        elif ptr[e] < len(trace):
            acts[e] = trace[ptr[e]]
            ptr[e] += 1
    return acts


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_terminated_and_truncated_episodes(wide):
    n, ms = 11, 33
    t, trace = kat_tables(n, ms, wide)
    assert len(trace) == 30
    r = Run(t)
    ptr, delay = np.zeros(n, dtype=np.int64), np.arange(n) % 6            # delays 0..5: 30 + delay > 33 for 4 and 5
    for k in range(2 * (ms + 2)):
        r.step(launch_obs64, kat_actions(r, trace, ptr, delay))
        assert last_lean(r.env) == (0 if wide else 1)
        r.col.collect(r.model.collect(), f"step {k}")
    flags = np.array([int(e["flags"]) for e in r.model.emitted])
    served = (flags & 1 != 0) & (flags & 16 != 0)
    assert served.sum() >= n and ((flags & 2 != 0) & (flags & 16 == 0)).sum() >= 2, flags.tolist()
    assert {int(e["length"]) for e, s in zip(r.model.emitted, served) if s} >= {30, 31, 32, 33}
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# despawn / respawn
# ---------------------------------------------------------------------------------------------------------------------------

def test_an_agent_truncated_by_despawn_produces_no_record():
    t = tables_of(11, agent_despawn_rate=0.15, agent_respawn_rate=0.3, grace_period=2, spawn_seed=4, **dict(COOP, max_steps=7))
    r = Run(t, seed=9)
    assert r.orc.oracle.ctx.spawn
    lone = 0                       # steps on which an agent was reported truncated although its env's episode went on
    for k in range(40):
        before = r.orc.records.copy()
        r.step(launch_obs64)
        stepped = (before[:, soa.W_STATUS] & soa.STATUS_DONE) == 0
        went_on = stepped & ((r.orc.records[:, soa.W_STATUS] & soa.STATUS_DONE) == 0)
        lone += int((r.trunc.to_host().any(axis=1) & went_on).sum())
        assert last_lean(r.env) == 0
        r.col.collect(r.model.collect(), f"step {k}")
    assert lone >= 10 and len(r.model.emitted) >= 3 * 11
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# auto_reset = False with reset_device
# ---------------------------------------------------------------------------------------------------------------------------

def test_frozen_envs_masked_resets_and_reset_stats():
    n = 11
    t = tables_of(n, **COOP)                                            # max_steps = 5: everybody starts together and ends at step 5
    r = Run(t, auto_reset=False, seed=3)
    env, mask = r.env, r.env.alloc((n,), np.uint8)

    def reset(chosen=None):
        """reset_device on both sides: the finished envs (no mask) or the chosen ones, finished or not"""
        done = (r.orc.records[:, soa.W_STATUS] & soa.STATUS_DONE) != 0
        which = np.nonzero(done)[0] if chosen is None else chosen
        if chosen is not None:
            m = np.zeros(n, dtype=np.uint8)
            m[chosen] = 1
            mask.from_host(m)
        env.reset_device(None if chosen is None else mask)
        for e in which:
            if not done[e]:
                r.model.abort(int(e))
            oracle_reset(r.orc, int(e))

    found = []
    for k in range(8):                                                  # steps 6, 7, 8: everybody is frozen, and was reported at step 5
        r.step()
        want = r.model.collect()
        found.append(len(want))
        r.col.collect(want, f"step {k}")
    assert found == [0, 0, 0, 0, n, 0, 0, 0]
    reset()
    r.step(); r.step()
    r.col.collect(r.model.collect(), "two steps into the second episode")
    cut = np.array([1, 4, 7])
    reset(cut)                                                          # cut short in mid-episode: no record
    r.col.collect(r.model.collect(), "behind the masked reset")
    sizes = []
    for k in range(5):                                                  # the others end after 3 more steps, the three after 5
        r.step()
        want = r.model.collect()
        sizes.append(sorted((want["env"]).tolist()))
        r.col.collect(want, f"second episode, step {k}")
    assert sizes == [[], [], [e for e in range(n) if e not in cut], [], cut.tolist()]
    late = [e for e in r.model.emitted if int(e["env"]) in cut and int(e["episode"]) >= 1]
    assert len(late) == 3 and all(int(e["length"]) == 5 and int(e["episode"]) == 2 for e in late)        # (the cut episode was index 1)
    # reset_stats empties what is pending
    reset()
    for _ in range(5):
        r.step()
    assert len(r.model.pending) == n
    env.reset_stats(); r.model.clear()
    r.col.collect(r.model.collect(), "behind reset_stats")
    reset()
    for k in range(5):
        r.step()
    want = r.model.collect()
    assert len(want) == n
    r.col.collect(want, "the first episodes behind reset_stats")
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the packed list
# ---------------------------------------------------------------------------------------------------------------------------

def test_packed_list_order_capacity_and_guards():
    n = 2 * EP_BLOCK + 37
    ms = 6
    t = tables_of(n, **dict(COOP, max_steps=ms))
    r = Run(t, seed=12)
    env, mask = r.env, r.env.alloc((n,), np.uint8)
    r.col.collect(r.model.collect(), "nobody has finished")             # count 0, the list untouched
    for k in range(ms):                                                 # everybody at once: same max_steps, same start
        r.step()
        want = r.model.collect()
        assert len(want) == (n if k == ms - 1 else 0)
        r.col.collect(want, f"together, step {k}")
    r.step()                                                            # (the reset pass)
    sparse = np.array(sorted(set(np.random.default_rng(1).choice(n, 40, replace=False).tolist()) | {0, 255, 256, 511, 512, n - 1}))
    for k in range(3):
        r.step()
    m = np.zeros(n, dtype=np.uint8)
    m[sparse] = 1
    mask.from_host(m)
    env.reset_device(mask)                                              # the sparse set starts over: it will end three steps behind the rest
    for e in sparse:
        r.model.abort(int(e))
        oracle_reset(r.orc, int(e))
    r.col.collect(r.model.collect(), "nobody has finished yet")
    events = []
    for k in range(3 * (ms + 1) + 4):
        r.step()
        want = r.model.collect()
        if len(want) == 0:
            r.col.collect(want, f"step {k}: nobody")
            continue
        kind = len(events) % 4
        events.append((kind, len(want)))
        if kind in (0, 1):                                              # everything, list and dense arrays
            r.col.collect(want, f"step {k}: everything")
        elif kind == 2:                                                 # capacity = count - 1: the first entries, the whole count; all of them seen
            r.col.collect(want, f"step {k}: capacity {len(want) - 1}", capacity=len(want) - 1)
            r.col.collect(want[:0], f"step {k}: the collect behind it")
        else:                                                           # all outputs null: the call marks
            env.collect_episodes()
            r.col.collect(want[:0], f"step {k}: behind a collect without outputs")
        assert (np.diff(want["env"]) > 0).all()
    sizes = {c for _, c in events}
    assert n - len(sparse) in sizes and len(sparse) in sizes and len(events) >= 6, events
    # the list alone, the count alone, the dense arrays alone
    for k in range(ms + 1):
        r.step()
    r.col.collect(r.model.collect(), "list alone", dense=False, count=False)
    for k in range(ms + 1):
        r.step()
    want = r.model.collect()
    r.col.collect(want, "count alone", dense=False, packed=False)
    for k in range(ms + 1):
        r.step()
    r.col.collect(r.model.collect(), "dense arrays alone", packed=False, count=False)
    assert len(want) == n
    r.close()


def test_count_and_order_at_the_largest_batch():
    """N = 131 072, the largest batch the call must be right for: 512 blocks, so every thread adds up two of the per-block totals.
    No oracle at this size: with max_steps = 2 every env is truncated at its second step whatever happens in it, so who is found, the
    lengths, flags, episode words and the order follow from the configuration; the returns are the device's own rewards of the two
    steps, added here with np.float64 adds (tests at small N check those rewards against the oracle)."""
    n, A = 131072, 2
    env = make(tables_of(n, **dict(COOP, max_steps=2)), auto_reset=False)
    env.reset(return_obs=False)
    act, rew = env.alloc((n, A), np.int32), env.alloc((n, A), np.float64)
    term, trunc, mask = env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8), env.alloc((n,), np.uint8)
    act.from_host(np.random.default_rng(3).integers(0, env.n_actions, (n, A)).astype(np.int32))
    col = Collector(env)

    def two_steps():
        total = np.zeros((n, A))
        for _ in range(2):
            env.step_device(act, None, rew, term, trunc)
            total += rew.to_host()
        return total

    def entries(which, episode, total):
        want = np.zeros(len(which), dtype=EP)
        want["env"], want["episode"], want["length"], want["flags"], want["finished"] = which, episode, 2, 2, 1
        want["ret"][:, :A] = total[which]
        return want

    col.collect(entries(np.arange(0), 0, np.zeros((n, A))), "nobody")
    total = two_steps()
    assert trunc.to_host().all() and not term.to_host().any()
    col.collect(entries(np.arange(n), 0, total), "everybody")
    col.collect(entries(np.arange(0), 0, total), "everybody, the collect behind it")
    # a sparse set that reaches into the first and the last block, and both sides of the block whose total the second loop round adds
    rng = np.random.default_rng(5)
    sparse = np.array(sorted(set(rng.choice(n, 300, replace=False).tolist()) | {0, 255, 256, 65535, 65536, 65791, 65792, n - 1}))
    m = np.zeros(n, dtype=np.uint8)
    m[sparse] = 1
    mask.from_host(m)
    env.reset_device(mask)
    total = two_steps()                                                 # (the others are frozen: reward 0, and no second record)
    col.collect(entries(sparse, 1, total), "a sparse set", capacity=len(sparse) - 1)
    col.collect(entries(np.arange(0), 1, total), "a sparse set, the collect behind it")
    env.close()


def test_finished_episodes_host_form():
    n = 37
    t = tables_of(n, env_id_base=1000, **COOP)
    r = Run(t, seed=2)
    assert r.env.finished_episodes().shape == (0,)
    seen = 0
    for k in range(14):
        r.step()
        got, want = r.env.finished_episodes(), r.model.collect()
        assert got.dtype == EP and same_entries(got, want), f"step {k}:\n got {got}\nwant {want}"
        seen += len(want)
    assert seen >= 2 * n and int(want["env"].min() if len(want) else 1000) >= 1000
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------
# inside a capture
# ---------------------------------------------------------------------------------------------------------------------------

def test_step_and_collect_inside_a_callers_capture():
    n, R = 300, 24
    t = tables_of(n, **dict(COOP, max_steps=5, num_layouts=8))
    env, ref = make(t), make(t)
    rng = np.random.default_rng(8)

    class B:
        def __init__(self, e):
            A = e.num_agents
            self.act, self.rew = e.alloc((n, A), np.int32), e.alloc((n, A), np.float64)
            self.term, self.trunc, self.obs32 = e.alloc((n, A), np.uint8), e.alloc((n, A), np.uint8), e.alloc((n, A, e.F), np.float32)
            self.col = Collector(e)
            self.col.fill()

    def issue(e, b):
        e.step_device_f32(b.act, b.obs32, b.rew, b.term, b.trunc)
        c = b.col
        e.collect_episodes(c.mask, c.ret, c.length, c.flags, c.list, c.cap, c.count)

    be, br = B(env), B(ref)
    for e in (env, ref):
        e.reset(return_obs=False)
    cs = CallerStream(env)
    with cs.capture():
        issue(env, be)                                                  # [step, collect]: captured, not executed
    assert last_mode(env) == STEP_F32
    assert np.array_equal(env.get_state(), ref.get_state()), "capturing must not have stepped anything"
    total = 0
    for k in range(R):
        acts = rng.integers(0, env.n_actions, (n, env.num_agents)).astype(np.int32)
        be.act.from_host(acts); br.act.from_host(acts)
        be.col.fill(); br.col.fill()
        cs.replay()
        cs.sync()
        issue(ref, br)
        g, w = be.col.read(), br.col.read()
        for name in g:
            assert np.array_equal(g[name], w[name]), f"replay {k}: {name}"
        total += int(w["count"][0])
    assert total >= 3 * n
    assert np.array_equal(env.get_state(), ref.get_state()) and env.stats()["episodes"] == total
    cs.close()
    env.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# shards
# ---------------------------------------------------------------------------------------------------------------------------

def test_three_unequal_shards_equal_one_handle():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from episodes_common import SENT64, SENT_FLAGS, SENT_LEN, SENT_MASK
    n, A = 37, 2
    many = ShardedVecEnv(n, COOP["level"], COOP["meta"], A, COOP["max_steps"], TWO, action_scheme="scheme3", num_layouts=3, device_ids=[0, 0, 0])
    assert sorted(c for _, c in many.ranges) == [12, 12, 13]
    r = Run(tables_of(n, **COOP), seed=4)
    one = r.env
    act, rew, term, trunc = many.alloc((A,), np.int32), many.alloc((A,), np.float64), many.alloc((A,), np.uint8), many.alloc((A,), np.uint8)
    mask, ret, length, flags = many.alloc((), np.uint8), many.alloc((A,), np.uint64), many.alloc((), np.int32), many.alloc((), np.uint32)
    # the packed list has no env axis: one list of `capacity` entries and one count per local shard, as sequences of the shards' buffers
    d_list = [env.alloc((13,), _native.EPISODE_DTYPE) for env in many.shards]
    d_count = [env.alloc((1,), np.int32) for env in many.shards]
    many.reset(return_obs=False)
    found = 0
    for k in range(16):
        acts = r.pol.act(r.orc.records)
        act.from_host(acts)
        many.step_device(act, None, rew, term, trunc)
        r.step(acts=acts)
        want = r.model.collect()
        found += len(want)
        if k % 2:                                                       # the host form: the shards' lists joined in shard order
            got = many.finished_episodes()
            assert same_entries(got, want) and same_entries(one.finished_episodes(), want), f"step {k}:\n got {got}\nwant {want}"
            continue
        for buf, sent in ((mask, SENT_MASK), (ret, SENT64), (length, SENT_LEN), (flags, SENT_FLAGS)):
            buf.from_host(np.full((n,) + buf.per_env, sent, dtype=buf.dtype))
        many.collect_episodes(mask, ret, length, flags, d_list, 13, d_count)
        single = r.col.collect(want, f"step {k}: the single handle")     # (every array of it against the model, guards included)
        for buf, name in ((mask, "mask"), (ret, "ret"), (length, "length"), (flags, "flags")):
            assert np.array_equal(buf.to_host().reshape(-1), single[name][:buf.to_host().size]), f"step {k}: {name} of the shards"
        counts = [int(c.to_host()[0]) for c in d_count]
        lists = [l.to_host()[:c] for l, c in zip(d_list, counts)]
        assert same_entries(np.concatenate(lists), want), f"step {k}: the shards' packed lists, joined"
    assert found >= 2 * n
    many.close(); r.close()
