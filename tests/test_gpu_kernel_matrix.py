"""GPU: every step-path kernel instantiation against the oracle, bit for bit, with a ledger of what was launched.

The library ships k_step<OPL, CPL, NA, SCHEME, MODE> for 3 instances x 4 agent counts x 2 schemes x 7 modes, k_step_lean for the 8
(agents, scheme) pairs of the small instance, and k_reset / k_observe / k_observe_f32 per instance and agent count; Inst::step picks
among them from run-time values.  The other tests reach that space through hand-picked lists.  This module walks it: 24 cells
(instance x agents x scheme), each the same small world - crowded_6x5, natural D = 6, F = 128, 35 envs so that the last workgroup is
partly empty at 8 and at 4 envs per workgroup - on the instance that max_dyn = None | 65 | 129 selects, and in every cell

  pass A  plain settings: one handle walks one continuous trajectory against one natural-D oracle, cut into seven segments of 30
          steps, one launch form per segment (cz_step_device, cz_step_device_compact, cz_step_device_f32, cz_rollout_actions,
          cz_rollout, cz_rollout_compact with and without a float64 trajectory), the order rotated by the cell's index; fused
          segments go out as two launches of 15 steps.  On the small instance cz_step_device must be the lean kernel, and a twin
          handle made under CZ_LEAN=0 replays that segment from the records at its start through the generic k_step<..., STEP>:
          the same bytes.
  pass B  wide recipe tables (marks of recipes 2 and 3 in W_MARKS_HI) with despawn / respawn on (per-agent grace fields in the
          status word): the same seven forms in segments of 24 steps; never the lean kernel.

Every output buffer holds 0xFF bytes (codes: the real code 7, float32 rows: a quiet-NaN sentinel with a guard region behind them)
before every launch; float64 compares as uint64, float32 rows as uint32 against np.float32 of the oracle's rows, codes decode through
obs_table() with padding bytes 255, records compare word for word with the oracle's widened to the padded D - and the running-return
words, which the oracle does not keep, with a float64 model (+= reward per step, zero at episode end).  No tolerance anywhere.
After reset and after pass A's third segment cz_observe_device / cz_observe_device_f32 write a window of the batch in every form;
at the end of each pass cz_get_stats equals, all four columns and bit for bit, a model made from the oracle's run alone.

After every launch cz_diag_last_step_mode / cz_diag_last_step_lean say which kernel it took; a cell asserts the set it saw, and the
last test that the union over the cells is all 176 (instance, agents, scheme, mode | lean).  The conditions that keep a cell from
passing vacuously (episodes finished, objects moved, inexact float32 elements, agents gone, marks set in either word) are asserted
on the oracle's run, never on the device's; their floors are about half of what the oracle gave on the CPU (profiles/r13/README.md)."""
import numpy as np
import pytest

from cooking_zoo_amd import soa
from fuzz_policy import BumperActions
from oracle_binding import VecOracle
from host_common import register_fixture_recipes
from vec_common import (SENTINEL, GuardedRows, Outs, bits, check_step, instance, junk, last_lean, last_mode, lean, make_env as make, strip,
                        want32, widen)

pytestmark = pytest.mark.gpu

N, LAYOUTS, LEVEL, META, MAX_STEPS = 35, 8, "crowded_6x5", "crowded_6x5", 20
WINDOW = (5, 9)                                                  # env_begin, env_count of the observe checks
INSTANCES = [(None, 0), (65, 1), (129, 2)]                       # (max_dyn, instance); None: the level's own D = 6
CELLS = [(inst, agents, scheme) for inst in range(3) for agents in (1, 2, 3, 4) for scheme in ("scheme3", "scheme1")]

STEP, ROLLOUT, ROLLOUT_ACTIONS, STEP_CODES, ROLLOUT_CODES, ROLLOUT_CODES_ONLY, STEP_F32 = range(7)          # StepMode, cz_kernels.h
VARIANTS = [("cz_step_device", STEP), ("cz_step_device_compact", STEP_CODES), ("cz_step_device_f32", STEP_F32),
            ("cz_rollout_actions", ROLLOUT_ACTIONS), ("cz_rollout", ROLLOUT), ("cz_rollout_compact beside float64", ROLLOUT_CODES),
            ("cz_rollout_compact", ROLLOUT_CODES_ONLY)]
FUSED = (ROLLOUT, ROLLOUT_ACTIONS, ROLLOUT_CODES, ROLLOUT_CODES_ONLY)
DEVICE_STREAM = (ROLLOUT, ROLLOUT_CODES, ROLLOUT_CODES_ONLY)     # the launch draws its own actions (keyed by seed, env id, agent, step)

PASS_A = dict(name="A", recipes=["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], segment=30, seed=140, wide=False, kw={})
PASS_B = dict(name="B", recipes=["FruitFeast", "PickyBanana", "BreadSnack", "FruitFeast"], segment=24, seed=206, wide=True,
              kw=dict(agent_despawn_rate=0.1, agent_respawn_rate=0.3, grace_period=2, spawn_seed=5))

# (seed + agents drives the policy and the on-device action stream.  With the bases 100 and 200 the oracle's run missed two floors at
# max_steps = 20 - 0, 1 and 4 terminations per instance, W_MARKS set on 56 env-steps of one cell - so the bases were changed, not the floors.)

LEDGER = {}               # (instance, agents, scheme) -> {(mode, lean)} over both passes; a cell enters when it starts
TERMINATIONS = {}         # (instance, agents, scheme) -> terminations of the oracle's pass A


def rotated(k):
    k %= len(VARIANTS)
    return VARIANTS[k:] + VARIANTS[:k]


class OracleRun:
    """The oracle's side of one pass: the natural-D twin of the cell's batch (device-free tables), the policy, and what is made
    from its run alone - the statistics model and the counters of the vacuity conditions."""

    def __init__(self, agents, scheme, ps):
        from cooking_zoo_amd.vec_env import BatchTables
        self.ps, self.A = ps, agents
        self.tables = BatchTables(N, LEVEL, META, agents, MAX_STEPS, ps["recipes"][:agents], action_scheme=scheme, num_layouts=LAYOUTS, **ps["kw"])
        self.dn = self.tables.dims
        assert (self.dn.W, self.dn.H, self.dn.D, self.tables.F) == (6, 5, 6, 128)
        assert self.tables.recipe_nodes == (16 if ps["wide"] else 8)
        self.orc = VecOracle.from_vec_env(self.tables)
        self.seed = ps["seed"] + agents
        self.pol = BumperActions(self.dn, self.tables.scheme_class.CODE, np.random.default_rng(self.seed))
        self.cur, self.fin = np.zeros((N, 4)), np.zeros((N, 4))          # running return; sum of finished episodes' returns, in order
        self.ints = dict(env_steps=0, episodes=0, length_sum=0, truncations=0, terminations=0)
        self.completed = [0] * 4
        self.episodes_of = np.zeros(N, np.int64)
        self.counts = dict(objects_changed=0, gone=0, marks=0, marks_hi=0, f32_elements=0, f32_inexact=0)

    def reset(self):
        obs = self.orc.reset()
        return obs, self.orc.records.copy(), self.cur.copy()

    def step(self, acts):
        """-> (observation, rewards, terminations, truncations, records, running returns) after the step"""
        orc, d, A = self.orc, self.dn, self.A
        before = orc.records.copy()
        obs, rew, term, trunc = orc.step(acts)
        after = orc.records
        # the statistics the device keeps (stats_from_oracle_run of test_gpu_rollout.py, vectorised; the episode's end flags are read
        # from the status word: with despawn / respawn on, an agent's truncation flag is also set on the step it leaves)
        stepped = (before[:, soa.W_STATUS] & soa.STATUS_DONE) == 0             # (a finished env's launch step is its reset pass)
        ended = stepped & ((after[:, soa.W_STATUS] & soa.STATUS_DONE) != 0)
        self.cur[stepped, :A] += rew[stepped]
        self.fin[ended] += self.cur[ended]
        self.cur[ended] = 0.0
        st = self.ints
        st["env_steps"] += int(stepped.sum())
        st["episodes"] += int(ended.sum())
        st["length_sum"] += int(after[ended, soa.W_T].sum())
        st["truncations"] += int(((after[ended, soa.W_STATUS] & soa.STATUS_TRUNC) != 0).sum())
        st["terminations"] += int(((after[ended, soa.W_STATUS] & soa.STATUS_TERM) != 0).sum())
        marks = after[:, soa.W_MARKS].astype(np.uint64)
        if self.ps["wide"]:
            marks |= after[:, soa.W_MARKS_HI].astype(np.uint64) << np.uint64(32)
        for a in range(A):                                               # the root node of recipe a: bit 8a, wide tables bit 16a
            self.completed[a] += int(((marks[ended] >> np.uint64((16 if self.ps["wide"] else 8) * a)) & np.uint64(1)).sum())
        self.episodes_of += ended
        # the vacuity counters
        c, dyn = self.counts, slice(d.dyn0_word0, d.dyn1_word0 + d.D)
        c["objects_changed"] += int((stepped & (before[:, dyn] != after[:, dyn]).any(axis=1)).sum())
        c["gone"] += int((((after[:, soa.W_STATUS] >> 8) & 0xF) != 0).sum())
        c["marks"] += int((after[:, soa.W_MARKS] != 0).sum())
        c["marks_hi"] += int((after[:, soa.W_MARKS_HI] != 0).sum())
        return obs.copy(), rew.copy(), term.copy(), trunc.copy(), after.copy(), self.cur.copy()

    def advance(self, mode, T, t0):
        """T steps of the variant's action source -> (actions [T][N][A], per step what `step` returns)"""
        if mode in DEVICE_STREAM:
            trial = self.orc.records.copy()
            err, _, _, _, _, acts = self.orc.oracle.rollout(trial, T, self.seed, t0, want_obs=False, want_actions=True)
            assert err == 0
            wants = [self.step(acts[t]) for t in range(T)]
            assert np.array_equal(trial, self.orc.records)               # the oracle's rollout and its steps over those actions agree
            return acts, wants
        acts, wants = [], []
        for _ in range(T):
            acts.append(self.pol.act(self.orc.records))
            wants.append(self.step(acts[-1]))
            self.pol.observe_result(self.orc.records)
        return np.stack(acts).astype(np.int32), wants

    def note_f32(self, wants):
        for w in wants:
            self.counts["f32_elements"] += w[0].size
            self.counts["f32_inexact"] += int((w[0].astype(np.float32).astype(np.float64) != w[0]).sum())

    def observe(self, begin, count):
        return np.stack([self.orc.oracle.observe(self.orc.records[e]) for e in range(begin, begin + count)])

    def stats(self):
        """what cz_get_stats must return: the per-env sums, env e in chain e of 256, through the binary tree of the reduction
        (test_stats_reduction_order_and_size in test_gpu_large.py)"""
        level = np.zeros((256, 4))
        level[:N] += self.fin
        while level.shape[0] > 1:
            half = level.shape[0] // 2
            level = level[:half] + level[half:]
        return dict(self.ints, recipes_completed=list(self.completed), return_sum=[float(v) for v in level[0]])

    def assert_not_vacuous(self):
        c, A = self.counts, self.A
        if not self.ps["wide"]:
            assert int(self.episodes_of.min()) >= 8, f"an env finished only {int(self.episodes_of.min())} episodes"
            assert c["objects_changed"] >= 1000, c
            assert c["f32_inexact"] >= 0.25 * c["f32_elements"] > 0, c
        else:
            assert c["gone"] >= 500 if A >= 2 else c["gone"] == 0, c
            assert c["marks"] >= 75, c
            assert A < 3 or c["marks_hi"] >= 8, c


def drive(run, cell, dev=None, after_third=None):
    """the pass: the seven variants in the cell's order, fused ones as two launches; dev = None walks the oracle alone"""
    segment, t = run.ps["segment"], 0
    for s, (name, mode) in enumerate(rotated(cell)):
        for T in ([segment // 2] * 2 if mode in FUSED else [segment]):
            acts, wants = run.advance(mode, T, t)
            if mode == STEP_F32:
                run.note_f32(wants)
            if dev is not None:
                dev.launch(name, mode, acts, wants, t)
            t += T
        if s == 2 and after_third is not None:
            after_third()
    return t


def check_records(ctx, env, want, dn, got=None):
    got = env.get_state() if got is None else got
    assert np.array_equal(strip(got), widen(want[4], dn, env.dims)), f"{ctx}: records"
    ret = np.ascontiguousarray(got[:, soa.RET_WORD0:soa.RET_WORD0 + 8]).view(np.uint64)
    assert np.array_equal(ret, want[5].view(np.uint64)), f"{ctx}: running returns"


class Device:
    """the device's side of one pass: the handle, its buffers, one `launch` per launch of `drive`"""

    def __init__(self, env, run, seen, lean_step, twin=None):
        self.env, self.run, self.seen, self.lean_step, self.twin = env, run, seen, lean_step, twin
        n, A, F, Fp, Tc = N, env.num_agents, env.F, env.codes_pitch, run.ps["segment"] // 2
        assert Fp % 16 == 0 and F <= Fp < F + 16
        self.table = env.obs_table()
        self.outs, self.outs_no_obs = Outs(env), Outs(env, skip=("obs",))
        self.codes, self.rows = env.alloc((n, A, Fp), np.uint8), GuardedRows(env)
        self.spec = [((Tc, n, A, F), np.float64), ((Tc, n, A), np.float64), ((Tc, n, A), np.uint8), ((Tc, n, A), np.uint8)]
        self.traj = [env.alloc(s, t) for s, t in self.spec]
        self.traj_act, self.traj_codes = env.alloc((Tc, n, A), np.int32), env.alloc((Tc, n, A, Fp), np.uint8)

    def note(self, env, ctx, mode, lean_flag=0):
        got = (last_mode(env), last_lean(env))
        self.seen.add(got)
        assert got == (mode, lean_flag), f"{ctx}: the launch took (mode, lean) = {got}, not {(mode, lean_flag)}"

    def decoded(self, ctx, codes):
        F = self.env.F
        assert (codes[..., F:] == 255).all(), f"{ctx}: padding bytes"
        return self.table[codes[..., :F]]

    def launch(self, name, mode, acts, wants, t0):
        env, dn = self.env, self.run.dn
        where = f"pass {self.run.ps['name']} {name}"
        if mode in FUSED:
            self.fused(where, mode, acts, wants, t0)
            return
        start = env.get_state() if mode == STEP and self.twin is not None else None
        kept = []
        for k, (a, want) in enumerate(zip(acts, wants)):
            ctx = f"{where} step {t0 + k}"
            if mode == STEP:
                got = self.outs.step(env, a)
                self.note(env, ctx, STEP, self.lean_step)
            elif mode == STEP_CODES:
                o = self.outs_no_obs
                o.fill()
                self.codes.from_host(np.full(self.codes.shape, 7, np.uint8))      # (a real code: 255 would read as 0.0, the padding value)
                o.act.from_host(a)
                env.step_device_compact(o.act, self.codes, o.buf["rew"], o.buf["term"], o.buf["trunc"])
                self.note(env, ctx, STEP_CODES)
                got = (self.decoded(ctx, self.codes.to_host()),) + o.get()[1:]
            else:
                o = self.outs_no_obs
                o.fill()
                self.rows.fill()
                o.act.from_host(a)
                env.step_device_f32(o.act, self.rows, o.buf["rew"], o.buf["term"], o.buf["trunc"])
                env.sync()
                self.note(env, ctx, STEP_F32)
                bad = np.argwhere(self.rows.rows() != want32(want[0]))
                assert not len(bad), f"{ctx}: float32 observation differs at {bad[:6].tolist()}"
                got = o.get()
            check_step(ctx, got, want)
            state = env.get_state()
            check_records(ctx, env, want, dn, state)
            kept.append((got, state))
        if start is not None:
            self.replay_on_twin(where, start, acts, kept, t0)

    def replay_on_twin(self, where, start, acts, kept, t0):
        """the generic k_step<1, 1, NA, S, STEP> over the segment the lean kernel has just walked: the same bytes"""
        twin = self.twin
        twin.reset(return_obs=False)
        twin.set_state(start)
        o = Outs(twin)
        for k, (a, (got, state)) in enumerate(zip(acts, kept)):
            ctx = f"{where} step {t0 + k}, the CZ_LEAN=0 twin"
            again = o.step(twin, a)
            self.note(twin, ctx, STEP, 0)
            for x, y, what in zip(again, got, ("observation", "rewards", "terminations", "truncations")):
                assert x.tobytes() == y.tobytes(), f"{ctx}: {what} differ from the lean kernel's"
            assert np.array_equal(twin.get_state(), state), f"{ctx}: records differ from the lean kernel's"

    def fused(self, where, mode, acts, wants, t0):
        env, run = self.env, self.run
        T = len(wants)
        assert T == self.spec[0][0][0]
        for b, (s, t) in zip(self.traj, self.spec):
            b.from_host(junk(s, t))
        d_obs, d_rew, d_term, d_trunc = self.traj
        if mode in (ROLLOUT_CODES, ROLLOUT_CODES_ONLY):
            self.traj_codes.from_host(np.full(self.traj_codes.shape, 7, np.uint8))
        if mode == ROLLOUT_ACTIONS:
            self.traj_act.from_host(acts)
            env.rollout_actions(self.traj_act, T, d_obs, d_rew, d_term, d_trunc)
        elif mode == ROLLOUT:
            env.rollout(T, run.seed, t0, d_obs, d_rew, d_term, d_trunc)
        else:
            env.rollout_compact(T, run.seed, t0, self.traj_codes, d_obs if mode == ROLLOUT_CODES else None, d_rew, d_term, d_trunc)
        env.sync()
        self.note(env, f"{where} steps {t0}..{t0 + T - 1}", mode)
        obs, rew, term, trunc = (b.to_host() for b in self.traj)
        codes = self.traj_codes.to_host() if mode in (ROLLOUT_CODES, ROLLOUT_CODES_ONLY) else None
        if mode == ROLLOUT_CODES_ONLY:
            assert (obs.view(np.uint8) == 0xFF).all(), f"{where}: a codes-only launch wrote float64 rows"
        for k, want in enumerate(wants):
            ctx = f"{where} step {t0 + k}"
            if mode != ROLLOUT_CODES_ONLY:
                check_step(ctx, (obs[k], rew[k], term[k], trunc[k]), want)
            if codes is not None:
                check_step(f"{ctx} (codes)", (self.decoded(ctx, codes[k]), rew[k], term[k], trunc[k]), want)
        check_records(f"{where} after step {t0 + T - 1}", env, wants[-1], run.dn)


def check_observe(env, run, when):
    """k_observe / k_observe_f32 on a window of the batch, every form: Oracle.observe of the oracle's records, and nothing outside"""
    begin, count = WINDOW
    n, A, F, Fp = N, env.num_agents, env.F, env.codes_pitch
    want, table = run.observe(begin, count), env.obs_table()
    d_obs, d_codes, rows = env.alloc((n, A, F), np.float64), env.alloc((n, A, Fp), np.uint8), GuardedRows(env)
    for with_obs, with_codes in ((True, False), (False, True), (True, True)):
        ctx = f"cz_observe_device {when}, {'float64' if with_obs else ''}{' + ' if with_obs and with_codes else ''}{'codes' if with_codes else ''}"
        d_obs.from_host(junk((n, A, F), np.float64))
        d_codes.from_host(np.full((n, A, Fp), 7, np.uint8))
        env.observe_device(d_obs if with_obs else None, d_codes if with_codes else None, env_begin=begin, env_count=count)
        env.sync()
        obs, codes = d_obs.to_host(), d_codes.to_host()
        if with_obs:
            assert np.array_equal(bits(obs[:count]), bits(want)), ctx
        if with_codes:
            assert (codes[:count, :, F:] == 255).all(), f"{ctx}: padding bytes"
            assert np.array_equal(bits(table[codes[:count, :, :F]]), bits(want)), ctx
        assert (obs[0 if not with_obs else count:].view(np.uint8) == 0xFF).all(), f"{ctx}: float64 rows outside the window"
        assert (codes[0 if not with_codes else count:] == 7).all(), f"{ctx}: codes outside the window"
    rows.fill()
    env.observe_device(d_obs32=rows, env_begin=begin, env_count=count)
    env.sync()
    got = rows.rows()
    assert np.array_equal(got[:count], want32(want)), f"cz_observe_device_f32 {when}"
    assert (got[count:] == SENTINEL).all(), f"cz_observe_device_f32 {when}: rows outside the window"
    for b in (d_obs, d_codes, rows.buf):
        b.free()


def check_stats(env, run):
    got, want = env.stats(), run.stats()
    for k in ("env_steps", "episodes", "length_sum", "truncations", "terminations", "recipes_completed"):
        assert got[k] == want[k], f"pass {run.ps['name']} statistics: {k} {got[k]}, the oracle's run gives {want[k]}"
    assert np.array_equal(bits(np.array(got["return_sum"])), bits(np.array(want["return_sum"]))), \
        f"pass {run.ps['name']} statistics: return_sum {got['return_sum']}, the oracle's run gives {want['return_sum']}"


def run_pass(ps, cell, seen):
    inst, agents, scheme = CELLS[cell]
    max_dyn, _ = INSTANCES[inst]
    run = OracleRun(agents, scheme, ps)
    args = (N, LEVEL, META, agents, ps["recipes"][:agents], scheme)
    kw = dict(max_steps=MAX_STEPS, max_dyn=max_dyn, num_layouts=LAYOUTS, **ps["kw"])
    env = make(*args, **kw)
    twin = None
    try:
        assert env.dims.D == (max_dyn or 6) and env.F == 128 and instance(env) == inst, f"max_dyn={max_dyn}: instance {instance(env)}"
        assert env.recipe_nodes == (16 if ps["wide"] else 8)
        assert (last_mode(env), last_lean(env)) == (-1, -1)
        lean_step = 1 if inst == 0 and not ps["wide"] else 0
        if lean_step:
            with lean(False):
                twin = make(*args, **kw)
        # k_reset, then k_observe / k_observe_f32
        obs0, rec0, ret0 = run.reset()
        assert np.array_equal(bits(env.reset()), bits(obs0)), "reset observation"
        check_records("reset", env, (None,) * 4 + (rec0, ret0), run.dn)
        assert (last_mode(env), last_lean(env)) == (-1, -1)
        if not ps["wide"]:
            check_observe(env, run, "after reset")
        dev = Device(env, run, seen, lean_step, twin)
        steps = drive(run, cell, dev, None if ps["wide"] else lambda: check_observe(env, run, "after the third segment"))
        assert steps == 7 * ps["segment"] and instance(env) == inst
        check_stats(env, run)
        run.assert_not_vacuous()
    finally:
        env.close()
        if twin is not None:
            twin.close()
    return run


@pytest.mark.parametrize("cell", range(len(CELLS)), ids=[f"inst{i}-{a}agents-{s}" for i, a, s in CELLS])
def test_every_variant_of_the_cell_matches_the_oracle(cell):
    from cooking_zoo_amd.cooking_book import recipe_drawer as rd
    inst = CELLS[cell][0]
    all_modes = {(mode, 0) for _, mode in VARIANTS}
    LEDGER[CELLS[cell]] = set()
    seen_a, seen_b = set(), set()
    run_a = run_pass(PASS_A, cell, seen_a)
    TERMINATIONS[CELLS[cell]] = run_a.ints["terminations"]
    assert seen_a == (all_modes | {(STEP, 1)} if inst == 0 else all_modes), f"pass A launched {sorted(seen_a)}"
    assert not rd.RECIPE_STORE
    register_fixture_recipes()
    try:
        run_pass(PASS_B, cell, seen_b)
    finally:
        rd.RECIPE_STORE.clear()
    assert seen_b == all_modes, f"pass B launched {sorted(seen_b)}"
    LEDGER[CELLS[cell]] = seen_a | seen_b


def test_zz_pass_a_terminations_per_instance():
    """recipes are completed, not only timed out: the oracle's pass A terminations over the eight cells of an instance"""
    whole = [i for i in range(3) if all(c in TERMINATIONS for c in CELLS if c[0] == i)]
    if not whole:
        pytest.skip("no instance had all of its eight cells run in this session")
    for i in whole:
        total = sum(TERMINATIONS[c] for c in CELLS if c[0] == i)
        assert total >= 5, f"instance {i}: {total} terminations over its eight cells"


def test_zz_all_176_step_kernels_ran():
    if len(LEDGER) < len(CELLS):
        pytest.skip(f"{len(LEDGER)} of {len(CELLS)} cells ran in this session")
    ran = {cell + (("lean",) if lean_flag else (mode,)) for cell, seen in LEDGER.items() for mode, lean_flag in seen}
    want = {cell + (mode,) for cell in CELLS for _, mode in VARIANTS} | {cell + ("lean",) for cell in CELLS if cell[0] == 0}
    assert len(want) == 176
    print(f"step kernels launched: {len(ran & want)} of {len(want)}")
    assert ran == want, f"never launched: {sorted(want - ran, key=str)}; unexpected: {sorted(ran - want, key=str)}"
