"""Action effects and masks on the device (cz_action_effects_device, k_action_effects): exact against `effects.host_effects` over the
oracle on the records read back with get_state - every kernel instance, agent count and both schemes, fresh layouts and records the
device stepped itself; every stored state of the unmodified reference; output subsets, agent sets, ignore sets and ranges with
sentinels and guards; refusals; what the call leaves alone; despawned agents and finished envs; stream order, a caller's graph and
unequal shards."""
import functools

import numpy as np
import pytest

import effects_common as ec
from cooking_zoo_amd import _native, effects, soa
from effects_common import OUTPUT_SUBSETS, OUTPUTS, EffectBufs
from vec_common import INSTANCE_CASES, TWO, CallerStream, instance, make_env, oracle_for, policy, strip

pytestmark = pytest.mark.gpu

# (level, meta, agents, recipes, scheme, kernel instance, device steps): every kernel instance and agent count in both schemes
CASES = [(lv, meta, A, rec, sch, inst, 90 if inst == 2 else 120) for lv, meta, A, rec, _s, inst in INSTANCE_CASES for sch in ("scheme1", "scheme3")]
CASES += [("coop_test", "example", 2, TWO, sch, 0, 200) for sch in ("scheme3", "scheme1")]
CASES += [("switch_test", "example", 2, ["MashedCarrotBanana", "TomatoSalad"], sch, 0, 200) for sch in ("scheme1", "scheme3")]
CASE_IDS = [f"{c[0]}-{c[2]}agents-{c[4]}" for c in CASES]
EVERY = 20


def run(env, bufs, outputs=OUTPUTS, **kw):
    bufs.fill()
    env.action_effects_device(**bufs.args(outputs), **kw)


class Stepper:
    """the device and its oracle twin under the biased-fuzz policy, stepped together through step_device"""

    def __init__(self, env, seed):
        n, A = env.num_envs, env.num_agents
        self.env, self.orc, self.pol = env, oracle_for(env), policy(env, seed)
        env.reset(return_obs=False)
        self.orc.reset()
        self.d_act = env.alloc((n, A), np.int32)
        self.d = dict(rew=env.alloc((n, A), np.float64), term=env.alloc((n, A), np.uint8), trunc=env.alloc((n, A), np.uint8))

    def step(self, count=1):
        for _ in range(count):
            acts = self.pol.act(self.orc.records)
            self.orc.step(acts, want_obs=False)
            self.pol.observe_result(self.orc.records)
            self.d_act.from_host(np.ascontiguousarray(acts, dtype=np.int32))
            self.env.step_device(self.d_act, None, self.d["rew"], self.d["term"], self.d["trunc"])


@functools.lru_cache(maxsize=None)
def run_case(k):
    """one case on the device, checked; -> (scheme code, [(model effects, live rows)]) for the census"""
    level, meta, A, recipes, scheme, inst, steps = CASES[k]
    n = 16
    env = make_env(n, level, meta, A, recipes, scheme, max_steps=steps + 50, num_layouts=4)
    assert instance(env) == inst, "the case runs on another kernel instance"
    assert env.num_actions == (5 if scheme == "scheme3" else 8)
    st = Stepper(env, 7 + k)
    bufs = EffectBufs(env, n)
    out = []
    for t in range(0, steps + 1, EVERY):
        if t:
            st.step(EVERY)
        recs = env.get_state()
        assert np.array_equal(strip(recs), strip(st.orc.records)), f"{CASE_IDS[k]} step {t}: the device's records are not the oracle's"
        want = ec.model(env, recs)
        run(env, bufs)
        bufs.check(f"{CASE_IDS[k]} after {t} device steps", OUTPUTS, want)
        assert np.array_equal(env.get_state(), recs), "the call wrote a record"
        out.append((want, ec.live_rows(recs, A)))
    env.close()
    return env.scheme_class.CODE, out


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_every_instance_agent_count_and_scheme(k):
    """fresh layouts (step 0) and records the device stepped itself, every 20 biased-fuzz steps up to 90 - 200"""
    scheme, out = run_case(k)
    assert any(w[live].any() for w, live in out) and any((w[live][:, 1:] == 0).any() for w, live in out)


def golden_env(ep):
    """an env of the episode's world holding the stored records (the kernel reads cells and objects from the record)"""
    gd = soa.Dims(*ep["dims"])
    recs = ec.golden_records(ep)
    env = make_env(len(recs), ep["level"], ep["meta_file"], gd.A, ep["recipes"], "scheme3" if ep["scheme"] == 3 else "scheme1", max_steps=500,
                   num_layouts=1, max_dyn=gd.D, auto_reset=False)
    assert env.dims.as_tuple() == gd.as_tuple()
    env.reset(return_obs=False)
    env.set_state(recs)
    return env, recs


@functools.lru_cache(maxsize=None)
def run_golden(k):
    ep = ec.golden()["episodes"][k]
    env, recs = golden_env(ep)
    want, raises = ec.golden_effects(ep)
    assert (want[raises] == 0).all()
    bufs = EffectBufs(env, len(recs))
    run(env, bufs)
    bufs.check(f"{ep['set']}: the reference's bytes", OUTPUTS, want)
    env.close()
    return ep["scheme"], want


@pytest.mark.parametrize("k", range(len(ec.golden()["episodes"])))
def test_every_stored_state_of_the_reference(k):
    """tests/golden/effects_ref.json.gz uploaded with set_state: the device gives the unmodified reference's byte for every agent and
    code (0 where the reference raises)"""
    run_golden(k)


def test_census_of_the_modules_cases():
    """per scheme over this module's cases - the device-stepped ones and the reference's states: every code seen with and without
    an effect, every bit set and clear"""
    census = ec.Census()
    for k in range(len(CASES)):
        scheme, out = run_case(k)
        for want, live in out:
            census.add(scheme, want, live)
    for k in range(len(ec.golden()["episodes"])):
        scheme, want = run_golden(k)
        census.add(scheme, want)
    census.check("test_gpu_effects", (1, 3))


@functools.lru_cache(maxsize=None)
def three_agents(n):
    """crowded_6x5 with three agents under scheme1, 80 biased-fuzz steps in: the tables and the oracle's records (do not write)"""
    from vec_common import tables_of
    tables = tables_of(n, "crowded_6x5", "crowded_6x5", 3, ["TomatoSalad", "TomatoLettuceSalad", "MashedCarrotBanana"], "scheme1", 400, 4)
    orc = oracle_for(tables)
    orc.reset()
    from fuzz_policy import BumperActions
    pol = BumperActions(tables.dims, 1, np.random.default_rng(3))
    for _ in range(80):
        orc.step(pol.act(orc.records), want_obs=False)
        pol.observe_result(orc.records)
    recs = orc.records.copy()
    recs.setflags(write=False)
    return tables, recs, ec.model(tables, recs)


def env_with(tables, recs):
    from vec_common import env_of
    env = env_of(tables)
    env.reset(return_obs=False)
    env.set_state(recs)
    return env


def test_output_subsets_agent_sets_and_ignore_sets():
    n = 16
    tables, recs, want = three_agents(n)
    env = env_with(tables, recs)
    bufs = EffectBufs(env, n)
    for outputs in OUTPUT_SUBSETS:
        for agents in range(1, 8):
            run(env, bufs, outputs, agents=agents)
            bufs.check(f"outputs={outputs} agents={agents:#x}", outputs, want, agents=agents)
    for ignore in ec.IGNORES:
        run(env, bufs, ignore=ignore)
        bufs.check(f"ignore={ignore:#x}", OUTPUTS, want, ignore=ignore)
    assert len({effects.mask_of(want, i).tobytes() for i in ec.IGNORES}) == len(ec.IGNORES), "the ignore sets do not tell the masks apart here"
    assert np.array_equal(env.get_state(), recs)
    env.close()


def test_ranges():
    n = 16
    tables, recs, want = three_agents(n)
    env = env_with(tables, recs)
    b = EffectBufs(env, 5)                                               # laid out for 5 envs, the guard right behind them
    run(env, b, env_begin=3, env_count=5)
    b.check("envs 3..7", OUTPUTS, want[3:8])
    run(env, b, env_begin=n - 1, env_count=1)
    b.check("the last env alone", OUTPUTS, np.concatenate([want[n - 1:], want[:4]]), rows=slice(0, 1))
    run(env, b, env_begin=n, env_count=0)
    b.check("an empty tail", (), want[:5])
    run(env, b, agents=0b101, env_begin=6, env_count=3)
    b.check("envs 6..8, agents 0 and 2", OUTPUTS, np.concatenate([want[6:9], want[:2]]), agents=0b101, rows=slice(0, 3))
    env.close()


@pytest.mark.parametrize("n", [1, 549])
def test_batch_sizes(n):
    """one env; 549 envs, which is not a multiple of the step kernel's 8 envs per workgroup"""
    env = make_env(n, "coop_test", "example", 2, TWO, "scheme3", max_steps=100, num_layouts=8)
    st = Stepper(env, 21)
    st.step(30)
    recs = env.get_state()
    bufs = EffectBufs(env, n)
    run(env, bufs)
    bufs.check(f"N = {n}", OUTPUTS, ec.model(env, recs))
    env.close()


def test_refusals_write_nothing():
    n = 16
    tables, recs, want = three_agents(n)
    env = env_with(tables, recs)
    b = EffectBufs(env, n)
    L = _native.lib()
    m, e = b.buf["mask"].ptr, b.buf["effects"].ptr
    for args, msg in (((0, n, 7, 0, None, None), "null"), ((0, 0, 7, 0, None, None), "null"), ((0, n, 0, 0, m, e), "agents"),
                      ((0, n, 8, 0, m, e), "agents"), ((0, n, 0x80000001, 0, m, None), "agents"), ((0, n, 7, 32, m, e), "ignore"),
                      ((0, n, 7, 0x100, None, e), "ignore"), ((10, 7, 7, 0, m, e), "range"), ((-1, 2, 7, 0, m, e), "range"),
                      ((0, n + 1, 7, 0, m, e), "range"), ((n + 1, 0, 7, 0, m, e), "range")):
        assert L.cz_action_effects_device(env._h, *args) != 0, f"{args} was accepted"
        text = L.cz_last_error(env._h).decode()
        assert msg in text, f"{args}: message {text!r}"
    with pytest.raises(_native.NativeError, match="null"):
        env.action_effects_device()
    assert L.cz_action_effects_device(None, 0, n, 7, 0, m, e) != 0
    env.sync()
    b.check("after the refusals", (), want)
    assert L.cz_num_actions(env._h) == 8 and env.num_actions == 8
    assert np.array_equal(env.get_state(), recs)
    env.close()


def test_the_call_leaves_records_statistics_and_episodes_alone():
    """two batches stepped alike through finished episodes, one of them asked for its masks every few steps: records, stats() and
    the episode rows are the same byte for byte"""
    n, outs = 16, []
    for ask in (False, True):
        env = make_env(n, "coop_test", "example", 2, TWO, "scheme3", max_steps=12, num_layouts=4)
        st = Stepper(env, 5)
        bufs = EffectBufs(env, n)
        for t in range(40):
            st.step()
            if ask and t % 3 == 0:
                before, stats = env.get_state(), env.stats()
                run(env, bufs)
                env.sync()
                assert np.array_equal(env.get_state(), before) and env.stats() == stats, f"step {t}: the call changed the records or the statistics"
        outs.append((env.get_state(), env.stats(), env.finished_episodes().tobytes()))
        env.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert outs[0][1]["episodes"] >= n


def test_despawned_agents():
    """coop_test with despawn / respawn on: a despawned agent's row is noop-only, a present agent's row is the model's with the
    absent one at -1"""
    n = 32
    env = make_env(n, "coop_test", "example", 2, TWO, "scheme3", max_steps=200, num_layouts=4, agent_despawn_rate=0.1, agent_respawn_rate=0.3,
                   grace_period=3, spawn_seed=4)
    st = Stepper(env, 11)
    bufs = EffectBufs(env, n)
    gone_rows = beside_gone = 0
    for _ in range(4):
        st.step(15)
        recs = env.get_state()
        assert np.array_equal(strip(recs), strip(st.orc.records))
        want = ec.model(env, recs)
        gone = ~ec.live_rows(recs, 2)
        assert not want[gone].any()
        gone_rows += int(gone.sum())
        beside_gone += int(want[gone.any(axis=1)].any(axis=(1, 2)).sum())
        run(env, bufs)
        bufs.check("despawn / respawn on", OUTPUTS, want)
        mask = bufs.read("mask")[0]
        assert (mask[gone] == [1, 0, 0, 0, 0]).all()
    assert gone_rows > 0 and beside_gone > 0, "no despawned agent, or none with a present neighbour that can do something"
    env.close()


def test_finished_envs():
    """auto_reset off, envs run to their end: finished envs give noop-only rows while their neighbours do not"""
    n = 16
    env = make_env(n, "coop_test", "example", 2, TWO, "scheme3", max_steps=20, num_layouts=4, auto_reset=False)
    st = Stepper.__new__(Stepper)
    st.env, st.orc, st.pol = env, oracle_for(env, auto_reset=0), policy(env, 2)
    env.reset(return_obs=False)
    st.orc.reset()
    st.d_act = env.alloc((n, 2), np.int32)
    st.d = dict(rew=env.alloc((n, 2), np.float64), term=env.alloc((n, 2), np.uint8), trunc=env.alloc((n, 2), np.uint8))
    st.step(20)
    recs = env.get_state()
    assert (recs[:, soa.W_STATUS] & soa.STATUS_DONE).all(), "max_steps did not end every env"
    recs[::2] = env.tables.layouts[0].init_record(env.dims, 0)          # every other env: a fresh world, not finished
    recs[::2, soa.W_RECIPES] = recs[1, soa.W_RECIPES]
    env.set_state(recs)
    want = ec.model(env, recs)
    assert not want[1::2].any() and want[::2].any(axis=(1, 2)).all()
    bufs = EffectBufs(env, n)
    run(env, bufs)
    bufs.check("finished envs beside running ones", OUTPUTS, want)
    assert (bufs.read("mask")[0][1::2] == [1, 0, 0, 0, 0]).all()
    env.close()


def test_stream_order_and_a_callers_graph():
    """step_device then action_effects_device with no synchronise in between gives the mask of the stepped state; inside a caller's
    capture, [action_effects_device -> step_device] replayed 20 times with the actions fixed: after each replay the mask is the
    model's of the state the previous step left"""
    n = 16
    env = make_env(n, "crowded_6x5", "crowded_6x5", 3, ["TomatoSalad", "TomatoLettuceSalad", "MashedCarrotBanana"], "scheme1", max_steps=60,
                   num_layouts=4)
    st = Stepper(env, 13)
    st.step(25)
    bufs = EffectBufs(env, n)
    acts = st.pol.act(st.orc.records)
    st.d_act.from_host(np.ascontiguousarray(acts, dtype=np.int32))
    bufs.fill()
    env.step_device(st.d_act, None, st.d["rew"], st.d["term"], st.d["trunc"])
    env.action_effects_device(**bufs.args(OUTPUTS))                     # (no wait in between)
    st.orc.step(acts, want_obs=False)
    recs = env.get_state()
    assert np.array_equal(strip(recs), strip(st.orc.records))
    bufs.check("behind a step on the stream", OUTPUTS, ec.model(env, recs))
    # the caller's graph
    steps_before = env.stats()["env_steps"]
    cs = CallerStream(env)
    bufs.fill()
    with cs.capture():
        env.action_effects_device(**bufs.args(OUTPUTS))
        env.step_device(st.d_act, None, st.d["rew"], st.d["term"], st.d["trunc"])
    assert (bufs.read("mask")[0] == ec.SENT["mask"]).all(), "capturing executed something"
    assert np.array_equal(env.get_state(), recs)
    for r in range(20):
        before = recs
        cs.replay()
        cs.sync()
        bufs.check(f"replay {r}", OUTPUTS, ec.model(env, before))
        st.orc.step(acts, want_obs=False)
        recs = env.get_state()
        assert np.array_equal(strip(recs), strip(st.orc.records)), f"replay {r}: the captured step"
    cs.close()
    assert env.stats()["env_steps"] - steps_before <= 20 * n
    env.close()


def test_sharded_unequal_shards():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n = 50
    tables, recs, want = three_agents(n)
    sh = ShardedVecEnv(n, "crowded_6x5", "crowded_6x5", 3, 400, ["TomatoSalad", "TomatoLettuceSalad", "MashedCarrotBanana"], device_ids=[0, 0, 0],
                       action_scheme="scheme1", num_layouts=4)
    assert [s.num_envs for s in sh.shards] == [17, 17, 16] and sh.num_actions == 8
    sh.reset(return_obs=False)
    sh.set_state(recs)
    d_m, d_e = sh.alloc((3, 8), np.uint8), sh.alloc((3, 8), np.uint8)
    sh.action_effects_device(d_m, d_e, ignore=effects.TURNED)
    sh.sync()
    assert np.array_equal(d_e.to_host(), want), "effects over the shards differ from the host model"
    assert np.array_equal(d_m.to_host(), effects.mask_of(want, effects.TURNED)), "masks over the shards"
    one = env_with(tables, recs)
    for got, single, w in zip(sh.action_mask(agents=0b110), one.action_mask(agents=0b110), (effects.mask_of(want), want)):
        assert np.array_equal(got, single), "the host convenience over the shards is not one handle's"
        assert np.array_equal(got[:, 1:], w[:, 1:]) and (got[:, 0, 1:] == 0).all() and (got[:, 0, 0] == (1 if w is not want else 0)).all()
    assert one.action_mask(env_count=0)[0].shape == (0, 3, 8)
    one.close()
    sh.close()
