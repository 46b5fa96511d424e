"""GPU: cz_gae_device (k_gae) and cz_logprob_device (k_logprob) against the numpy model of cooking_zoo_amd/targets.py, as bits.

Conventions of test_gpu_policy.py: float32 outputs compared as uint32, a sentinel in every output before every launch, one guard row
in front of and one behind each output that must come back untouched.  The GAE shapes are the smallest that cover partial waves
(1, 37, 111 series), several workgroups (260, 1098 series) and every remainder of T over the rows k_gae loads ahead (T = 1, 2, 7, 8, 16, 33
over blocks of 2, 4, 8 or 16 rows); the extents of both calls are the caller's, so small handles serve every shape."""
import numpy as np
import pytest

from cooking_zoo_amd import _native, targets
from policy_common import PolicyTraj, weights
from targets_common import ACT_OUTSIDE, DONE_BYTES, F32_SENT, GAMMA, LAM, bits32, gae_data, gae_float32, synthetic_logits
from vec_common import COOP, CROWDED4, CallerStream, make_env, tables_of

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (37, 1), (37, 3), (65, 4), (549, 2)]
LENGTHS = (1, 2, 7, 8, 16, 33)


@pytest.fixture(scope="module")
def handles():
    """agents -> a small handle with that many agents (scheme1: 8 actions); 5 -> a two-agent scheme3 handle (5 actions)"""
    envs = {a: make_env(4, "crowded_6x5", "crowded_6x5", a, CROWDED4[:a], "scheme1", max_steps=5) for a in (1, 2, 3, 4)}
    envs[5] = make_env(4, **COOP)
    yield envs
    for env in envs.values():
        env.close()


class Guarded:
    """a float32 output of `rows` rows as uint32 with a guard row on both sides; `.ptr` is row 0 of the output"""

    def __init__(self, env, rows, per_row):
        self.rows, self.per_row = rows, per_row
        self.buf = env.alloc((rows + 2, per_row), np.uint32)
        self.ptr = self.buf.ptr + 4 * per_row
        self.fill()

    def fill(self):
        self.buf.from_host(np.full((self.rows + 2, self.per_row), F32_SENT, np.uint32))

    def get(self, ctx):
        got = self.buf.to_host()
        assert (got[0] == F32_SENT).all() and (got[-1] == F32_SENT).all(), f"{ctx}: a store went outside the output"
        return got[1:-1]

    def untouched(self):
        return bool((self.buf.to_host() == F32_SENT).all())

    def free(self):
        self.buf.free()


def upload(env, *arrays):
    out = []
    for a in arrays:
        if a is None:
            out.append(None)
            continue
        b = env.alloc(a.shape, a.dtype)
        b.from_host(a)
        out.append(b)
    return out


def free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


# ---------------------------------------------------------------------------------------------------------------------------
# GAE
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,A", SHAPES, ids=[f"{n}x{a}" for n, a in SHAPES])
def test_gae_equals_the_host_model(handles, n, A):
    env = handles[A]
    for T in LENGTHS:
        adv, ret = Guarded(env, T, n * A), Guarded(env, T, n * A)
        for flags in ("term", "trunc", "both", "null"):
            r, te, tr, V = gae_data(T, n, A, seed=T, flags="term" if flags == "null" else flags)
            if flags == "null":
                tr = None
            d = upload(env, r, te, tr, V)
            adv.fill()
            ret.fill()
            env.gae_device(T, d[0], d[1], d[2], d[3], adv.ptr, ret.ptr, gamma=GAMMA, lam=LAM, env_count=n)
            env.sync()
            want_adv, want_ret = targets.host_gae(r, te, tr, V, GAMMA, LAM)
            ctx = f"T = {T}, {n} x {A}, {flags}"
            bad = np.argwhere(adv.get(ctx) != bits32(want_adv).reshape(T, -1))
            assert not len(bad), f"{ctx}: advantages differ in bits at (t, series) {bad[:6].tolist()}"
            bad = np.argwhere(ret.get(ctx) != bits32(want_ret).reshape(T, -1))
            assert not len(bad), f"{ctx}: returns differ in bits at (t, series) {bad[:6].tolist()}"
            free(*d)
        adv.free()
        ret.free()


def gae_against_the_model(env, ctx, T, n, A, r, te, tr, V):
    adv, ret = Guarded(env, T, n * A), Guarded(env, T, n * A)
    d = upload(env, r, te, tr, V)
    env.gae_device(T, *d, adv.ptr, ret.ptr, gamma=GAMMA, lam=LAM, env_count=n)
    env.sync()
    want_adv, want_ret = targets.host_gae(r, te, tr, V, GAMMA, LAM)
    for o, w, name in ((adv, want_adv, "advantages"), (ret, want_ret, "returns")):
        bad = np.argwhere(o.get(ctx) != bits32(w).reshape(T, -1))
        assert not len(bad), f"{ctx}: {name} differ in bits at (t, series) {bad[:6].tolist()}"
        o.free()
    free(*d)


@pytest.mark.parametrize("n,A", [(37, 3), (549, 2)], ids=["37x3", "549x2"])
def test_gae_done_is_any_non_zero_flag_byte(handles, n, A):
    """the flags as bytes 2, 0x80 and 0xFF, and term = 0x01 with trunc = 0xFE where both are set: `!= 0` is the definition"""
    for T in LENGTHS:
        r, te, tr, V = gae_data(T, n, A, seed=T, done_share=0.2, byte=DONE_BYTES)
        one = gae_data(T, n, A, seed=T, done_share=0.2)
        assert np.array_equal(te != 0, one[1] != 0) and np.array_equal(tr != 0, one[2] != 0), "`byte` moved a flag"
        if T >= 7:
            assert ((te == 0x01) & (tr == 0xFE)).any(), "no step with term = 0x01 and trunc = 0xFE: the case shows nothing"
            assert all(((te == b) & (tr == 0)).any() and ((tr == b) & (te == 0)).any() for b in DONE_BYTES), "a flag byte never stands alone"
            assert ((te | tr) == 0).any(), "every step is done"
        assert not ((te == 1) & (tr == 0)).any() and not (tr == 1).any(), "a flag written as 1 alone: that is the other tests' case"
        gae_against_the_model(handles[A], f"flag bytes, T = {T}, {n} x {A}", T, n, A, r, te, tr, V)
        if T == 16:                                                # ... and without the truncations array
            gae_against_the_model(handles[A], f"flag bytes, T = {T}, {n} x {A}, no truncations", T, n, A, r, te, None, V)


def test_gae_over_six_decades(handles):
    """every series' rewards and values times 10^k, k from -3 .. 3: the float64 recurrence at other exponents, under the suite's bar
    that the same recurrence in float32 gives other bits in at least 25 % of the advantages"""
    n, A = 549, 2
    k = np.random.default_rng(21).integers(-3, 4, (n, A))
    assert len(np.unique(k)) == 7
    for T in (7, 33):
        r, te, tr, V = gae_data(T, n, A, seed=200 + T)
        r = r * 10.0 ** k
        V = (V.astype(np.float64) * 10.0 ** k).astype(np.float32)
        adv, _ = targets.host_gae(r, te, tr, V, GAMMA, LAM)
        share = float((bits32(adv) != bits32(gae_float32(r, te, tr, V, GAMMA, LAM))).mean())
        print(f"six decades, T = {T}: {share:.1%} of the advantages differ from the float32 recurrence")
        assert share >= 0.25, f"T = {T}: only {share:.1%} of the advantages differ from the float32 recurrence: the case shows nothing"
        assert np.isfinite(adv).all() and float(np.abs(adv).max()) < 1e6
        gae_against_the_model(handles[A], f"six decades, T = {T}", T, n, A, r, te, tr, V)


@pytest.mark.parametrize("shape", [f"{d}x{w}" for d in (2, 4, 8, 16) for w in (64, 256)])
def test_every_k_gae_instance_the_library_carries(monkeypatch, shape):
    """CZ_GAE_SHAPE is read when a handle is made: every instance gives the default's bits, at every remainder of T over its block"""
    monkeypatch.setenv("CZ_GAE_SHAPE", shape)
    env = make_env(4, **COOP)
    n, A = 549, 2
    for T in LENGTHS + (40,):
        r, te, tr, V = gae_data(T, n, A, seed=100 + T)
        d = upload(env, r, te, tr, V)
        adv, ret = Guarded(env, T, n * A), Guarded(env, T, n * A)
        env.gae_device(T, *d, adv.ptr, ret.ptr, gamma=GAMMA, lam=LAM, env_count=n)
        env.sync()
        want_adv, want_ret = targets.host_gae(r, te, tr, V, GAMMA, LAM)
        assert np.array_equal(adv.get(shape), bits32(want_adv).reshape(T, -1)), f"{shape}, T = {T}: advantages"
        assert np.array_equal(ret.get(shape), bits32(want_ret).reshape(T, -1)), f"{shape}, T = {T}: returns"
        free(*d)
        adv.free()
        ret.free()
    env.close()
    monkeypatch.setenv("CZ_GAE_SHAPE", "3x64")
    env = make_env(4, **COOP)
    with pytest.raises(_native.NativeError, match="the library carries"):
        env.gae_device(1, *upload(env, *gae_data(1, 4, A)), env.alloc((4, A), np.uint32), None)
    env.close()


def test_gae_parameters_outputs_alone_and_agent_masks(handles):
    n, A, T = 65, 4, 7
    env = handles[A]
    r, te, tr, V = gae_data(T, n, A, seed=11)
    assert (te | tr).any()
    d = upload(env, r, te, tr, V)
    adv, ret = Guarded(env, T, n * A), Guarded(env, T, n * A)
    for gamma, lam in ((1.0, 1.0), (0.9, 0.0), (0.0, 1.0), (0.5, 0.25)):
        want = targets.host_gae(r, te, tr, V, gamma, lam)
        for outs in ((adv, ret), (adv, None), (None, ret)):
            adv.fill()
            ret.fill()
            env.gae_device(T, *d, *(None if o is None else o.ptr for o in outs), gamma=gamma, lam=lam, env_count=n)
            env.sync()
            for o, w, name in ((adv, want[0], "advantages"), (ret, want[1], "returns")):
                if o in outs:
                    assert np.array_equal(o.get(name), bits32(w).reshape(T, -1)), f"gamma {gamma} lam {lam}: {name} with outputs {outs}"
                else:
                    assert o.untouched(), f"{name} were not asked for"
    want = [bits32(w) for w in targets.host_gae(r, te, tr, V, GAMMA, LAM)]
    for mask in (0b0001, 0b1010, 0b0111, 0b1000, 0b10110):        # (bits past the last agent select nobody)
        adv.fill()
        ret.fill()
        env.gae_device(T, *d, adv.ptr, ret.ptr, agents=mask, env_count=n)
        env.sync()
        chosen = np.array([(mask >> a) & 1 for a in range(A)], bool)
        for o, w in ((adv, want[0]), (ret, want[1])):
            got = o.get(f"agents {mask:#x}").reshape(T, n, A)
            assert np.array_equal(got[:, :, chosen], w[:, :, chosen]) and (got[:, :, ~chosen] == F32_SENT).all(), f"agents {mask:#x}"
    free(*d)
    adv.free()
    ret.free()


def test_refusals_launch_nothing(handles):
    n, A, T = 37, 3, 7
    env = handles[A]
    r, te, tr, V = gae_data(T, n, A, seed=12)
    d = upload(env, r, te, tr, V)
    adv, ret = Guarded(env, T, n * A), Guarded(env, T, n * A)
    lg, act = upload(env, synthetic_logits(n, A, 8), np.zeros((n, A), np.int32))
    lp, en = Guarded(env, n, A), Guarded(env, n, A)

    def gae(**kw):
        a = dict(T=T, r=d[0], te=d[1], tr=d[2], V=d[3], adv=adv.ptr, ret=ret.ptr, gamma=GAMMA, lam=LAM, agents=None, env_count=n)
        a.update(kw)
        env.gae_device(a["T"], a["r"], a["te"], a["tr"], a["V"], a["adv"], a["ret"], gamma=a["gamma"], lam=a["lam"], agents=a["agents"],
                       env_count=a["env_count"])

    def logprob(**kw):
        a = dict(lg=lg, act=act, lp=lp.ptr, en=en.ptr, sets=(0, 0, 0), rows=n)
        a.update(kw)
        env.logprob_device(a["lg"], a["act"], a["lp"], a["en"], sets=a["sets"], rows=a["rows"])

    def refused(message, call, **kw):
        with pytest.raises(_native.NativeError, match=message):
            call(**kw)
        env.sync()
        assert adv.untouched() and ret.untouched() and lp.untouched() and en.untouched(), f"a refused call ({message}) wrote something"

    for T_bad in (0, -1):
        refused("T is", gae, T=T_bad)
    for n_bad in (0, -5):
        refused("env_count is", gae, env_count=n_bad)
    for name in ("r", "te", "V"):
        refused("pointer is null", gae, **{name: None})
    refused("both output pointers are null", gae, adv=None, ret=None)
    for mask in (0, 1 << A, 0xF0):
        refused("none of the 3 agents", gae, agents=mask)
    for bad in (-0.01, 1.0000001, float("nan"), float("inf")):
        refused("gamma is", gae, gamma=bad)
        refused("lambda is", gae, lam=bad)
    for rows_bad in (0, -1):
        refused("rows is", logprob, rows=rows_bad)
    refused("pointer is null", logprob, lg=None)
    refused("pointer is null", logprob, act=None)
    refused("both output pointers are null", logprob, lp=None, en=None)
    refused("every agent's byte of sets is 0xFF", logprob, sets=(None, None, None))
    gae()                                                          # ... and the handle works afterwards
    logprob()
    env.sync()
    assert np.array_equal(adv.get("after"), bits32(targets.host_gae(r, te, tr, V, GAMMA, LAM)[0]).reshape(T, -1))
    assert not lp.untouched()
    free(*d, lg, act)
    for g in (adv, ret, lp, en):
        g.free()


# ---------------------------------------------------------------------------------------------------------------------------
# log-probabilities
# ---------------------------------------------------------------------------------------------------------------------------

# (A = 3 and A = 1 do not divide the workgroup's 256 threads: a workgroup boundary falls inside an [A]-row, and k_logprob takes the
# agent from i % A)
@pytest.mark.parametrize("which,rows", [(w, r) for w in (5, 4) for r in (1, 37, 549 * 3)] + [(w, r) for w in (3, 1) for r in (37, 549 * 3)],
                         ids=lambda v: str(v))
def test_logprob_equals_the_host_model(handles, which, rows):
    env = handles[which]
    A, Cn = env.num_agents, env.num_actions
    assert (A, Cn) == ((2, 5) if which == 5 else (which, 8))
    lg = synthetic_logits(rows, A, Cn, seed=rows)
    rng = np.random.default_rng(rows)
    act = rng.integers(0, Cn, (rows, A)).astype(np.int32)
    outside = rng.random((rows, A)) < 0.1
    act[outside] = rng.choice([ACT_OUTSIDE, -1, Cn, 2 ** 31 - 1], int(outside.sum()))
    if rows == 1:
        act[0, 0], act[0, 1] = Cn - 1, ACT_OUTSIDE
    want_lp, want_en = (bits32(w) for w in targets.host_logprob(lg, act))
    assert (want_lp[act == ACT_OUTSIDE] == 0).all()
    d_lg, d_act = upload(env, lg, act)
    lp, en = Guarded(env, rows, A), Guarded(env, rows, A)
    everyone = (0,) * A
    left_out = sorted({0, A // 2, A - 1}) if A >= 2 else []        # the first, the middle or the last agent (one agent: nobody)
    for sets in [everyone] + [everyone[:a] + (None,) + everyone[a + 1:] for a in left_out]:
        chosen = np.array([s is not None for s in sets])
        for outs in ((lp, en), (lp, None), (None, en)):
            lp.fill()
            en.fill()
            env.logprob_device(d_lg, d_act, *(None if o is None else o.ptr for o in outs), sets=sets, rows=rows)
            env.sync()
            for o, w, name in ((lp, want_lp, "logp"), (en, want_en, "entropy")):
                if o not in outs:
                    assert o.untouched(), f"{name} was not asked for"
                    continue
                got = o.get(name)
                bad = np.argwhere(got[:, chosen] != w[:, chosen])
                assert not len(bad), f"C = {Cn}, {rows} rows, sets {sets}: {name} differs in bits at (row, agent) {bad[:6].tolist()}"
                assert (got[:, ~chosen] == F32_SENT).all(), f"{name} of an agent at 0xFF was written"
    free(d_lg, d_act)
    lp.free()
    en.free()


# ---------------------------------------------------------------------------------------------------------------------------
# on the device's own trajectory, inside a capture, over shards
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_devices_own_trajectory_eagerly_and_from_a_callers_graph():
    n, A, T = 48, 2, 30
    env = make_env(n, **COOP)
    W = weights(env.F, env.num_actions, 1, 21, scale2=0.03)
    env.load_policy(*W)
    env.reset(return_obs=False)
    tr = PolicyTraj(env, T)
    got = tr.rollout(env, (0, 0), "sample", 5)
    done = (got["term"] | got["trunc"]) != 0
    assert done.any() and not done.all(), "the trajectory holds no done (max_steps = 12 < T): the case shows nothing"
    assert len(np.unique(got["act"])) >= 2
    V = np.random.default_rng(8).standard_normal((T + 1, n, A)).astype(np.float32)
    d_V, = upload(env, V)
    b = tr.buf
    adv, ret, lp, en = (Guarded(env, T, n * A) for _ in range(4))
    want_adv, want_ret = targets.host_gae(got["rew"].view(np.float64), got["term"], got["trunc"], V, GAMMA, LAM)
    want_lp, want_en = targets.host_logprob(got["logits"].view(np.float32), got["act"])

    def calls():                                                   # rewards, flags, logits and actions straight from device memory
        env.logprob_device(b["logits"], b["act"], lp.ptr, en.ptr, sets=(0, 0), rows=T * n)
        env.gae_device(T, b["rew"], b["term"], b["trunc"], d_V, adv.ptr, ret.ptr)

    def check(ctx):
        for o, w, name in ((adv, want_adv, "advantages"), (ret, want_ret, "returns"), (lp, want_lp, "logp"), (en, want_en, "entropy")):
            assert np.array_equal(o.get(ctx).reshape(T, n, A), bits32(w)), f"{ctx}: {name}"
            o.fill()

    calls()
    env.sync()
    check("eager")
    assert float(np.abs(np.exp(want_lp.astype(np.float64))).max()) <= 1.0 and (want_lp < 0).any()
    cs = CallerStream(env)
    with cs.capture():
        calls()
    assert all(o.untouched() for o in (adv, ret, lp, en)), "capturing must not have launched anything"
    for k in range(2):
        cs.replay()
        cs.sync()
        check(f"replay {k}")
    cs.close()
    env.close()


def test_unequal_shards_equal_the_host_model(monkeypatch):
    from cooking_zoo_amd import sharded
    n, A, T = 67, 2, 7                                             # 37 + 30
    t = tables_of(n, **dict(COOP, max_steps=6))
    monkeypatch.setattr(sharded, "plan_shards", lambda num_envs, world_size, k: [(0, 37), (37, 30)])
    many = sharded.ShardedVecEnv(n, tables=t, device_ids=[0, 0], auto_reset=False, level=None, meta_file=None, num_agents=None, max_steps=None,
                                 recipes=None)
    try:
        assert [c for _, c in many.ranges] == [37, 30]
        r, te, tr, V = gae_data(T, n, A, seed=13)
        lg = synthetic_logits(T * n, A, 5, seed=14).reshape(T, n, A, 5)
        act = np.random.default_rng(15).integers(0, 5, (T, n, A)).astype(np.int32)
        bufs = {}
        for name, arr, per, lead in (("r", r, (A,), T), ("te", te, (A,), T), ("tr", tr, (A,), T), ("V", V, (A,), T + 1), ("lg", lg, (A, 5), T),
                                     ("act", act, (A,), T)):
            bufs[name] = many.alloc(per, arr.dtype, leading=(lead,))
            bufs[name].from_host(arr)
        outs = {name: many.alloc((A,), np.uint32, leading=(T,)) for name in ("adv", "ret", "lp", "en")}
        for o in outs.values():
            o.from_host(np.full((T, n, A), F32_SENT, np.uint32))
        many.gae_device(T, bufs["r"], bufs["te"], bufs["tr"], bufs["V"], outs["adv"], outs["ret"], gamma=GAMMA, lam=LAM)
        many.logprob_device(bufs["lg"], bufs["act"], outs["lp"], outs["en"], sets=(0, None))
        many.sync()
        want = dict(zip(("adv", "ret"), targets.host_gae(r, te, tr, V, GAMMA, LAM)))
        want.update(zip(("lp", "en"), targets.host_logprob(lg, act)))
        for name in ("adv", "ret"):
            assert np.array_equal(outs[name].to_host(), bits32(want[name])), name
        for name in ("lp", "en"):
            got = outs[name].to_host()
            assert np.array_equal(got[:, :, 0], bits32(want[name])[:, :, 0]) and (got[:, :, 1] == F32_SENT).all(), name
        many.logprob_device(bufs["lg"], bufs["act"], outs["lp"], None, rows=T * n)
        many.sync()
        assert np.array_equal(outs["lp"].to_host(), bits32(want["lp"]))
        with pytest.raises(ValueError):
            many.logprob_device(bufs["lg"], bufs["act"], outs["lp"], None, rows=T * n + 1)
    finally:
        many.close()
