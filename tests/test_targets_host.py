"""CPU: the definitions of cooking_zoo_amd/targets.py checked without a GPU - host_gae against a scalar second model and by hand, with
the condition that makes equal bits mean something (the same recurrence carried in float32 gives other bits); cz_log against np.log;
host_logprob against numpy's float64 log-softmax, with ties, the clamp and an action outside the range; the two entry points in
header, library and binding with the ABI number still 10; k_gae and k_logprob in the built library's metadata."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from cooking_zoo_amd import policy, targets
from host_common import HEADER, LIB, device_code  # noqa: F401  (device_code: the fixture)
from targets_common import GAMMA, LAM, bits32, gae_data, gae_float32, scalar_gae, synthetic_logits

NEW_SYMBOLS = ["cz_gae_device", "cz_logprob_device"]


# ---------------------------------------------------------------------------------------------------------------------------
# host_gae
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", ["term", "trunc", "both"])
def test_host_gae_equals_the_scalar_model(flags):
    r, te, tr, V = gae_data(33, 41, 3, seed=1, flags=flags)
    assert (te | tr).any() and ((te | tr) == 0).any()
    for gamma, lam in ((GAMMA, LAM), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5)):
        adv, ret = targets.host_gae(r, te, tr, V, gamma, lam)
        want_adv, want_ret = scalar_gae(r, te, tr, V, gamma, lam)
        assert adv.dtype == ret.dtype == np.float32 and adv.shape == ret.shape == r.shape
        assert np.array_equal(bits32(adv), bits32(want_adv)) and np.array_equal(bits32(ret), bits32(want_ret)), (gamma, lam)


def test_gae_one_step():
    r, V = np.array([[0.5]]), np.array([[0.25], [2.0]], np.float32)
    zero, one = np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8)
    adv, ret = targets.host_gae(r, zero, zero, V, 0.5, 0.7)
    assert adv[0, 0] == np.float32(0.5 + 0.5 * 2.0 - 0.25) and ret[0, 0] == np.float32(1.5)
    for te, tr in ((one, zero), (zero, one), (one, one), (one, None)):
        adv, ret = targets.host_gae(r, te, tr, V, 0.5, 0.7)
        assert adv[0, 0] == np.float32(0.25) and ret[0, 0] == np.float32(0.5), "a done step's target is its reward alone"


def test_a_done_cuts_the_bootstrap_and_the_carry():
    """T = 3 with a done at t = 1: step 1 sees neither V[2] nor A[2]; step 0 carries A[1] and bootstraps from V[1] as usual"""
    g, l = 0.5, 0.5
    r = np.array([1.0, 2.0, 4.0]).reshape(3, 1)
    V = np.array([0.5, 0.25, 8.0, 16.0], np.float32).reshape(4, 1)
    te = np.array([0, 1, 0], np.uint8).reshape(3, 1)
    adv, ret = targets.host_gae(r, te, None, V, g, l)
    a2 = 4.0 + g * 16.0 - 8.0
    a1 = 2.0 - 0.25
    a0 = (1.0 + g * 0.25 - 0.5) + g * l * a1
    assert adv[:, 0].tolist() == [a0, a1, a2] and ret[:, 0].tolist() == [a0 + 0.5, a1 + 0.25, a2 + 8.0]
    free, _ = targets.host_gae(r, np.zeros_like(te), None, V, g, l)
    assert free[2, 0] == adv[2, 0] and free[1, 0] == (2.0 + g * 8.0 - 0.25) + g * l * a2 and free[0, 0] != adv[0, 0]


def test_lambda_zero_is_the_td_error():
    r, te, tr, V = gae_data(9, 50, 2, seed=2)
    adv, ret = targets.host_gae(r, te, tr, V, GAMMA, 0.0)
    done = (te | tr) != 0
    V64 = V.astype(np.float64)
    d = (r + np.where(done, 0.0, np.float64(GAMMA) * V64[1:])) - V64[:-1]
    assert np.array_equal(bits32(adv), bits32(d.astype(np.float32)))
    assert np.array_equal(bits32(ret), bits32((d + V64[:-1]).astype(np.float32)))


def test_dyadic_returns_are_exact():
    """gamma = lam = 1, no dones, rewards and values multiples of 2^-6 below 2^10: nothing rounds, so ret[t] is the reward sum from
    t on plus V_T and adv[t] that minus V[t], exactly"""
    rng = np.random.default_rng(3)
    T, n = 20, 64
    r = rng.integers(-2000, 2000, (T, n)) / 64.0
    V = (rng.integers(-2000, 2000, (T + 1, n)) / 64.0).astype(np.float32)
    zero = np.zeros((T, n), np.uint8)
    adv, ret = targets.host_gae(r, zero, zero, V, 1.0, 1.0)
    want = np.cumsum(r[::-1], axis=0)[::-1] + V[T].astype(np.float64)
    assert np.array_equal(ret.astype(np.float64), want) and np.array_equal(adv.astype(np.float64), want - V[:T])


def test_no_truncations_is_all_zero_truncations():
    r, te, _, V = gae_data(12, 30, 2, seed=4, flags="term")
    a, b = targets.host_gae(r, te, None, V, GAMMA, LAM), targets.host_gae(r, te, np.zeros_like(te), V, GAMMA, LAM)
    assert np.array_equal(bits32(a[0]), bits32(b[0])) and np.array_equal(bits32(a[1]), bits32(b[1]))
    with pytest.raises(ValueError):
        targets.host_gae(r, te, None, V[:-1], GAMMA, LAM)


def test_advantages_are_sensitive_to_the_precision_of_the_recurrence():
    """at least 25 % of the advantages differ in bits from the same recurrence carried in float32 (measured: 69 %): the bits pin the
    float64 arithmetic"""
    r, te, tr, V = gae_data(32, 4096, 1, seed=0)
    adv, _ = targets.host_gae(r, te, tr, V, GAMMA, LAM)
    other = gae_float32(r, te, tr, V, GAMMA, LAM)
    share = float((bits32(adv) != bits32(other)).mean())
    print(f"float32 recurrence: {share:.1%} of the advantages differ in bits")
    assert share >= 0.25, f"only {share:.1%} of the advantages differ from the float32 recurrence"
    assert float(np.abs(adv - other).max()) < 1e-3                  # (the same quantity all the same)


# ---------------------------------------------------------------------------------------------------------------------------
# cz_log, host_logprob
# ---------------------------------------------------------------------------------------------------------------------------

def log_points():
    rng = np.random.default_rng(5)
    edges = np.array([1.0, 2.0, 4.0, 8.0])
    s = np.concatenate([np.linspace(1.0, 8.0, 200001), rng.uniform(1.0, 8.0, 100000), 1.0 + 10.0 ** -np.arange(0, 17.0), edges,
                        np.nextafter(edges, 0.0), np.nextafter(edges, 9.0)])
    return s[(s >= 1.0) & (s <= 8.0)]


def test_cz_log_against_numpy():
    """measured maximum of |cz_log - np.log| on these 300 000 points of [1, 8]: 4.5e-16 (at 7.389); the bound 1e-14 follows from
    cz_exp's 1e-15 relative: a Newton step's fixed point y has |S exp(-y) - 1| of that size"""
    s = log_points()
    assert len(s) >= 300000 and s.min() == 1.0 and s.max() == 8.0 and (s == 1.0 + 1e-15).any()
    err = np.abs(targets.cz_log(s) - np.log(s))
    print(f"cz_log: max abs error {err.max():.3g} at {s[err.argmax()]!r}")
    assert float(err.max()) <= 1e-14
    assert targets.cz_log(1.0) == 0.0 and targets.cz_log(np.array([1.0]))[0] == 0.0


def test_logprob_against_numpy_float64():
    """the float64 log-probabilities against numpy's z - log(sum(exp z)): within 1e-14 absolute wherever float64 can say so - rows
    whose log-probabilities all stay above -32, where both sides' last subtraction rounds by at most 3.6e-15 - and within 1e-14 plus
    one float64 ulp of the reference everywhere (at -1000, the clamp rows, an ulp is 1.1e-13: the reference's own rounding)"""
    for C_ in (5, 8):
        lg = synthetic_logits(3000, 2, C_, seed=C_)
        z, L = targets.logprob64(lg)
        mine = z - L[..., None]
        x = lg.astype(np.float64)
        x = x - x.max(axis=-1, keepdims=True)
        want = x - np.log(np.exp(x).sum(axis=-1, keepdims=True))
        near = (want > -32.0).all(axis=-1)
        assert near.mean() > 0.5 and not near.all()
        assert float(np.abs(mine - want)[near].max()) <= 1e-14
        assert (np.abs(mine - want) <= 1e-14 + np.spacing(np.abs(want))).all()
        # every action's float32 log-probability exponentiates to a distribution
        every = np.stack([targets.host_logprob(lg, np.full(lg.shape[:-1], c, np.int32))[0] for c in range(C_)], axis=-1)
        assert every.dtype == np.float32 and float(np.abs(np.exp(every.astype(np.float64)).sum(-1) - 1.0).max()) <= 1e-6
        _, ent = targets.host_logprob(lg, np.zeros(lg.shape[:-1], np.int32))
        p = np.exp(want)
        assert float(np.abs(ent - -(p * want).sum(-1)).max()) <= 1e-6 and (ent >= 0).all() and float(ent.max()) <= np.log(C_) + 1e-6


def test_logprob_ties_clamp_and_actions_outside():
    tie = np.array([[2.0, 2.0, -1.0, 2.0, 0.0]], np.float32)
    lp = [float(targets.host_logprob(tie, np.array([c]))[0][0]) for c in range(5)]
    assert lp[0] == lp[1] == lp[3] and lp[0] > lp[4] > lp[2]
    flat = np.zeros((1, 8), np.float32)                           # S = 8: cz_log's last octave
    lp8, ent8 = targets.host_logprob(flat, np.array([7]))
    assert lp8[0] == np.float32(-np.log(8.0)) and ent8[0] == np.float32(np.log(8.0))
    far = np.array([[0.0, -1000.0, -1000.0, -1000.0, -1000.0]], np.float32)
    lp_far, ent_far = targets.host_logprob(far, np.array([1]))
    assert lp_far[0] == np.float32(-1000.0)                        # z itself, not the clamped -64: only cz_exp's argument is clamped
    assert 1.0 + 4 * policy.cz_exp(-64.0) == 1.0                   # ... whose e = cz_exp(-64) the sum absorbs: S = 1, cz_log = 0
    lp_one, _ = targets.host_logprob(far, np.array([0]))
    assert lp_one[0] == 0.0 and bits32(lp_one)[0] == 0, "one overwhelming action has logp == 0.0"
    assert 0.0 <= float(ent_far[0]) < 1e-20
    for outside in (-1, 5, -7777, 2 ** 31 - 1):
        lp_out, ent_out = targets.host_logprob(tie, np.array([outside]))
        assert bits32(lp_out)[0] == 0 and ent_out[0] == targets.host_logprob(tie, np.array([0]))[1][0]


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_and_the_abi_number_stays_ten():
    from cooking_zoo_amd import _abi, _native
    text = open(HEADER).read()
    gae = ("int cz_gae_device(cz_handle h, int32_t T, int64_t env_count, const double *d_rewards, const uint8_t *d_terminations,\n"
           "                  const uint8_t *d_truncations, const float *d_values, double gamma, double lambda, uint32_t agents,\n"
           "                  float *d_advantages, float *d_returns);\n")
    logprob = ("int cz_logprob_device(cz_handle h, int64_t rows, const float *d_logits, const int32_t *d_actions, uint32_t sets,\n"
               "                      float *d_logp, float *d_entropy);\n")
    assert "\n" + gae in text and "\n" + logprob in text
    assert _native.header_abi_version() == 10 == _abi.CZ_ABI_VERSION
    lib = C.CDLL(LIB)
    lib.cz_abi_version.restype = C.c_int32
    assert lib.cz_abi_version() == 10


def test_library_exports_and_binding_lists_the_entry_points():
    from cooking_zoo_amd import _native
    lib = C.CDLL(LIB)
    bound = {name: args for name, _, args in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name + " is not exported"
        assert name in bound and name in _native.ADDED_SYMBOLS, name
    assert [len(bound[n]) for n in NEW_SYMBOLS] == [12, 7]
    assert bound["cz_gae_device"][7:9] == [C.c_double, C.c_double]


def test_python_layer_has_the_methods():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for cls in (CookingVecEnv, ShardedVecEnv):
        assert list(inspect.signature(cls.gae_device).parameters) == ["self", "T", "d_rewards", "d_term", "d_trunc", "d_values", "d_adv", "d_ret",
                                                                      "gamma", "lam", "agents", "env_count"]
        assert list(inspect.signature(cls.logprob_device).parameters) == ["self", "d_logits", "d_actions", "d_logp", "d_entropy", "sets", "rows"]
        defaults = {k: v.default for k, v in inspect.signature(cls.gae_device).parameters.items()}
        assert defaults["gamma"] == 0.99 and defaults["lam"] == 0.95 and defaults["d_adv"] is None and defaults["agents"] is None


def test_the_library_has_the_kernels(device_code):  # noqa: F811
    meta, _ = device_code
    gae = [k for k in meta if re.match(r"_ZN2cz5k_gaeILi\d+ELi\d+EEEvNS_7GaeArgsE$", k)]
    assert len(gae) >= 1, sorted(k for k in meta if "gae" in k)
    for c in (5, 8):
        assert f"_ZN2cz9k_logprobILi{c}EEEvNS_11LogprobArgsE" in meta
    for k in gae + [f"_ZN2cz9k_logprobILi{c}EEEvNS_11LogprobArgsE" for c in (5, 8)]:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, f"{k} spills or keeps an array in scratch"
