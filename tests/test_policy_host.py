"""CPU: the MLP policy's definition (cooking_zoo_amd/policy.py) checked without a GPU - the float32 fmaf emulation against libm's fmaf,
the midpoint cases included; host_logits against a scalar second model; cz_exp against np.exp; the sampling rule by hand and by
frequencies; the keyed draw against the library's cz_spawn_uniform; the entry points in header, library and binding with the ABI
number still 10; the mode 9 kernels in the built library's metadata; and the condition that makes the GPU comparison sensitive: on
real rows a float32 matrix product in another summation order gives other logit bits."""
import ctypes as C
import ctypes.util
import inspect
import math
import re

import numpy as np
import pytest

from cooking_zoo_amd import policy
from host_common import HEADER, INSTANCES, LIB, device_code  # noqa: F401  (device_code: the fixture)
from oracle_binding import VecOracle
from policy_common import ROLLOUT_POLICY, dense_conditions, dense_rows, exact_logit_weights, logit_cases, logits_per_set, swap_columns, weights
from vec_common import TWO, tables_of

NEW_SYMBOLS = ["cz_load_policy_device", "cz_policy_sets", "cz_policy_device", "cz_rollout_policy"]

libm = C.CDLL(ctypes.util.find_library("m"))
libm.fmaf.restype = C.c_float
libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


def libm_fmaf(a, b, c):
    return np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)


def naive_fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def midpoint_triples(rng, n):
    """c = a 24-bit integer times a power of two, a * b within a few ulps of half an ulp of c: the exact sum sits next to a float32
    midpoint and has more than 53 bits, so rounding it to float64 first and to float32 afterwards goes wrong"""
    m = rng.integers(1 << 23, 1 << 24, n)
    e = rng.integers(-20, 20, n)
    c = (np.ldexp(m.astype(np.float64), e) * rng.choice([-1.0, 1.0], n)).astype(np.float32)        # ulp(c) = 2^e
    a = rng.uniform(1.0, 2.0, n).astype(np.float32)
    b = (np.ldexp(0.5, e) / a.astype(np.float64)).astype(np.float32)                               # a * b = 2^(e-1) (1 + d), |d| <= 2^-24
    b = (b.view(np.int32) + rng.integers(-3, 4, n).astype(np.int32)).view(np.float32)               # ... and a few ulps of b either way
    return a, (b * rng.choice([-1.0, 1.0], n).astype(np.float32)).astype(np.float32), c


def test_fmaf_emulation_equals_libm_on_random_triples():
    rng = np.random.default_rng(1)
    n = 40000
    a, b, c = (rng.standard_normal(n).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, n).astype(np.float32) for _ in range(3))
    assert np.array_equal(policy.fmaf32(a, b, c).view(np.uint32), libm_fmaf(a, b, c).view(np.uint32))


def test_fmaf_emulation_equals_libm_on_float32_midpoints_where_the_naive_form_fails():
    rng = np.random.default_rng(2)
    a, b, c = midpoint_triples(rng, 40000)
    want = libm_fmaf(a, b, c)
    assert np.array_equal(policy.fmaf32(a, b, c).view(np.uint32), want.view(np.uint32))
    wrong = int((naive_fmaf(a, b, c).view(np.uint32) != want.view(np.uint32)).sum())
    assert wrong >= 100, f"the construction does not reach the double-rounding cases ({wrong} of {len(a)}): the test above shows nothing"


# ---------------------------------------------------------------------------------------------------------------------------
# host_logits
# ---------------------------------------------------------------------------------------------------------------------------

def scalar_logits(x, w1, b1, w2, b2):
    """the definition in Python loops over libm's fmaf and numpy float32 scalars"""
    F, Cn = len(x), len(b2)
    h = []
    for j in range(64):
        acc = float(b1[j])
        for f in range(F):
            acc = libm.fmaf(float(w1[j][f]), float(x[f]), acc)
        h.append(np.float32(acc) if acc > 0 else np.float32(0))
    out = []
    for c in range(Cn):
        p = [np.float32(w2[c][j]) * h[j] for j in range(64)]
        for k in range(6):                                         # the butterfly itself, every lane: p_j + p_(j xor 2^k)
            p = [np.float32(p[j] + p[j ^ (1 << k)]) for j in range(64)]
        assert all(np.float32(v).tobytes() == np.float32(p[0]).tobytes() for v in p), "the lanes of a butterfly disagree"
        out.append(np.float32(p[0] + np.float32(b2[c])))
    return np.array(out, np.float32)


@pytest.fixture(scope="module")
def oracle_rows():
    """float32 rows of the oracle on coop_test / example_odd (F = 283): the reset observation and a few steps of the action stream"""
    tables = tables_of(6, "coop_test", "example_odd", 2, TWO, "scheme3", 12, 3)
    orc = VecOracle.from_vec_env(tables)
    rows = [orc.reset().copy()]
    err, _, _, _, _, acts = orc.oracle.rollout(orc.records.copy(), 4, 5, 0, want_obs=False, want_actions=True)
    assert err == 0
    for t in range(4):
        rows.append(orc.step(acts[t])[0].copy())
    return np.stack(rows).astype(np.float32)                      # [5][6][2][283]


@pytest.mark.parametrize("F", [5, 283])
def test_host_logits_equals_the_scalar_model(oracle_rows, F):
    x = oracle_rows[:, :2, :, :F].reshape(-1, F)[:6]
    W = weights(F, 5, 1, F)
    got = policy.host_logits(x, W[0][0], W[1][0], W[2][0], W[3][0])
    want = np.stack([scalar_logits(r, W[0][0], W[1][0], W[2][0], W[3][0]) for r in x])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_logits_are_sensitive_to_the_summation_order(oracle_rows):
    """at least 25 % of the expected logits differ in bits from the plain float32 matrix products: the bits pin the arithmetic"""
    x = oracle_rows.reshape(-1, oracle_rows.shape[-1])
    for Cn in (5, 8):
        w1, b1, w2, b2 = (w[0] for w in weights(x.shape[1], Cn, 1, Cn))
        want = policy.host_logits(x, w1, b1, w2, b2)
        other = (np.maximum(x @ w1.T + b1, 0) @ w2.T + b2).astype(np.float32)
        share = float((want.view(np.uint32) != other.view(np.uint32)).mean())
        assert share >= 0.25, f"only {share:.1%} of the logits differ from the matrix-product form"
        assert int((want.argmax(-1) != other.argmax(-1)).sum()) <= len(x) // 50     # (actions barely notice: the logits are the check)


def test_observation_rows_never_reach_the_last_columns_of_w1_and_dense_rows_do(oracle_rows):
    """the gap the dense GPU test closes, as a fact of the data: the oracle's rows at F = 283 are 0.0 in the whole last quad (and in
    about half their features), so exchanging two columns of W1 there leaves every expected logit as it was - a pack that did so
    on the device would pass every comparison on such rows.  On dense_rows the same exchange changes every row."""
    F = oracle_rows.shape[-1]
    x = oracle_rows.reshape(-1, F)
    assert F == 283 and (x[:, 280:] == 0).all(), "the oracle's rows reach the last quad: this test and the comment above test_row_tails are out of date"
    used = int((x != 0).any(axis=0).sum())
    assert used <= F * 6 // 10, f"{used} of {F} features are non-zero in some row"
    w1, b1, w2, b2 = (w[0] for w in weights(F, 5, 1, 3, scale2=0.03))
    other = swap_columns(w1, F - 2)
    assert (other != w1).any()
    bits = lambda rows, w: policy.host_logits(rows, w, b1, w2, b2).view(np.uint32)
    assert np.array_equal(bits(x, other), bits(x, w1)), "the exchange shows on observation rows after all"
    dense = dense_rows(6, 2, F, 1).reshape(-1, F)
    assert (dense != 0).all() and all(len(np.unique(r)) == F for r in dense)
    assert (bits(dense, other) != bits(dense, w1)).any(axis=-1).all(), "the exchange leaves a dense row's logits as they were"
    W4 = weights(F, 5, 4, 3, scale2=0.03)
    share = dense_conditions("F = 283", dense, W4, logits_per_set(dense, W4))
    print(f"dense rows, F = 283: {share:.1%} of the logits differ from the matrix-product form")


@pytest.mark.parametrize("Cn", [5, 8])
def test_exact_logit_weights_give_their_logits_in_bits_for_any_row(oracle_rows, Cn):
    F = oracle_rows.shape[-1]
    rows = np.concatenate([oracle_rows.reshape(-1, F)[:8], dense_rows(4, 2, F, Cn).reshape(-1, F), -4.0 * dense_rows(1, 2, F, 9).reshape(-1, F)])
    for name, (L, dead) in logit_cases(Cn).items():
        assert L.dtype == np.float32 and L.shape == (Cn,)
        w = exact_logit_weights(F, L, dead)
        got = policy.host_logits(rows, *w)
        assert (got.view(np.uint32) == L.view(np.uint32)).all(), f"{name}: the logits are not L in bits"
        assert (policy.host_actions(got) == int(L.argmax())).all()
        if dead:
            assert (w[1] < 0).all() and (w[2] != 0).all() and (w[3] == L).all(), "dead: every hidden unit off, the logits from b2"
    # the sampling rule on them, by hand: u just below 1 takes the last action with a share of the sum; ties split the draw range
    pick = lambda L, u: int(policy.sample_from(L[None], np.array([u]))[0])
    cases = logit_cases(Cn)
    flat, tie, clamp, one = (cases[k][0] for k in ("flat", "tie3", "clamp", "one"))
    assert [pick(flat, (c + 0.5) / Cn) for c in range(Cn)] == list(range(Cn))
    assert pick(tie, 0.0) == 0 and pick(tie, 0.5) == 3 and pick(tie, 1.0 - 2.0 ** -53) == Cn - 1 and policy.host_actions(tie[None])[0] == 1
    assert pick(clamp, 0.0) == 0 and pick(clamp, 1e-25) == 1     # 70 below the maximum: clamped to exp(-64), still a share of its own
    assert all(pick(one, u) == Cn - 2 for u in (2.0 ** -53, 0.3, 1.0 - 2.0 ** -53))


# ---------------------------------------------------------------------------------------------------------------------------
# cz_exp, sampling, the keyed draw
# ---------------------------------------------------------------------------------------------------------------------------

def test_cz_exp_against_numpy():
    z = np.concatenate([np.linspace(-64.0, 0.0, 200001), -np.random.default_rng(3).uniform(0, 64, 200000), [0.0, -64.0, -1e-300, -0.5 * math.log(2)]])
    got, want = policy.cz_exp(z), np.exp(z)
    assert float(np.max(np.abs(got - want) / want)) <= 1e-15
    assert policy.cz_exp(0.0) == 1.0


def test_sampling_rule_by_hand():
    lg = np.array([[0.0, 0.0, 0.0, 0.0]], np.float32)             # S = 1, 2, 3, 4
    pick = lambda u, l=lg: int(policy.sample_from(l, np.array([u]))[0])
    assert pick(0.0) == 0                                          # u = 0: thr = 0, S_0 = 1 > 0
    assert pick(0.25) == 1                                         # thr = 1.0: S_0 > thr is false - a tie goes to the next action
    assert pick(0.2499) == 0 and pick(0.5) == 2 and pick(0.75) == 3 and pick(0.999) == 3
    # the C - 1 fallback: no S_c exceeds thr.  A keyed draw stays below 1 and never gets there; u = 1 by hand does (thr = S_(C-1))
    assert pick(1.0) == 3
    far = np.array([[0.0, -1000.0, -1000.0]], np.float32)          # z below -64 is clamped: e = cz_exp(-64) > 0, absorbed by S_0 = 1
    assert policy.cz_exp(-64.0) > 0 and pick(0.0, far) == 0 and pick(1.0 - 2.0 ** -53, far) == 0 and pick(1.0, far) == 2
    assert policy.host_actions(np.array([[1.0, 3.0, 3.0, 2.0]], np.float32))[0] == 1       # greedy: the first of the largest


def test_sampling_frequencies_follow_softmax():
    lg = np.array([0.3, -1.2, 2.0, 0.0, 1.1], np.float32)
    n = 200000
    env = np.arange(n) % 4096
    step = np.arange(n) // 4096
    acts = policy.host_actions(np.broadcast_to(lg, (n, 5)), "sample", 77, env, step, 1)
    p = np.exp(lg.astype(np.float64) - lg.max())
    p /= p.sum()
    freq = np.bincount(acts, minlength=5) / n
    sd = np.sqrt(p * (1 - p) / n)
    assert (np.abs(freq - p) <= 5 * sd).all(), (freq, p, sd)


def test_the_draw_is_the_librarys_keyed_stream():
    lib = C.CDLL(LIB)
    lib.cz_spawn_uniform.restype = C.c_double
    lib.cz_spawn_uniform.argtypes = [C.c_uint64, C.c_int64, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32]
    for seed, g, step, a in [(0, 0, 0, 0), (77, 4095, 31, 3), (2 ** 63 + 5, 2 ** 33 + 7, 2 ** 32 - 1, 2), (1, 1, 1, 1)]:
        assert float(policy.draw(seed, g, step, a)) == lib.cz_spawn_uniform(seed, g, 0, step, 0x300 + a, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_and_the_abi_number_stays_ten():
    from cooking_zoo_amd import _abi, _native
    text = open(HEADER).read()
    assert re.search(r"^int cz_load_policy_device\(cz_handle h, int32_t n_sets, const float \*d_w1, const float \*d_b1, const float \*d_w2, "
                     r"const float \*d_b2\);", text, flags=re.M)
    assert re.search(r"^int cz_policy_device\(cz_handle h, int64_t env_begin, int64_t env_count, const float \*d_obs32, uint32_t sets, int32_t mode,"
                     r"\s+uint64_t seed, uint32_t step, int32_t \*d_actions, float \*d_logits\);", text, flags=re.M)
    assert re.search(r"^int cz_rollout_policy\(cz_handle h, int32_t T, uint32_t sets, int32_t mode, uint64_t seed, uint32_t step0, float \*d_obs32,"
                     r"\s+int32_t \*d_actions, float \*d_logits, double \*d_rewards, uint8_t \*d_terminations, uint8_t \*d_truncations\);", text, flags=re.M)
    assert "#define CZ_POLICY_GREEDY 0" in text and "#define CZ_POLICY_SAMPLE 1" in text and "NOT pinned" in text
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
    assert [len(bound[n]) for n in NEW_SYMBOLS] == [6, 1, 10, 12]


def test_python_layer_has_the_methods():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for cls in (CookingVecEnv, ShardedVecEnv):
        assert list(inspect.signature(cls.load_policy).parameters) == ["self", "w1", "b1", "w2", "b2"]
        assert list(inspect.signature(cls.rollout_policy).parameters) == ["self", "T", "d_obs32", "d_actions", "d_logits", "d_rewards", "d_term",
                                                                          "d_trunc", "sets", "mode", "seed", "step0"]
        assert list(inspect.signature(cls.policy_device).parameters)[:8] == ["self", "d_obs32", "d_actions", "d_logits", "sets", "mode", "seed", "step"]
        assert isinstance(cls.policy_sets, property)
    assert policy.pack_sets((1, 0, None), 3) == 0xFFFF0001 and policy.pack_sets((0, 0, 0, 0), 2) == 0xFFFF0000
    with pytest.raises(ValueError):
        policy.pack_sets((4,), 1)


def test_every_instance_has_its_policy_rollout_kernels(device_code):  # noqa: F811
    meta, code = device_code
    names = [(inst, f"_ZN2cz6k_stepILi{opl}ELi{cpl}ELi{na}ELi{scheme}ELi{ROLLOUT_POLICY}EEEvPjPKiPKdiiiiiiiNS_6ParamsE")
             for inst, (opl, cpl) in INSTANCES.items() for na in (1, 2, 3, 4) for scheme in (1, 3)]
    assert len(names) == 24
    missing = [(inst, k) for inst, k in names if k not in meta or k not in code]
    assert not missing, missing
    for _, k in names:                                             # the hidden layer is an explicit fused multiply-add, lane = unit
        assert any(l.startswith(("v_fma_f32", "v_fmac_f32")) for l in code[k]), k
    for na in (1, 2, 3, 4):
        assert f"_ZN2cz8k_policyILi{na}EEEvNS_10PolicyArgsE" in meta
    assert "_ZN2cz13k_policy_packILi0EEEvPfiiiPKfS3_S3_S3_" in meta
