"""CPU: the value head's definition (cooking_zoo_amd/policy.py, step 3b) checked without a GPU - host_value against a scalar loop
model; the hand cases whose value is known in bits for any finite row; host_value as host_logits of a set whose W2 row c is wv and
whose b2[c] is bv (the same arithmetic); the condition that makes the GPU comparison sensitive - on dense rows a float32 matrix
product in another summation order gives other value bits; the entry points in header, library and binding with the ABI number
still 10; and the mode 10 kernels in the built library's metadata."""
import ctypes as C
import ctypes.util
import inspect
import re

import numpy as np
import pytest

from cooking_zoo_amd import policy
from host_common import HEADER, INSTANCES, LIB, device_code  # noqa: F401  (device_code: the fixture)
from policy_common import dense_rows, weights
from value_common import ROLLOUT_POLICY_VALUE, matrix_product_value, value_as_logit_set, value_weights

NEW_SYMBOLS = ["cz_load_value_device", "cz_value_sets", "cz_value_device", "cz_rollout_policy_value"]

libm = C.CDLL(ctypes.util.find_library("m"))
libm.fmaf.restype = C.c_float
libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


def scalar_value(x, w1, b1, wv, bv):
    """the definition in Python loops over libm's fmaf and numpy float32 scalars"""
    h = []
    for j in range(policy.HIDDEN):
        acc = np.float32(b1[j])
        for f in range(len(x)):
            acc = np.float32(libm.fmaf(float(w1[j][f]), float(x[f]), float(acc)))
        h.append(acc if acc > 0 else np.float32(0))
    p = [np.float32(wv[j]) * h[j] for j in range(policy.HIDDEN)]
    for k in range(6):
        p = [np.float32(p[j] + p[j ^ (1 << k)]) for j in range(policy.HIDDEN)]
    assert len({np.float32(v).view(np.uint32) for v in p}) == 1, "after six levels every lane holds one value"
    return np.float32(p[0] + np.float32(bv[0]))


@pytest.mark.parametrize("F", [5, 128, 283])
def test_host_value_equals_the_scalar_model(F):
    W, V = weights(F, 5, 2, F), value_weights(2, F)
    x = dense_rows(3, 2, F, F)
    for s in range(2):
        got = policy.host_value(x, W[0][s], W[1][s], V[0][s], V[1][s])
        assert got.shape == (3, 2) and got.dtype == np.float32
        want = np.array([[scalar_value(x[i, a], W[0][s], W[1][s], V[0][s], V[1][s]) for a in range(2)] for i in range(3)], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # torch's own shapes: weight [1, 64], bias [1]
    assert np.array_equal(policy.host_value(x, W[0][0], W[1][0], V[0][0][None], V[1][0]).view(np.uint32),
                          policy.host_value(x, W[0][0], W[1][0], V[0][0], V[1][0]).view(np.uint32))
    with pytest.raises(ValueError):
        policy.host_value(x, W[0][0], W[1][0], V[0][0][:63], V[1][0])


def test_hand_cases_give_known_bits_for_any_finite_row():
    F = 37
    x = dense_rows(6, 3, F, 1) * np.float32(100.0)
    for v in (0.75, -3.1415927, 1e-3, 12345.678):
        v = np.float32(v)
        w1, b1 = np.zeros((policy.HIDDEN, F), np.float32), np.zeros(policy.HIDDEN, np.float32)
        b1[0] = 1.0                                                # hidden unit 0 is 1.0, the others 0.0: the butterfly adds zeros to v
        wv, bv = np.zeros(policy.HIDDEN, np.float32), np.zeros(1, np.float32)
        wv[0] = v
        got = policy.host_value(x, w1, b1, wv, bv)
        assert (got.view(np.uint32) == v.view(np.uint32)).all(), v
        # a dead hidden layer: every unit 0.0, an ordinary wv - the value is bv's bits
        dead_wv = value_weights(1, 9)[0][0]
        got = policy.host_value(x, w1, np.full(policy.HIDDEN, -1.0, np.float32), dead_wv, np.array([v], np.float32))
        assert (got.view(np.uint32) == v.view(np.uint32)).all(), v


@pytest.mark.parametrize("Cn", [5, 8])
def test_a_value_is_the_logit_of_a_set_whose_output_row_is_the_value_head(Cn):
    F = 131
    W, V = weights(F, Cn, 2, 3), value_weights(2, 4)
    x = dense_rows(7, 2, F, 5)
    for s in range(2):
        want = policy.host_value(x, W[0][s], W[1][s], V[0][s], V[1][s])
        for c in (0, Cn // 2, Cn - 1):
            lg = policy.host_logits(x, *value_as_logit_set(W[0][s], W[1][s], V[0][s], V[1][s], Cn, c))
            assert np.array_equal(lg[..., c].view(np.uint32), want.view(np.uint32)), (s, c)
        assert not np.array_equal(policy.host_logits(x, W[0][s], W[1][s], W[2][s], W[3][s])[..., 0].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("F", [128, 283, 385])
def test_the_matrix_product_form_gives_other_bits_on_dense_rows(F):
    W, V = weights(F, 5, 2, F + 1), value_weights(2, F + 1)
    x = dense_rows(40, 2, F, F + 1).reshape(-1, F)
    differ = total = 0
    for s in range(2):
        want = policy.host_value(x, W[0][s], W[1][s], V[0][s], V[1][s]).view(np.uint32)
        differ += int((matrix_product_value(x, W[0][s], W[1][s], V[0][s], V[1][s]).view(np.uint32) != want).sum())
        total += want.size
        swapped = W[0][s].copy()
        swapped[:, [F - 2, F - 1]] = W[0][s][:, [F - 1, F - 2]]
        same = int((policy.host_value(x, swapped, W[1][s], V[0][s], V[1][s]).view(np.uint32) == want).sum())
        assert same == 0, f"the last two columns of W1 exchanged give the same value in {same} rows"
    share = differ / total
    print(f"F = {F}: {share:.1%} of the values differ from the matrix-product form")
    assert share >= 0.25, f"only {share:.1%} of the values differ from the matrix-product form: a comparison in bits shows nothing"


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_and_the_abi_number_stays_ten():
    from cooking_zoo_amd import _abi, _native
    text = open(HEADER).read()
    assert re.search(r"^int cz_load_value_device\(cz_handle h, int32_t n_sets, const float \*d_wv, const float \*d_bv\);", text, flags=re.M)
    assert re.search(r"^int32_t cz_value_sets\(cz_handle h\);", text, flags=re.M)
    assert re.search(r"^int cz_value_device\(cz_handle h, int64_t rows, const float \*d_obs32, uint32_t vsets, float \*d_values\);", text, flags=re.M)
    assert re.search(r"^int cz_rollout_policy_value\(cz_handle h, int32_t T, uint32_t sets, uint32_t vsets, int32_t mode, uint64_t seed, uint32_t step0,"
                     r"\s+float \*d_obs32, int32_t \*d_actions, float \*d_logits, float \*d_values, double \*d_rewards,"
                     r"\s+uint8_t \*d_terminations, uint8_t \*d_truncations\);", text, flags=re.M)
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
    assert [len(bound[n]) for n in NEW_SYMBOLS] == [4, 1, 5, 14]


def test_python_layer_has_the_methods():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for cls in (CookingVecEnv, ShardedVecEnv):
        assert list(inspect.signature(cls.load_value).parameters) == ["self", "wv", "bv"]
        assert list(inspect.signature(cls.value_device).parameters) == ["self", "d_obs32", "d_values", "vsets", "rows"]
        assert list(inspect.signature(cls.rollout_policy_value).parameters) == ["self", "T", "d_obs32", "d_values", "d_actions", "d_logits", "d_rewards",
                                                                                "d_term", "d_trunc", "sets", "vsets", "mode", "seed", "step0"]
        assert inspect.signature(cls.rollout_policy_value).parameters["vsets"].default is None
        assert isinstance(cls.value_sets, property)
    assert policy.pack_sets((None, 1, 0), 3) == 0xFF0001FF


def test_every_instance_has_its_value_rollout_kernels(device_code):  # noqa: F811
    meta, code = device_code
    names = [(inst, f"_ZN2cz6k_stepILi{opl}ELi{cpl}ELi{na}ELi{scheme}ELi{ROLLOUT_POLICY_VALUE}EEEvPjPKiPKdiiiiiiiNS_6ParamsE")
             for inst, (opl, cpl) in INSTANCES.items() for na in (1, 2, 3, 4) for scheme in (1, 3)]
    assert len(names) == 24
    missing = [(inst, k) for inst, k in names if k not in meta or k not in code]
    assert not missing, missing
    for _, k in names:
        assert any(l.startswith(("v_fma_f32", "v_fmac_f32")) for l in code[k]), k
    for na in (1, 2, 3, 4):
        assert f"_ZN2cz7k_valueILi{na}EEEvNS_9ValueArgsE" in meta
    assert any(k.startswith("_ZN2cz12k_value_packILi0EEE") for k in meta)
