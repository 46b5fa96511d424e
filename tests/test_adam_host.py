"""CPU: the definition of cz_adam_step_device (cooking_zoo_amd/adam.py) - the vectorised model against the scalar second model as bits,
hand cases, the model against float64 Adam with beta**t bias correction within a derived bound, the pinned order of the norm's sum,
and the entry points in header, library and binding with the ABI number still 10."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from cooking_zoo_amd import adam
from adam_common import U32, gradients, mid_state, pad6, reference_steps, same, tensors
from ppo_common import canon

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cookingzoo.h")
LIB = os.path.join(REPO, "cooking_zoo_amd", "csrc", "libcookingzoo_hip.so")
NEW_SYMBOLS = ["cz_sizeof_params", "cz_adam_chunk", "cz_adam_reserve", "cz_adam_step_device"]
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-5, weight_decay=0.01, max_norm=0.5)


def three_steps(step, P, M, V, state, mask, F, C, n, value, seed, **hyper):
    for k in range(3):
        P, M, V, state = step(P, gradients(F, C, n, seed + k, value), M, V, state, mask, **hyper)
    return P, M, V, state


# (sets loaded, mask, F, C, value tensors): F = 17 makes w1 1088 elements a set - a whole chunk and a remainder of 64
MODEL_CASES = [(n, (1 << n) - 1, 17, 5, n % 2 == 1) for n in (1, 2, 3, 4)] + [(3, mask, 5, 8, mask % 2 == 0) for mask in range(1, 8)]


@pytest.mark.parametrize("case", MODEL_CASES, ids=[f"n{c[0]}-mask{c[1]:03b}-{'value' if c[4] else 'novalue'}" for c in MODEL_CASES])
def test_the_vectorised_model_is_the_scalar_model_in_bits(case):
    n, mask, F, Cn, value = case
    P, M, V = tensors(F, Cn, n, n + mask, value)
    hyper = dict(HYPER, weight_decay=0.01 if mask % 2 else 0.0, max_norm=0.5 if n % 2 else 0.0)
    a = three_steps(adam.host_adam_step, P, M, V, adam.fresh_state(), mask, F, Cn, n, value, 10 * n + mask, **hyper)
    b = three_steps(adam.scalar_adam_step, P, M, V, adam.fresh_state(), mask, F, Cn, n, value, 10 * n + mask, **hyper)
    same(f"{case}", a, b)
    assert a[3][0] == 3.0 and a[3][5] == 0.0 and a[3][7] == 0.0 and a[3][6] == hyper["lr"]
    assert a[3][1] == (0.9 * 0.9) * 0.9 and (hyper["max_norm"] == 0) == (a[3][4] == 1.0)
    for k in range(n):                                         # a set outside the mask is untouched; a set inside moved everywhere
        for i in range(6 if value else 4):
            moved = canon(a[0][i][k]) != canon(P[i][k])
            assert moved.mean() > 0.99 if (mask >> k) & 1 else not moved.any(), f"set {k}, tensor {i}"
            assert ((mask >> k) & 1) or (np.array_equal(a[1][i][k], M[i][k]) and np.array_equal(a[2][i][k], V[i][k]))


def tiny(F=1, n=1, fill=0.0):
    """groups whose tensors are all `fill`, of the smallest shapes: w1 [n][64][F], ..."""
    from adam_common import shapes
    return pad6([np.full(s, fill, np.float32) for s in shapes(F, 5, n, False)])


def test_one_element_by_hand():
    """a single non-zero gradient element: every number of the step written out"""
    G, P, M, V = tiny(), tiny(fill=0.5), tiny(), tiny()
    G[0][0, 3, 0] = 0.25
    P2, M2, V2, st = adam.host_adam_step(P, G, M, V, adam.fresh_state(), 1, lr=0.1, beta1=0.5, beta2=0.75, eps=0.125, max_norm=0.0)
    # norm 0.25; m = 0.5 * 0.25 = 0.125; v = 0.25 * 0.0625 = 0.015625; mh = 0.125 / 0.5 = 0.25; vh = 0.015625 / 0.25 = 0.0625; sqrt 0.25
    assert st.tolist() == [1.0, 0.5, 0.75, 0.25, 1.0, 0.0, 0.1, 0.0]
    assert M2[0][0, 3, 0] == 0.125 and V2[0][0, 3, 0] == 0.015625
    assert P2[0][0, 3, 0] == np.float32(0.5 - 0.1 * (0.25 / (0.25 + 0.125)))
    # every other element: m = v = 0 and the parameter stays
    others = np.ones(P[0].shape, bool)
    others[0, 3, 0] = False
    assert (P2[0][others] == 0.5).all() and (M2[0][others] == 0).all() and all((p == 0.5).all() for p in P2[1:4])
    # clipped to half its norm: the moments see 0.125
    _, M3, _, st3 = adam.host_adam_step(P, G, M, V, adam.fresh_state(), 1, lr=0.1, beta1=0.5, beta2=0.75, eps=0.125, max_norm=0.125)
    assert st3[4] == 0.125 / (0.25 + 1e-6) and M3[0][0, 3, 0] == np.float32(0.5 * (st3[4] * 0.25))


def test_a_zero_gradient_moves_the_parameters_by_weight_decay_alone():
    P, M, V = tiny(fill=0.75), tiny(), tiny()
    P2, M2, V2, st = adam.host_adam_step(P, tiny(), M, V, adam.fresh_state(), 1, lr=0.5, eps=1e-8, weight_decay=0.25, max_norm=1.0)
    assert st[3] == 0.0 and st[4] == 1.0 and st[0] == 1.0
    assert all((p == np.float32(0.75 - (0.5 * 0.25) * 0.75)).all() for p in P2[:4]) and all((m == 0).all() for m in M2[:4] + V2[:4])
    P3 = adam.host_adam_step(P, tiny(), M, V, adam.fresh_state(), 1, lr=0.5, eps=1e-8, weight_decay=0.0)[0]
    assert all(np.array_equal(a, b) for a, b in zip(P3[:4], P[:4]))


def test_a_max_norm_above_the_norm_is_the_unclipped_run():
    P, M, V = tensors(9, 5, 2, 1)
    G = gradients(9, 5, 2, 1)
    norm = float(np.sqrt(adam.grad_total(G, 3)))
    a = adam.host_adam_step(P, G, M, V, mid_state(), 3, **dict(HYPER, max_norm=norm * 1.5))
    b = adam.host_adam_step(P, G, M, V, mid_state(), 3, **dict(HYPER, max_norm=0.0))
    assert a[3][4] == 1.0 and a[3][3] == norm
    same("max_norm above the norm", a, b)
    c = adam.host_adam_step(P, G, M, V, mid_state(), 3, **dict(HYPER, max_norm=norm * 0.5))
    assert 0.49 < c[3][4] < 0.5 and not np.array_equal(c[0][0], a[0][0])


@pytest.mark.parametrize("elements", (1023, 1024, 1025))
def test_the_chunk_edge(elements):
    """a segment of 1023, 1024 and 1025 elements: the partials by hand, and both models through a step"""
    rng = np.random.default_rng(elements)
    seg = (rng.standard_normal(elements) * 0.1).astype(np.float32)
    parts = adam.chunk_partials(seg)
    assert len(parts) == (1 if elements <= 1024 else 2)
    sq = np.zeros(2048)
    sq[:elements] = seg.astype(np.float64) ** 2
    for c, part in enumerate(parts):
        lane = [((sq[1024 * c + l] + sq[1024 * c + l + 256]) + sq[1024 * c + l + 512]) + sq[1024 * c + l + 768] for l in range(256)]
        for k in range(8):
            lane = [lane[l] + lane[l ^ (1 << k)] for l in range(256)]
        assert len(set(lane)) == 1 and lane[0] == part
    # w1 segments of that many elements do not exist (64 F), so the edge goes through the models as sets: F = 16 is 1024 a set, and one
    # element more or less is the neighbouring tensor's business; F = 15, 16, 17 gives 960, 1024, 1088
    F = 15 + (elements - 1023)
    P, M, V = tensors(F, 5, 2, elements)
    G = gradients(F, 5, 2, elements)
    same(f"F = {F}", adam.host_adam_step(P, G, M, V, mid_state(), 2, **HYPER), adam.scalar_adam_step(P, G, M, V, mid_state(), 2, **HYPER))


@pytest.mark.parametrize("poison", (np.inf, -np.inf, np.nan))
def test_a_gradient_that_is_not_finite_skips_the_call(poison):
    P, M, V = tensors(7, 5, 3, 2)
    for step in (adam.host_adam_step, adam.scalar_adam_step):
        G = gradients(7, 5, 3, 2)
        G[2][1, 4, 60] = poison
        state = mid_state(5)
        state[5] = 2.0
        P2, M2, V2, st = step(P, G, M, V, state, 0b010, **HYPER)
        for a, b in zip(P2 + M2 + V2, P + M + V):
            assert a.tobytes() == b.tobytes()
        assert st[5] == 3.0 and st[4] == 0.0 and np.array_equal(st[[0, 1, 2, 6, 7]], state[[0, 1, 2, 6, 7]])
        # the poisoned set outside the mask: not read at all
        P3, _, _, st3 = step(P, G, M, V, state, 0b101, **HYPER)
        assert st3[5] == 2.0 and st3[0] == 6.0 and np.isfinite(st3[3]) and not np.array_equal(P3[0][0], P[0][0])


def test_the_model_against_float64_adam_within_the_derived_bound():
    """Twenty steps from zero moments with clipping and weight decay, against Adam in float64 throughout - float64 moments, bias
    correction 1 - beta**t, numpy's own norm (adam_common.reference_steps).  The bound is propagated beside the reference, element by
    element, from the roundings of adam.py and nothing else: the two coefficients differ by 2 (count + 4) 2^-53 relative (a float64
    sum of exact squares in any order, sqrt, +, /); a moment carries beta times its earlier error, the gradient's, a few float64
    roundings and one float32 store of 2^-24 relative; bc differs by (t + 3) 2^-53; sqrt moves by at most min(sqrt(e), e / sqrt(vh));
    the quotient's error follows from numerator and denominator errors; the parameter adds lr times that and one float32 store a step.
    The bound is of the order of 20 float32 roundings of the parameter; it must hold everywhere, be tight enough that the largest
    error uses a tenth of it somewhere, and two mutants must leave it in most elements: eps inside the square root, and no bias
    correction."""
    F, Cn, n, mask, T = 12, 5, 3, 0b101, 20
    hyper = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-3, weight_decay=0.01, max_norm=0.5)
    P = tensors(F, Cn, n, 3)[0]
    grads = [gradients(F, Cn, n, 100 + t) for t in range(T)]
    zero = lambda: [np.zeros_like(p) for p in P]
    got, M, V, state = P, zero(), zero(), adam.fresh_state()
    coefs = []
    for G in grads:
        got, M, V, state = adam.host_adam_step(got, G, M, V, state, mask, **hyper)
        coefs.append(state[4])
    assert state[0] == T and min(coefs) < 0.9, "the run never clips: the coefficient's path is not exercised"
    ref, bounds = reference_steps(P, grads, mask, **hyper)
    worst, inside_of = 0.0, {}
    for i in range(6):
        for k in (0, 2):
            err = np.abs(got[i][k].astype(np.float64) - ref[i][k])
            assert (err <= bounds[i][k]).all(), f"tensor {i}, set {k}: {int((err > bounds[i][k]).sum())} elements outside the derived bound"
            assert (bounds[i][k] <= 64 * U32 * np.maximum(np.abs(ref[i][k]), 0.05)).all(), "the bound is no longer of the order of the roundings"
            worst = max(worst, float((err / bounds[i][k]).max()))
        assert np.array_equal(got[i][1], P[i][1])
    assert worst > 0.1, f"the largest error uses {worst:.3f} of its bound: the bound is too loose to tell anything"
    for mutant in ("eps_inside", "no_bias_correction"):
        mref = reference_steps(P, grads, mask, mutant=mutant, **hyper)[0]
        outside = np.concatenate([(np.abs(got[i][k].astype(np.float64) - mref[i][k]) > bounds[i][k]).reshape(-1) for i in range(6) for k in (0, 2)])
        inside_of[mutant] = 1.0 - outside.mean()
        assert outside.mean() > 0.9, f"mutant {mutant}: only {outside.mean():.3f} of the elements leave the bound"


def test_the_pinned_order_of_the_norm_is_observable():
    """the chunked butterfly order against one serial chain over the same squares (np.cumsum adds strictly left to right): the two
    totals differ in more than half of 200 draws (measured: in all 200), so a device that summed in another order would be seen"""
    differ = 0
    for seed in range(200):
        G = gradients(20, 5, 2, seed)
        squares = np.concatenate([(g[k].astype(np.float64) ** 2).reshape(-1) for g in G for k in range(2)])
        differ += float(np.cumsum(squares)[-1]) != float(adam.grad_total(G, 3))
    print(f"the pinned order differs from one serial chain in {differ} of 200 draws")
    assert differ > 100


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_and_the_abi_number_stays_ten():
    from cooking_zoo_amd import _abi, _native
    text = open(HEADER).read()
    assert re.search(r"^typedef struct cz_params \{ float \*w1, \*b1, \*w2, \*b2, \*wv, \*bv; \} cz_params;", text, flags=re.M)
    assert re.search(r"^#define CZ_ADAM_KEEP_TABLE 1u$", text, flags=re.M)
    assert re.search(r"^int32_t cz_sizeof_params\(void\);", text, flags=re.M)
    assert re.search(r"^int32_t cz_adam_chunk\(void\);", text, flags=re.M)
    assert re.search(r"^int cz_adam_reserve\(cz_handle h\);", text, flags=re.M)
    assert re.search(r"^int cz_adam_step_device\(cz_handle h, uint32_t set_mask, const cz_params \*params, const cz_params \*grads,"
                     r"\s+const cz_params \*exp_avg, const cz_params \*exp_avg_sq, double \*d_state,"
                     r"\s+double lr, const double \*d_lr /\* may be NULL \*/, double beta1, double beta2, double eps,"
                     r"\s+double weight_decay, double max_norm, uint32_t flags\);", text, flags=re.M)
    assert "cooking_zoo_amd/adam.py" in text
    assert _native.header_abi_version() == 10 == _abi.CZ_ABI_VERSION
    lib = C.CDLL(LIB)
    for name in ("cz_abi_version", "cz_adam_chunk", "cz_sizeof_params"):
        getattr(lib, name).restype = C.c_int32
    assert lib.cz_abi_version() == 10 and lib.cz_adam_chunk() == adam.ADAM_CHUNK == 1024
    assert lib.cz_sizeof_params() == C.sizeof(_native.CzParams) == 6 * C.sizeof(C.c_void_p) and _native.CZ_ADAM_KEEP_TABLE == 1


def test_library_exports_binding_python_layer_and_the_refusals_that_need_no_device():
    from cooking_zoo_amd import _native
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    lib = C.CDLL(LIB)
    bound = {name: args for name, _, args in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name + " is not exported"
        assert name in bound and name in _native.ADDED_SYMBOLS, name
    assert [len(bound[n]) for n in NEW_SYMBOLS] == [0, 0, 1, 15]
    assert list(inspect.signature(CookingVecEnv.adam_reserve).parameters) == ["self"]
    sig = inspect.signature(CookingVecEnv.adam_step_device).parameters
    assert list(sig) == ["self", "params", "grads", "exp_avg", "exp_avg_sq", "d_state", "sets", "lr", "d_lr", "betas", "eps", "weight_decay",
                         "max_norm", "keep_table"]
    assert [sig[k].default for k in list(sig)[6:]] == [None, 1e-3, None, (0.9, 0.999), 1e-8, 0.0, 0.0, False]
    assert not hasattr(ShardedVecEnv, "adam_step_device"), "gradients over shards still lack their all-reduce: no optimiser there"
    # a null handle is refused before anything else is looked at
    lib.cz_last_error.restype = C.c_char_p
    lib.cz_adam_reserve.argtypes = [C.c_void_p]
    lib.cz_adam_step_device.argtypes = bound["cz_adam_step_device"]
    assert lib.cz_adam_reserve(None) == 1 and b"null handle" in lib.cz_last_error(None)
    group = _native.CzParams()
    assert lib.cz_adam_step_device(None, 1, C.byref(group), C.byref(group), C.byref(group), C.byref(group), None, 1e-3, None, 0.9, 0.999, 1e-8,
                                   0.0, 0.0, 0) == 1
    # the models refuse what the call refuses
    P, M, V = tensors(4, 5, 2, 0)
    G = gradients(4, 5, 2, 0)
    for mask in (0, 4, 7):
        with pytest.raises(ValueError, match="set_mask"):
            adam.host_adam_step(P, G, M, V, adam.fresh_state(), mask)
    with pytest.raises(ValueError, match="together"):
        adam.host_adam_step(P[:5] + [None], G, M, V, adam.fresh_state(), 1)
    with pytest.raises(ValueError, match="presence of the value tensors"):
        adam.host_adam_step(P, G[:4] + [None, None], M, V, adam.fresh_state(), 1)
    assert adam.fresh_state().tolist() == [0, 1, 1, 0, 0, 0, 0, 0] and adam.fresh_state().dtype == np.float64
