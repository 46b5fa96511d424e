"""CPU: the definition of cz_ppo_grad_device (cooking_zoo_amd/ppo.py) - the vectorised model against the scalar second model as bits,
hand cases, cz_exp on [0, 64], the model against torch float64 autograd within a derived bound, the pinned summation order, a census
of the cases the inputs reach, and the entry points in header, library and binding with the ABI number still 10."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cooking_zoo_amd import policy, ppo
from policy_common import weights
from ppo_common import canon, gamma, grad_bound, trajectory
from targets_common import ACT_OUTSIDE
from value_common import value_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cookingzoo.h")
LIB = os.path.join(REPO, "cooking_zoo_amd", "csrc", "libcookingzoo_hip.so")
NEW_SYMBOLS = ["cz_ppo_reserve", "cz_ppo_reserved", "cz_ppo_chunk", "cz_ppo_grad_device"]
NAMES = ("gw1", "gb1", "gw2", "gb2", "gwv", "gbv")
COEF = dict(clip=0.2, c_value=0.5, c_entropy=0.01)


def same(ctx, a, b):
    for name, u, v in zip(NAMES, a[0], b[0]):
        bad = np.argwhere(canon(u) != canon(v))
        assert not len(bad), f"{ctx}: {name} differs in bits in {len(bad)} of {u.size} elements, first at {bad[0].tolist()}"
    assert np.array_equal(canon(a[1]), canon(b[1])), f"{ctx}: statistics {a[1].tolist()} and {b[1].tolist()}"


# (R, A, F, C, sets, vsets, positions of an index or None): small enough for the scalar model's exact rational fmaf
SCALAR_CASES = [(5, 2, 6, 5, (0, 1), (0, 2), None), (70, 2, 5, 5, (1, None), (1, 0), 67), (9, 3, 4, 8, (0, 0, None), (None, 1, 1), None),
                (66, 1, 3, 8, (2,), (2,), 130), (4, 4, 5, 5, (0, 1, 2, None), (None, None, None, None), None)]


@pytest.mark.parametrize("case", SCALAR_CASES, ids=[f"R{c[0]}-A{c[1]}-F{c[2]}-C{c[3]}" for c in SCALAR_CASES])
def test_the_vectorised_model_is_the_scalar_model_in_bits(case):
    R, A, F, Cn, sets, vsets, M = case
    W, V = weights(F, Cn, 3, R + F, scale2=0.3), value_weights(3, R)
    data = trajectory(R, A, F, W, sets, R + A)
    index = None if M is None else np.random.default_rng(R).integers(-1, R + 1, M)
    a = ppo.host_ppo_grad(*data, W, V, sets, vsets, index=index, **COEF)
    b = ppo.scalar_ppo_grad(*data, W, V, sets, vsets, index=index, **COEF)
    same(f"{case}", a, b)
    assert a[1][5] > 0 or a[1][6] > 0
    if M is not None:
        assert a[1][7] > 0, "no index out of range: the case shows nothing"
    assert any(np.abs(g).max() > 0 for g in a[0])


def test_hand_cases_one_position_all_clipped_and_no_entropy_term():
    F, Cn = 6, 5
    W, V = weights(F, Cn, 2, 3, scale2=0.3), value_weights(2, 3)
    x, act, lpo, adv, ret = trajectory(8, 1, F, W, (0,), 1)
    act[:] = np.arange(8)[:, None] % Cn                          # every action inside the range
    # one position, no critic, no entropy term, a clip nothing reaches: g_c = -(Adv * ratio) * (delta_c,act - p_c), db2 is g itself
    one = (x[:1], act[:1], lpo[:1], adv[:1], ret[:1])
    (gw1, gb1, gw2, gb2, gwv, gbv), st = ppo.host_ppo_grad(*one, W, None, (0,), (None,), clip=10.0, c_value=0.5, c_entropy=0.0)
    h = policy.host_hidden(x[0, 0], W[0][0], W[1][0])
    z, L = ppo.targets.logprob64(policy.host_heads(h[None], W[2][0], W[3][0]))
    q = z[0] - L[0]
    ratio = policy.cz_exp(np.float64(np.float32(q[act[0, 0]])) - np.float64(lpo[0, 0]))
    want = (-(np.float64(adv[0, 0]) * ratio) * ((np.arange(Cn) == act[0, 0]) - policy.cz_exp(q))).astype(np.float32)
    assert np.array_equal(gb2[0], want), (gb2[0], want)
    assert (gw1[1] == 0).all() and (gwv == 0).all() and (gbv == 0).all() and st[5] == 1 and st[6] == 0
    assert np.array_equal(gw2[0], want[:, None] * h[None, :])     # one pass: dW2[c][j] = fmaf(g_c, h_j, 0) = the rounded product
    # an all-clipped minibatch without an entropy term: exactly zero policy gradient, in every tensor; the value part is untouched
    far = lpo - np.float32(3.0) * np.sign(adv)                    # ratio around e^(+-3), on the advantage's side of the interval
    data = (x, act, far, adv, ret)
    (gw1, gb1, gw2, gb2, gwv, gbv), st = ppo.host_ppo_grad(*data, W, V, (0,), (1,), clip=0.2, c_value=0.5, c_entropy=0.0)
    assert st[4] == 1.0 and st[5] == 8, st
    assert (gw1[0] == 0).all() and (gb1[0] == 0).all() and (gw2 == 0).all() and (gb2 == 0).all()
    assert np.abs(gw1[1]).max() > 0 and np.abs(gwv[1]).max() > 0 and gbv[1, 0] != 0
    # ... and with the entropy term that term alone is left: the gradient of -c_entropy * mean H
    with_h = ppo.host_ppo_grad(*data, W, V, (0,), (1,), clip=0.2, c_value=0.5, c_entropy=0.01)
    assert np.abs(with_h[0][2][0]).max() > 0 and np.abs(with_h[0][3][0].sum()) < 1e-8          # (the softmax's gradients sum to zero over c)
    # c_entropy = 0 and c_value = 0 with nothing clipped
    free = ppo.host_ppo_grad(x, act, lpo, adv, ret, W, V, (0,), (0,), clip=10.0, c_value=0.0, c_entropy=0.0)
    assert free[1][4] == 0.0 and (free[0][4] == 0).all() and np.abs(free[0][0][0]).max() > 0
    same("scalar, clip 10", free, ppo.scalar_ppo_grad(x, act, lpo, adv, ret, W, V, (0,), (0,), clip=10.0, c_value=0.0, c_entropy=0.0))


def test_cz_exp_on_the_widened_domain():
    z = np.concatenate([np.linspace(0.0, 64.0, 200001), np.random.default_rng(0).uniform(-64.0, 64.0, 200000), [64.0, -64.0, 0.0]])
    rel = np.abs(policy.cz_exp(z) / np.exp(z) - 1.0)
    print(f"cz_exp on [-64, 64]: largest relative error against np.exp {rel.max():.3g}")
    assert rel.max() <= 2.3e-16 and policy.cz_exp(0.0) == 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# against torch float64 autograd
# ---------------------------------------------------------------------------------------------------------------------------

TORCH_CASE = dict(R=200, A=2, F=16, C=5, M=150, sets=(0, 1), vsets=(0, 2), seed=1)


def torch_case():
    c = TORCH_CASE
    W, V = weights(c["F"], c["C"], 3, c["seed"], scale2=0.15), value_weights(3, c["seed"])
    data = trajectory(c["R"], c["A"], c["F"], W, c["sets"], c["seed"])
    index = np.random.default_rng(c["seed"]).integers(-1, c["R"] + 1, c["M"])
    return W, V, data, index


def autograd_reference(tmp_path, W, V, data, index, sets, vsets):
    """the three variants' float64 gradients from a child interpreter: this one must not import torch (cooking_zoo_amd/_native.py
    refuses a torch that arrives after the library)"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    params = list(W) + [V[0], V[1]]
    np.savez(src, obs=data[0], act=data[1], lpo=data[2], adv=data[3], ret=data[4], idx=np.asarray(index, np.int64),
             sets=np.array([-1 if s is None else s for s in sets]), vsets=np.array([-1 if s is None else s for s in vsets]),
             coef=np.array([COEF["clip"], COEF["c_value"], COEF["c_entropy"]]), **{f"p{i}": p for i, p in enumerate(params)})
    p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "ppo_torch_ref.py"), src, dst], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    out = np.load(dst)
    return [[out[f"v{k}_g{i}"] for i in range(6)] for k in range(3)]


def test_the_model_against_torch_float64_autograd_within_the_derived_bound(tmp_path):
    """Every element of host_ppo_grad stays within a bound derived from the arithmetic, not tuned: u = 2^-24, gamma_k = k u / (1 - k u).

    Forward.  acc_j runs F fmafs behind the bias: |pre_j - pre64_j| <= e1_j = gamma_(F+1) (|x| . |W1_j| + |b1_j|); ReLU is 1-Lipschitz,
    so e1 bounds h too, PROVIDED no float64 pre-activation lies within e1 of zero (asserted; then both arithmetics have the same
    live units).  A head (64 products, six levels, the bias - well inside gamma_70, the figure tests/test_gpu_zz_value_torch.py uses):
    el_c = gamma_70 ((|h| + e1) . |W2_c| + |b2_c|) + e1 . |W2_c|, likewise ev for the value.  log-softmax moves by at most the
    largest logit error, so |dq_c| <= eq_c = el_c + max el (+ Q64, the float64 head's own error, counted in ppo_common); dp_c = p_c (e^eq_c -
    1); dH = sum(dp |q| + p eq + dp eq); the ratio moves by dr = ratio (e^(eq_act + u (|q_act| + 1)) - 1) - q_act is rounded to float32 once -, PROVIDED no float64 ratio lies within dr of 1
    +- eps where the advantage is not zero (asserted; then both clip the same samples).  dglp = |Adv| dr where unclipped, and
    dg_c = inv_p (dglp |delta - p_c| + (|glp| + dglp) dp_c + c_entropy (dp_c |q_c + H| + (p_c + dp_c)(eq_c + dH))) + u (|g_c| + ...)
    for the one rounding to float32; dgv = inv_v c_value ev + u |gv|.

    Backward of a pass.  dh_j is a chain of C (+ 1) fmafs: edh_j = gamma_(C+1) (|g| . |W2_.j| + |gv| |wv_j|) + dg . |W2_.j| + dgv |wv_j|;
    da has the same live units.  Accumulation.  An element's sum is a chain of at most L fmafs or adds within a chunk (L: the most
    passes one chunk sends into the set) and one add per chunk: gamma_(L + chunks) times the sum of the terms' magnitudes, plus the
    terms' own propagated errors - dW2: sum((|g_c| + dg_c)(|h_j| + e1_j)) and sum(dg_c (|h_j| + e1_j) + |g_c| e1_j); db2: sum |g_c|,
    sum dg_c; dwv / dbv the same with gv; db1: sum(|da_j| + eda_j), sum eda_j; dW1: the same times |x_f|.  (ppo_common.grad_bound.)"""
    c = TORCH_CASE
    W, V, data, index = torch_case()
    sets, vsets = c["sets"], c["vsets"]
    bounds, margin_pre, margin_ratio = grad_bound(data, W, V, sets, vsets, index, **COEF)
    assert margin_pre > 0, f"a float64 pre-activation lies within its forward bound of zero ({margin_pre:.3g}): choose another seed"
    assert margin_ratio > 0, f"a float64 ratio lies within its bound of 1 +- eps ({margin_ratio:.3g}): choose another seed"
    got, stats = ppo.host_ppo_grad(*data, W, V, sets, vsets, index=index, **COEF)
    assert stats[4] > 0 and stats[5] > 0 and stats[6] > 0 and stats[7] > 0
    ref, no_clip, flipped = autograd_reference(tmp_path, W, V, data, index, sets, vsets)
    for name, g, r, b in zip(NAMES, got, ref, bounds):
        r = r.reshape(g.shape)
        err = np.abs(g.astype(np.float64) - r)
        print(f"{name}: largest error / bound {float((err / np.maximum(b, 1e-300)).max()):.3f}, largest bound {b.max():.3g}, largest gradient {np.abs(r).max():.3g}")
        assert (err <= b).all(), f"{name}: {int((err > b).sum())} of {err.size} elements outside the bound, worst {float((err / b).max()):.3f}"
        assert b.max() < 1e-3 * np.abs(r).max(), f"{name}: the bound {b.max():.3g} says nothing about gradients of {np.abs(r).max():.3g}"
    # the wrong variants fall outside: the policy sets' four tensors (the critic's own set and the value heads do not see the policy loss)
    for what, wrong in (("the clip ignored", no_clip), ("the entropy term's sign flipped", flipped)):
        out = total = 0
        for k in (0, 1, 2, 3):
            for s in {s for s in sets if s is not None}:
                out += int((np.abs(got[k][s].astype(np.float64) - wrong[k].reshape(got[k].shape)[s]) > bounds[k][s]).sum())
                total += got[k][s].size
        print(f"{what}: {out / total:.1%} of the elements outside the bound")
        assert out / total > 0.9, f"{what}: only {out / total:.1%} of the elements outside the bound: the comparison shows nothing"


def test_the_summation_order_is_pinned_and_the_census_of_cases():
    W, V, data, index = torch_case()
    c = TORCH_CASE
    chunked, st = ppo.host_ppo_grad(*data, W, V, c["sets"], c["vsets"], index=index, **COEF)
    chain, st1 = ppo.host_ppo_grad(*data, W, V, c["sets"], c["vsets"], index=index, chunk=1 << 20, **COEF)
    differ = sum(int((canon(a) != canon(b)).sum()) for a, b in zip(chunked, chain))
    total = sum(a.size for a in chunked)
    print(f"chunks of 64 against one chain: {differ / total:.1%} of the gradient elements differ in bits")
    assert differ > 0
    assert np.array_equal(st[4:], st1[4:])                        # counts are exact in any order
    # census: what the inputs of the comparisons above reach
    x, act, lpo, adv, ret = data
    ok = (index >= 0) & (index < c["R"])
    assert (~ok).sum() == st[7] > 0, "an out-of-range row"
    rows = index[ok]
    assert (act[rows] == ACT_OUTSIDE).any(), "an out-of-range action"
    seen = set()
    for a, s in enumerate(c["sets"]):
        h = policy.host_hidden(x[rows, a], W[0][s], W[1][s])
        z, L = ppo.targets.logprob64(policy.host_heads(h, W[2][s], W[3][s]))
        inside = act[rows, a] != ACT_OUTSIDE
        qa = np.take_along_axis(z, np.where(inside, act[rows, a], 0)[:, None], axis=1)[:, 0] - L
        ratio = policy.cz_exp(qa - lpo[rows, a].astype(np.float64))
        for r, A_, i in zip(ratio, adv[rows, a], inside):
            if i:
                seen.add(("above" if r > 1.2 else "below" if r < 0.8 else "inside", "plus" if A_ > 0 else "minus"))
    assert seen == {(w, s) for w in ("above", "below", "inside") for s in ("plus", "minus")}, seen
    assert st[4] > 0 and st[4] < 1


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_and_the_abi_number_stays_ten():
    from cooking_zoo_amd import _abi, _native
    text = open(HEADER).read()
    assert re.search(r"^int cz_ppo_reserve\(cz_handle h, int64_t max_positions\);", text, flags=re.M)
    assert re.search(r"^int64_t cz_ppo_reserved\(cz_handle h\);", text, flags=re.M)
    assert re.search(r"^int32_t cz_ppo_chunk\(void\);", text, flags=re.M)
    assert re.search(r"^int cz_ppo_grad_device\(cz_handle h, int64_t rows, int64_t positions, const int32_t \*d_index /\* may be NULL \*/,"
                     r"\s+const float \*d_obs32, const int32_t \*d_actions, const float \*d_logp_old, const float \*d_adv, const float \*d_ret,"
                     r"\s+uint32_t sets, uint32_t vsets, double clip, double c_value, double c_entropy,"
                     r"\s+float \*d_gw1, float \*d_gb1, float \*d_gw2, float \*d_gb2, float \*d_gwv, float \*d_gbv, double \*d_stats\);", text, flags=re.M)
    assert "cooking_zoo_amd/ppo.py" in text
    assert _native.header_abi_version() == 10 == _abi.CZ_ABI_VERSION
    lib = C.CDLL(LIB)
    lib.cz_abi_version.restype = C.c_int32
    lib.cz_ppo_chunk.restype = C.c_int32
    assert lib.cz_abi_version() == 10 and lib.cz_ppo_chunk() == ppo.PPO_CHUNK == 64


def test_library_exports_binding_and_python_layer():
    from cooking_zoo_amd import _native
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    lib = C.CDLL(LIB)
    bound = {name: args for name, _, args in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name + " is not exported"
        assert name in bound and name in _native.ADDED_SYMBOLS, name
    assert [len(bound[n]) for n in NEW_SYMBOLS] == [2, 1, 0, 21]
    assert list(inspect.signature(CookingVecEnv.ppo_reserve).parameters) == ["self", "max_positions"]
    assert list(inspect.signature(CookingVecEnv.ppo_grad_device).parameters) == ["self", "d_obs32", "d_actions", "d_logp_old", "d_adv", "d_ret", "grads",
                                                                                 "d_index", "sets", "vsets", "clip", "c_value", "c_entropy", "d_stats", "rows"]
    defaults = {k: p.default for k, p in inspect.signature(CookingVecEnv.ppo_grad_device).parameters.items()}
    assert (defaults["clip"], defaults["c_value"], defaults["c_entropy"], defaults["vsets"], defaults["d_index"]) == (0.2, 0.5, 0.01, None, None)
    assert not hasattr(ShardedVecEnv, "ppo_grad_device"), "gradients over shards need an all-reduce: not in this library yet"
