"""Helpers shared by the tests of cz_ppo_grad_device (definition: cooking_zoo_amd/ppo.py): a synthetic trajectory on dense rows whose
old log-probabilities lie around the new ones so that every clipping case occurs, and the guarded device buffers of one call.
(pytest rewrites asserts in test modules only: every assert here carries its own message.)"""
import numpy as np

from cooking_zoo_amd import policy, targets
from policy_common import dense_rows
from targets_common import ACT_OUTSIDE, F32_SENT

GUARD = 64                                                      # sentinel elements before and behind every output
STAT_SENT = 0x7FF8BEEF0BADF00D                                  # float64 outputs, as uint64: a quiet NaN no result equals


def trajectory(R, A, F, W, sets, seed, spread=0.25):
    """-> (x float32 [R][A][F] dense rows, actions int32 [R][A], logp_old, adv, ret float32 [R][A]): the actions uniform over the C
    actions with every 11th entry ACT_OUTSIDE (an agent that did not act), logp_old the model's own log-probability under W plus
    N(0, spread^2) - so the ratio lies on both sides of 1 +- 0.2 - advantages and returns standard normal"""
    rng = np.random.default_rng(5000 + seed)
    C = W[2].shape[1]
    x = dense_rows(R, A, F, seed)
    act = rng.integers(0, C, (R, A)).astype(np.int32)
    act.reshape(-1)[5::11] = ACT_OUTSIDE
    logp = np.zeros((R, A), np.float32)
    for a in range(A):
        s = sets[a] if a < len(sets) and sets[a] is not None else 0
        logp[:, a] = targets.host_logprob(policy.host_logits(x[:, a], W[0][s], W[1][s], W[2][s], W[3][s]), act[:, a])[0]
    logp = (logp + rng.standard_normal((R, A)) * spread).astype(np.float32)
    adv, ret = rng.standard_normal((R, A)).astype(np.float32), rng.standard_normal((R, A)).astype(np.float32)
    return x, act, logp, adv, ret


def canon(a):
    """float bits with -0.0 folded into +0.0: zeros compare equal whatever their sign"""
    a = np.ascontiguousarray(a)
    return (a + a.dtype.type(0)).view(np.uint32 if a.dtype == np.float32 else np.uint64)


class PpoCall:
    """the device side of cz_ppo_grad_device calls on one trajectory: the five inputs, and six gradient buffers plus the statistics
    with GUARD sentinel elements before and behind each"""

    def __init__(self, env, data, n_sets):
        self.env = env
        x, act, logp, adv, ret = data
        self.R = len(x)
        F, C, H = env.F, env.num_actions, policy.HIDDEN
        self.inputs = []
        for v, t in ((x, np.float32), (act, np.int32), (logp, np.float32), (adv, np.float32), (ret, np.float32)):
            b = env.alloc(v.shape, t)
            b.from_host(v)
            self.inputs.append(b)
        self.shapes = [(n_sets, H, F), (n_sets, H), (n_sets, C, H), (n_sets, C), (n_sets, H), (n_sets, 1)]
        self.grads = [env.alloc((int(np.prod(s)) + 2 * GUARD,), np.uint32) for s in self.shapes]
        self.stats = env.alloc((8 + 2 * GUARD,), np.uint64)
        self.index = None

    def set_index(self, index):
        if self.index is not None:
            self.index.free()
        self.index = None
        if index is not None:
            self.index = self.env.alloc((len(index),), np.int32)
            self.index.from_host(np.asarray(index, np.int32))

    def fill(self):
        for b in self.grads:
            b.from_host(np.full(b.shape, F32_SENT, np.uint32))
        self.stats.from_host(np.full(self.stats.shape, STAT_SENT, np.uint64))

    def launch(self, with_value=True, with_stats=True, **kw):
        ptrs = [b.ptr + 4 * GUARD for b in self.grads]
        if not with_value:
            ptrs[4] = ptrs[5] = None
        self.env.ppo_grad_device(*self.inputs, tuple(ptrs), d_index=self.index, d_stats=self.stats.ptr + 8 * GUARD if with_stats else None,
                                 rows=self.R, **kw)

    def get(self, ctx):
        """-> ([six arrays as uint32 in their shapes, sentinels where nothing was written], stats uint64 [8]); asserts the guards"""
        out = []
        for b, s in zip(self.grads, self.shapes):
            h = b.to_host()
            assert (h[:GUARD] == F32_SENT).all() and (h[-GUARD:] == F32_SENT).all(), f"{ctx}: a store outside a gradient buffer of shape {s}"
            out.append(h[GUARD:-GUARD].reshape(s))
        h = self.stats.to_host()
        assert (h[:GUARD] == STAT_SENT).all() and (h[-GUARD:] == STAT_SENT).all(), f"{ctx}: a store outside the statistics"
        return out, h[GUARD:-GUARD]

    def run(self, ctx, **kw):
        self.fill()
        self.launch(**kw)
        self.env.sync()
        return self.get(ctx)

    def free(self):
        self.set_index(None)
        for b in self.inputs + self.grads + [self.stats]:
            b.free()


def check_grads(ctx, got, want, with_value=True, with_stats=True):
    """the device's (gradients, stats) against host_ppo_grad's, as bits with zeros of either sign equal"""
    names = ("gw1", "gb1", "gw2", "gb2", "gwv", "gbv")
    for k, (g, w, name) in enumerate(zip(got[0], want[0], names)):
        if k >= 4 and not with_value:
            assert (g == F32_SENT).all(), f"{ctx}: {name} was written through a null pointer's neighbour"
            continue
        g = canon(g.view(np.float32))
        bad = np.argwhere(g != canon(w))
        assert not len(bad), (f"{ctx}: {name} differs in bits in {len(bad)} of {g.size} elements, first at {bad[0].tolist()}: "
                              f"{g[tuple(bad[0])]:#x} for {canon(w)[tuple(bad[0])]:#x}")
    if with_stats:
        s = canon(got[1].view(np.float64))
        assert np.array_equal(s, canon(want[1])), f"{ctx}: statistics {got[1].view(np.float64).tolist()} for {want[1].tolist()}"
    else:
        assert (got[1] == STAT_SENT).all(), f"{ctx}: statistics were written without a pointer"


# ---------------------------------------------------------------------------------------------------------------------------
# the derived bound of the float32 gradients against a float64 evaluation (tests/test_ppo_host.py carries the derivation)
# ---------------------------------------------------------------------------------------------------------------------------

def gamma(k):
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


U64 = 2.0 ** -53                                                # the unit roundoff of float64
# |q_c - log softmax| of the float64 head before any float32 error: cz_log is within 1e-14 of log on [1, 8] - the bound
# tests/test_targets_host.py asserts -; S is a sum of C <= 8 values of cz_exp (2.2e-16 < 2 U64 relative each) through C - 1 adds, so
# log S moves by at most (2 + 7) U64; z_c and q_c = z_c - L are one rounding each of magnitudes up to 128 (64 and the clamp beyond)
Q64 = 1e-14 + 9 * U64 + 2 * 128 * U64


def grad_bound(data, W, V, sets, vsets, index, clip, c_value, c_entropy, chunk=64):
    """-> (six float64 arrays bounding |host_ppo_grad - the float64 gradient| per element, the smallest margin of a pre-activation
    over its forward bound, the smallest margin of a ratio from 1 +- clip over its bound): everything in float64 from absolute
    values; see the docstring of tests/test_ppo_host.py::test_the_model_against_torch_float64_autograd_within_the_derived_bound"""
    u = 2.0 ** -24
    obs, act, lpo, adv, ret = (np.asarray(v) for v in data)
    R, A, F = obs.shape
    idx = np.arange(R) if index is None else np.asarray(index, np.int64)
    M = len(idx)
    ok = (idx >= 0) & (idx < R)
    rows = idx[ok]
    pos = np.nonzero(ok)[0]
    w1, b1, w2, b2 = (np.asarray(v, np.float64) for v in W)
    wv, bv = np.asarray(V[0], np.float64).reshape(len(w1), -1), np.asarray(V[1], np.float64).reshape(-1)
    n, C = w2.shape[0], w2.shape[1]
    setof = lambda t, a: None if a >= len(t) or t[a] is None or t[a] == 0xFF else int(t[a])
    n_p, n_v = sum(setof(sets, a) is not None for a in range(A)), sum(setof(vsets, a) is not None for a in range(A))
    inv_p, inv_v = (1.0 / (M * n_p) if n_p else 0.0), (1.0 / (M * n_v) if n_v else 0.0)
    shapes = [(n, 64, F), (n, 64), (n, C, 64), (n, C), (n, 64), (n, 1)]
    S, E = [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]        # sums of magnitudes; propagated input errors
    longest = np.zeros((n, (M + chunk - 1) // chunk), np.int64)                 # passes per (set, chunk)
    margin_pre, margin_ratio = np.inf, np.inf

    def hidden(x, k):
        pre = x @ w1[k].T + b1[k]
        e1 = gamma(F + 1) * (np.abs(x) @ np.abs(w1[k]).T + np.abs(b1[k]))      # F fmaf roundings behind the bias; ReLU is 1-Lipschitz
        return pre, e1, np.maximum(pre, 0)

    def head(h, e1, w, b):                                                     # 64 products, six levels, the bias: well inside gamma_70
        return h @ w.T + b, gamma(70) * ((np.abs(h) + e1) @ np.abs(w).T + np.abs(b)) + e1 @ np.abs(w).T

    def one_pass(k, where, x, pre, e1, h, G, dG, gv, dgv):
        """the passes of positions `where` into set k: G / dG [m][C] and gv / dgv [m], zeros where the part is absent"""
        dh = G @ w2[k] + gv[:, None] * wv[k]
        edh = gamma(C + 1) * ((np.abs(G) + dG) @ np.abs(w2[k]) + (np.abs(gv) + dgv)[:, None] * np.abs(wv[k])) + dG @ np.abs(w2[k]) + dgv[:, None] * np.abs(wv[k])
        live = pre > 0
        da, eda = np.abs(dh) * live, edh * live
        ha = np.abs(h) + e1
        Ga, gva = np.abs(G) + dG, np.abs(gv) + dgv
        S[2][k] += Ga.T @ ha;               E[2][k] += dG.T @ ha + np.abs(G).T @ e1
        S[3][k] += Ga.sum(0);               E[3][k] += dG.sum(0)
        S[4][k] += gva @ ha;                E[4][k] += dgv @ ha + np.abs(gv) @ e1
        S[5][k] += gva.sum();               E[5][k] += dgv.sum()
        S[1][k] += (da + eda).sum(0);       E[1][k] += eda.sum(0)
        S[0][k] += (da + eda).T @ np.abs(x); E[0][k] += eda.T @ np.abs(x)
        np.add.at(longest[k], where // chunk, 1)

    for a in range(A):
        s, vs = setof(sets, a), setof(vsets, a)
        x = obs[rows, a].astype(np.float64)
        m = len(x)
        G, dG, has_p = np.zeros((m, C)), np.zeros((m, C)), np.zeros(m, bool)
        gv, dgv = np.zeros(m), np.zeros(m)
        if s is not None:
            pre, e1, h = hidden(x, s)
            margin_pre = min(margin_pre, float((np.abs(pre) - e1).min()))
            logits, el = head(h, e1, w2[s], b2[s])
            eq = el + el.max(axis=1, keepdims=True) + Q64                      # log-sum-exp is 1-Lipschitz in the largest logit error
            z = logits - logits.max(axis=1, keepdims=True)
            q = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
            p = np.exp(q)
            dp = p * (np.expm1(eq) + 2 * U64)                                  # (... and cz_exp's own 2.2e-16)
            H = -(p * q).sum(axis=1)
            dH = (dp * np.abs(q) + p * eq + dp * eq).sum(axis=1) + (C + 1) * U64 * (p * np.abs(q)).sum(axis=1)     # C products, C - 1 adds, the sign
            ac = act[rows, a].astype(np.int64)
            has_p = (ac >= 0) & (ac < C)
            ai = np.where(has_p, ac, 0)[:, None]
            qa = np.take_along_axis(q, ai, 1)[:, 0]
            ratio = np.exp(qa - lpo[rows, a].astype(np.float64))
            dr = ratio * (np.expm1(np.take_along_axis(eq, ai, 1)[:, 0] + u * np.abs(qa) + U64 * 64) + 2 * U64)   # q_act rounded to float32 once, d once, cz_exp
            Adv = adv[rows, a].astype(np.float64)
            edge = np.minimum(np.abs(ratio - (1.0 + clip)), np.abs(ratio - (1.0 - clip))) - dr
            if (has_p & (Adv != 0)).any():
                margin_ratio = min(margin_ratio, float(edge[has_p & (Adv != 0)].min()))
            clipped = ((Adv > 0) & (ratio > 1.0 + clip)) | ((Adv < 0) & (ratio < 1.0 - clip))
            glp, dglp = np.where(clipped, 0.0, -(Adv * ratio)), np.where(clipped, 0.0, np.abs(Adv) * dr)
            t = (np.arange(C)[None, :] == ac[:, None]) - p
            qH, dqH = q + H[:, None], eq + dH[:, None]
            G = inv_p * (glp[:, None] * t + c_entropy * (p * qH))
            dG = inv_p * (dglp[:, None] * np.abs(t) + (np.abs(glp) + dglp)[:, None] * dp + c_entropy * (dp * np.abs(qH) + (p + dp) * dqH))
            mag = inv_p * (np.abs(glp)[:, None] * np.abs(t) + c_entropy * (p * np.abs(qH)))
            dG = dG + u * (np.abs(G) + dG) + 8 * U64 * mag                     # the one rounding to float32; the eight float64 operations of g_c
            G, dG = G * has_p[:, None], dG * has_p[:, None]
        if vs is not None:
            if vs != s:
                pre_v, e1_v, h_v = hidden(x, vs)
                margin_pre = min(margin_pre, float((np.abs(pre_v) - e1_v).min()))
            else:
                pre_v, e1_v, h_v = pre, e1, h
            v, ev = head(h_v, e1_v, wv[vs][None, :], bv[vs:vs + 1])
            gv = inv_v * c_value * (v[:, 0] - ret[rows, a].astype(np.float64))
            dgv = inv_v * c_value * ev[:, 0]
            dgv = dgv + u * (np.abs(gv) + dgv) + 3 * U64 * inv_v * c_value * (np.abs(v[:, 0]) + np.abs(ret[rows, a].astype(np.float64)))   # float32 once; -, *, *
        zero_c, zero = np.zeros((m, C)), np.zeros(m)
        if s is not None and vs == s:
            one_pass(s, pos, x, pre, e1, h, G, dG, gv, dgv)                    # (a position without a policy part: gv alone, G = 0)
        else:
            if s is not None and has_p.any():
                one_pass(s, pos[has_p], x[has_p], pre[has_p], e1[has_p], h[has_p], G[has_p], dG[has_p], zero[has_p], zero[has_p])
            if vs is not None:
                one_pass(vs, pos, x, pre_v, e1_v, h_v, zero_c, zero_c, gv, dgv)
    bounds = []
    for Sk, Ek in zip(S, E):
        b = np.zeros_like(Sk)
        for k in range(n):                                                      # the longest chain of a chunk, then one add per chunk
            b[k] = gamma(int(longest[k].max()) + longest.shape[1]) * Sk[k] + Ek[k]
            # the float64 reference itself: an element is a sum of at most longest.sum() terms in any order, each through at most
            # F + 64 + 4 C + 32 float64 operations of both layers, the softmax and the loss: gamma64 of that count times the magnitudes
            k64 = (int(longest[k].sum()) + F + 64 + 4 * C + 32) * U64
            b[k] += k64 / (1.0 - k64) * Sk[k]
        bounds.append(b)
    return bounds, margin_pre, margin_ratio
