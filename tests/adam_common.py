"""Helpers shared by the tests of cz_adam_step_device (definition: cooking_zoo_amd/adam.py): synthetic parameter, gradient and moment
tensors, the comparison as bits, a float64 Adam with beta**t bias correction and the bound of the model's distance from it, and the
guarded device buffers of one run of calls.
(pytest rewrites asserts in test modules only: every assert here carries its own message.)"""
import numpy as np

from cooking_zoo_amd import adam, policy
from policy_common import dense_rows, logits_per_set, weights
from ppo_common import GUARD, STAT_SENT, canon
from targets_common import F32_SENT
from value_common import value_weights

NAMES = adam.NAMES
U32, U64 = 2.0 ** -24, 2.0 ** -53                               # the unit roundoffs of float32 and float64


def shapes(F, C, n, value=True):
    s = [(n, policy.HIDDEN, F), (n, policy.HIDDEN), (n, C, policy.HIDDEN), (n, C)]
    return s + ([(n, policy.HIDDEN), (n, 1)] if value else [])


def pad6(group):
    group = list(group)
    return group + [None] * (6 - len(group))


def gradients(F, C, n, seed, value=True, scale=0.05):
    """one gradient group N(0, scale^2), float32: ordinary magnitudes, no zero, nothing near the subnormals"""
    rng = np.random.default_rng(7000 + seed)
    out = []
    for s in shapes(F, C, n, value):
        g = (rng.standard_normal(s) * scale).astype(np.float32)
        g[np.abs(g) < 2.0 ** -30] = np.float32(scale)
        out.append(g)
    return pad6(out)


def tensors(F, C, n, seed, value=True):
    """-> (P, M, V): parameters as the policy tests draw them, first moments N(0, 0.02^2), second moments positive around 1e-3 - a run
    in mid-course, so that the first call already reads every array"""
    rng = np.random.default_rng(6000 + seed)
    P = list(weights(F, C, n, seed, scale2=0.3)) + (list(value_weights(n, seed)) if value else [])
    P = [np.ascontiguousarray(p, np.float32).reshape(s) for p, s in zip(P, shapes(F, C, n, value))]
    M = [(rng.standard_normal(p.shape) * 0.02).astype(np.float32) for p in P]
    V = [(rng.uniform(0.2, 2.0, p.shape) * 1e-3).astype(np.float32) for p in P]
    return pad6(P), pad6(M), pad6(V)


def mid_state(t=3, beta1=0.9, beta2=0.999):
    s = adam.fresh_state()
    s[0], s[1], s[2] = t, beta1 ** t, beta2 ** t
    return s


def same(ctx, got, want, state=True):
    """(P, M, V, state) twice, as bits with zeros of either sign equal"""
    for group, a, b in zip("PMV", got[:3], want[:3]):
        for name, u, v in zip(NAMES, a, b):
            assert (u is None) == (v is None), f"{ctx}: {group}.{name} is present on one side only"
            if u is None:
                continue
            u, v = canon(np.asarray(u, np.float32).reshape(np.shape(v))), canon(v)
            bad = np.argwhere(u != v)
            assert not len(bad), (f"{ctx}: {group}.{name} differs in bits in {len(bad)} of {u.size} elements, first at {bad[0].tolist()}: "
                                  f"{u[tuple(bad[0])]:#x} for {v[tuple(bad[0])]:#x}")
    if state:
        a, b = np.asarray(got[3], np.float64), np.asarray(want[3], np.float64)
        assert np.array_equal(canon(a), canon(b)), f"{ctx}: state {a.tolist()} for {b.tolist()}"


# ---------------------------------------------------------------------------------------------------------------------------
# float64 Adam as the textbooks have it, and how far the definition may lie from it
# ---------------------------------------------------------------------------------------------------------------------------

def reference_steps(P, grads, set_mask, lr, beta1, beta2, eps, weight_decay, max_norm, mutant=None):
    """T steps from zero moments in float64 throughout: float64 moments, bias correction 1 - beta**t, clip_grad_norm_'s coefficient from
    numpy's own sum of squares.  With mutant=None also the bound of |host_adam_step's parameters - these| per element, propagated
    step by step from the roundings adam.py makes (the derivation: tests/test_adam_host.py).  mutant "eps_inside": sqrt(vh + eps);
    "no_bias_correction": mh = m, vh = v.  -> (parameters float64, bounds or None)"""
    n = P[0].shape[0]
    sets = [k for k in range(n) if (set_mask >> k) & 1]
    live = [i for i in range(6) if P[i] is not None]
    p = {i: np.asarray(P[i], np.float64).copy() for i in live}
    m = {i: np.zeros_like(p[i]) for i in live}
    v = {i: np.zeros_like(p[i]) for i in live}
    ep, em, ev = ({i: np.zeros_like(p[i]) for i in live} for _ in range(3))
    for t, G in enumerate(grads, start=1):
        g = {i: np.asarray(G[i], np.float64) for i in live}
        count = sum(g[i][k].size for i in live for k in sets)
        norm = np.sqrt(sum(float((g[i][k] ** 2).sum()) for i in live for k in sets))
        coef = 1.0 if max_norm == 0 else min(1.0, max_norm / (norm + 1e-6))
        # the sum of `count` exact squares through float64 adds in any order is within gamma64(count) of the true sum - the model's
        # chain and numpy's pairwise sum alike -, sqrt halves a relative error and adds one rounding, `+ 1e-6` and `/` one each; min(1, .)
        # is 1-Lipschitz: two values of the coefficient differ by at most rc relative
        rc = 2.0 * (count + 4) * U64
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        # the model's bc is 1 - (a product of t factors, t roundings), the reference's 1 - pow: absolute (t + 3) U64 at most
        rb1, rb2 = (t + 3) * U64 / bc1, (t + 3) * U64 / bc2
        for i in live:
            for k in sets:
                gc = coef * g[i][k]
                eg = np.abs(gc) * (rc + U64)
                terms = beta1 * np.abs(m[i][k]) + (1.0 - beta1) * np.abs(gc)  # (the two products may cancel: roundings go by their sizes)
                m[i][k] = beta1 * m[i][k] + (1.0 - beta1) * gc
                v[i][k] = beta2 * v[i][k] + (1.0 - beta2) * gc * gc
                # moments: the carried error, the gradient's, three / four float64 roundings on each side, then the store as float32
                em[i][k] = beta1 * em[i][k] + (1.0 - beta1) * eg + 8 * U64 * (terms + em[i][k])
                em[i][k] += U32 * (np.abs(m[i][k]) + em[i][k])
                ev[i][k] = beta2 * ev[i][k] + (1.0 - beta2) * (2 * np.abs(gc) * eg + eg * eg) + 10 * U64 * (v[i][k] + ev[i][k])
                ev[i][k] += U32 * (v[i][k] + ev[i][k])
                if mutant == "no_bias_correction":
                    mh, vh = m[i][k], v[i][k]
                else:
                    mh, vh = m[i][k] / bc1, v[i][k] / bc2
                emh = em[i][k] / bc1 + (np.abs(mh) + em[i][k] / bc1) * (rb1 + 2 * U64)
                evh = ev[i][k] / bc2 + (vh + ev[i][k] / bc2) * (rb2 + 2 * U64)
                if mutant == "eps_inside":
                    den = np.sqrt(vh + eps)
                else:
                    den = np.sqrt(vh) + eps
                # |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= |a - b| / sqrt b, and <= sqrt |a - b| always
                root = np.sqrt(vh)
                es = np.minimum(np.sqrt(evh), evh / np.maximum(root, 1e-300)) + 2 * U64 * root
                eden = es + 2 * U64 * den
                assert (den - eden > 0).all(), "the bound's denominator reaches 0: eps is too small for this derivation"
                q = mh / den
                eq = emh / (den - eden) + np.abs(mh) * eden / (den * (den - eden)) + 2 * U64 * np.abs(q)
                if weight_decay != 0:
                    lw = lr * weight_decay
                    p[i][k] = p[i][k] - lw * p[i][k]
                    ep[i][k] = ep[i][k] * (1.0 + lw) + 6 * U64 * np.abs(p[i][k])
                p[i][k] = p[i][k] - lr * q
                ep[i][k] = ep[i][k] + lr * eq + 4 * U64 * (lr * np.abs(q) + np.abs(p[i][k]))
                ep[i][k] += U32 * (np.abs(p[i][k]) + ep[i][k])                 # the parameter's store as float32
    return [p.get(i) for i in range(6)], (None if mutant else [ep.get(i) for i in range(6)])


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------

class AdamCall:
    """the device side of a run of cz_adam_step_device calls: P, M, V and the state with GUARD sentinel elements before and behind
    each, the gradients plain"""

    def __init__(self, env, P, G, M, V, state):
        self.env = env
        self.live = [i for i in range(6) if P[i] is not None]
        self.shapes = {i: P[i].shape for i in self.live}
        mk = lambda: {i: env.alloc((P[i].size + 2 * GUARD,), np.uint32) for i in self.live}
        self.P, self.M, self.V = mk(), mk(), mk()
        self.G = {i: env.alloc(P[i].shape, np.float32) for i in self.live}
        self.state = env.alloc((8 + 2 * GUARD,), np.uint64)
        self.lr = env.alloc((1,), np.float64)
        for dev, host in ((self.P, P), (self.M, M), (self.V, V)):
            for i in self.live:
                self.put(dev[i], host[i])
        self.set_grads(G)
        self.set_state(state)

    @staticmethod
    def put(buf, arr):
        h = np.full(buf.shape, F32_SENT, np.uint32)
        h[GUARD:-GUARD] = np.ascontiguousarray(arr, np.float32).reshape(-1).view(np.uint32)
        buf.from_host(h)

    def set_grads(self, G):
        for i in self.live:
            self.G[i].from_host(np.ascontiguousarray(G[i], np.float32))

    def set_state(self, state):
        h = np.full(self.state.shape, STAT_SENT, np.uint64)
        h[GUARD:-GUARD] = np.asarray(state, np.float64).view(np.uint64)
        self.state.from_host(h)

    def set_lr(self, lr):
        self.lr.from_host(np.array([lr], np.float64))

    def groups(self):
        grp = lambda dev, off: [dev[i].ptr + off if i in dev else None for i in range(6)]
        return grp(self.P, 4 * GUARD), grp(self.G, 0), grp(self.M, 4 * GUARD), grp(self.V, 4 * GUARD)

    def launch(self, **kw):
        self.env.adam_step_device(*self.groups(), self.state.ptr + 8 * GUARD, **kw)

    def get(self, ctx):
        """-> (P, M, V as float32 arrays in their shapes, None where absent; state float64 [8]); asserts the guards"""
        out = []
        for name, dev in (("P", self.P), ("M", self.M), ("V", self.V)):
            grp = [None] * 6
            for i in self.live:
                h = dev[i].to_host()
                assert (h[:GUARD] == F32_SENT).all() and (h[-GUARD:] == F32_SENT).all(), f"{ctx}: a store outside {name}.{NAMES[i]}"
                grp[i] = h[GUARD:-GUARD].view(np.float32).reshape(self.shapes[i])
            out.append(grp)
        h = self.state.to_host()
        assert (h[:GUARD] == STAT_SENT).all() and (h[-GUARD:] == STAT_SENT).all(), f"{ctx}: a store outside the state"
        return out[0], out[1], out[2], h[GUARD:-GUARD].view(np.float64).copy()

    def free(self):
        for dev in (self.P, self.M, self.V, self.G):
            for b in dev.values():
                b.free()
        self.state.free()
        self.lr.free()


class View:
    """a float32 array inside a device buffer, in the shape load_policy / load_value ask for"""
    dtype = np.dtype(np.float32)

    def __init__(self, ptr, shape):
        self.ptr, self.shape = ptr, tuple(shape)


class TableProbe:
    """what the weight table holds, seen through policy_device and value_device on a few dense rows: the logits and values of every
    loaded set, and the same from the numpy model under given parameters"""

    def __init__(self, env, seed, rows=5):
        self.env, self.R, self.A = env, rows, env.num_agents
        self.x = dense_rows(rows, self.A, env.F, seed)
        self.d_x = env.alloc(self.x.shape, np.float32)
        self.d_x.from_host(self.x)
        self.d_lg = env.alloc((rows, self.A, env.num_actions), np.float32)
        self.d_v = env.alloc((rows, self.A), np.float32)

    def read(self, n_sets, value=True):
        """-> (logits [n_sets][R][A][C], values [n_sets][R][A] or None) as the device computes them from its table now"""
        logits, values = [], []
        for s in range(n_sets):
            self.env.policy_device(self.d_x, None, self.d_lg, sets=(s,) * self.A, env_count=self.R)
            if value:
                self.env.value_device(self.d_x, self.d_v, vsets=(s,) * self.A, rows=self.R)
            self.env.sync()
            logits.append(self.d_lg.to_host())
            values.append(self.d_v.to_host())
        return np.stack(logits), (np.stack(values) if value else None)

    def expect(self, P, value=True):
        """the same under the parameter group P, from policy.host_logits / host_value"""
        n = P[0].shape[0]
        logits = np.stack(logits_per_set(self.x, P[:4]))
        values = np.stack([policy.host_value(self.x, P[0][s], P[1][s], P[4][s], P[5][s]) for s in range(n)]) if value else None
        return logits, values

    def check(self, ctx, P, value=True):
        got, want = self.read(P[0].shape[0], value), self.expect(P, value)
        assert np.array_equal(canon(got[0]), canon(want[0])), f"{ctx}: the table's logits are not the model's under these parameters"
        assert not value or np.array_equal(canon(got[1]), canon(want[1])), f"{ctx}: the table's values are not the model's under these parameters"
        return got

    def free(self):
        for b in (self.d_x, self.d_lg, self.d_v):
            b.free()
