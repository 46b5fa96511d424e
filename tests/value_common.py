"""Helpers shared by the tests of the value heads (cz_load_value_device, cz_value_device, cz_rollout_policy_value): value-head weights,
the guarded values buffer of a rollout, the model of the values a rollout writes, and the set whose logit c is a value.
(pytest rewrites asserts in test modules only: every assert here carries its own message.)"""
import numpy as np

from cooking_zoo_amd import policy
from policy_common import PolicyTraj
from vec_common import SENTINEL

ROLLOUT_POLICY_VALUE = 10                                       # cz::StepMode in cz_kernels.h


def value_weights(n_sets=2, seed=0, scale=0.3):
    """n_sets value heads N(0, scale^2) in torch's layouts, stacked: (wv [n][64], bv [n][1]) float32"""
    rng = np.random.default_rng(3000 + seed)
    return ((rng.standard_normal((n_sets, policy.HIDDEN)) * scale).astype(np.float32), (rng.standard_normal((n_sets, 1)) * scale).astype(np.float32))


def value_as_logit_set(w1, b1, wv, bv, Cn, c):
    """one weight set of Cn actions whose W2 row c is wv and whose b2[c] is bv, the other rows ordinary: its logit c is the value"""
    rng = np.random.default_rng(77 + c)
    w2 = (rng.standard_normal((Cn, policy.HIDDEN)) * 0.3).astype(np.float32)
    b2 = (rng.standard_normal(Cn) * 0.3).astype(np.float32)
    w2[c], b2[c] = np.asarray(wv, np.float32).reshape(-1), np.float32(np.asarray(bv).reshape(-1)[0])
    return np.asarray(w1, np.float32), np.asarray(b1, np.float32), w2, b2


def matrix_product_value(x, w1, b1, wv, bv):
    """the plain float32 matrix-product form of one set's value: another summation order, other bits"""
    return (np.maximum(x @ w1.T + b1, 0) @ np.asarray(wv, np.float32).reshape(-1) + np.asarray(bv, np.float32).reshape(-1)[0]).astype(np.float32)


def expected_values(rows, W, V, vsets):
    """rows uint32 / float32 [...][A][F], W stacked weight sets, V = (wv [n][64], bv [n][1]) -> (values float32 [...][A] with NaN where
    no value head wrote, mask [A] of the agents with one)"""
    x = np.ascontiguousarray(rows).view(np.float32)
    A = x.shape[-2]
    out = np.full(x.shape[:-1], np.nan, np.float32)
    mask = np.zeros(A, bool)
    for a in range(A):
        s = vsets[a] if a < len(vsets) else None
        if s is None or s == policy.NONE:
            continue
        mask[a] = True
        out[..., a] = policy.host_value(x[..., a, :], W[0][s], W[1][s], V[0][s], V[1][s])
    return out, mask


def check_values(ctx, got, want, mask):
    """the device's values uint32 [...][A] against the model's float32; entries of agents without a value set: the sentinel"""
    bad = np.argwhere(got[..., mask] != np.ascontiguousarray(want[..., mask]).view(np.uint32))
    assert not len(bad), f"{ctx}: values differ in bits at (..., value agent) {bad[:6].tolist()}"
    assert (got[..., ~mask] == SENTINEL).all(), f"{ctx}: values of an agent without a value set were written"


class ValueTraj(PolicyTraj):
    """PolicyTraj plus the values uint32 [T + 2][n][A] of cz_rollout_policy_value: rows 0 .. T are the launch's, row T + 1 the guard"""

    def __init__(self, env, T, skip=(), sharded=False):
        super().__init__(env, T, skip, sharded)
        n, A = env.num_envs, env.num_agents
        self.vshape = (T + 2, n, A)
        self.values = env.alloc((A,), np.uint32, leading=(T + 2,)) if sharded else env.alloc(self.vshape, np.uint32)
        self.vsets = None

    def fill(self):
        super().fill()
        self.values.from_host(np.full(self.vshape, SENTINEL, np.uint32))

    def get(self):
        out = super().get()
        v = self.values.to_host()
        assert (v[self.T + 1] == SENTINEL).all(), "values: a store went past row T"
        out["values"] = v[:self.T + 1]
        return out

    def launch(self, env, sets, mode, seed, step0):
        b = self.buf
        env.rollout_policy_value(self.T, b["rows"], self.values, b["act"], b["logits"], b["rew"], b["term"], b["trunc"], sets=sets,
                                 vsets=self.vsets, mode=mode, seed=seed, step0=step0)

    def rollout(self, env, sets, mode, seed, step0=0, vsets=None):
        self.vsets = vsets
        return super().rollout(env, sets, mode, seed, step0)


def split_values(got):
    """a ValueTraj result -> (what PolicyTraj would have returned, the values [T + 1][n][A])"""
    rest = {k: v for k, v in got.items() if k != "values"}
    return rest, got["values"]
