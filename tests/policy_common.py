"""Helpers shared by the tests of the MLP policy (cz_load_policy_device, cz_policy_device, cz_rollout_policy): weight sets, the levels
with movable static objects, the sentinel-filled buffers of a policy rollout and the two halves of every rollout comparison.
(pytest rewrites asserts in test modules only: every assert here carries its own message.)"""
import json
import os

import numpy as np

from cooking_zoo_amd import policy, soa
from vec_common import SENTINEL, strip, want32

ROLLOUT_POLICY = 9                                              # cz::StepMode in cz_kernels.h
NAN64 = 0xFFF8A5A5A5A5A5A5                                      # the rewards' sentinel: a NaN no reward equals
ACT_SENT = -7777                                                # the actions' sentinel: no action code
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cooking_zoo_amd", "utils")
# level -> (meta file, instance, {(static class, k-th entry of it): (x candidates, y candidates)}, the fourth agent's spawn area):
# grids whose quotients are inexact in float32, pools whose layouts differ in their descriptor rows, four agents on every instance
MOVABLE = {
    "crowded_6x5": ("crowded_6x5", 0, {("Cutboard", 0): ([0], [2, 3]), ("Blender", 0): ([5], [1, 2])}, None),
    "limit_8x31": ("limits", 1, {("Cutboard", 0): ([0], [2, 5, 9]), ("Blender", 0): ([3, 5], [30])},
                   {"MAX_COUNT": 1, "X_POSITION": [1, 2, 3, 4, 5, 6], "Y_POSITION": list(range(1, 30))}),
    "huge_20x20": ("huge_20x20", 2, {("Cutboard", 0): ([3, 7, 11], [4]), ("Blender", 0): ([0], [8, 12])},
                   {"MAX_COUNT": 1, "X_POSITION": list(range(2, 18)), "Y_POSITION": [6, 7, 11, 12]}),
}


def write_movable_levels(d):
    """-> {level: (level file, meta file, instance)}: copies of the shipped files under directory `d` in which two static objects draw
    their cell from a short list, with a fourth agent entry and "Agent": 4 in the meta file"""
    out = {}
    for level, (meta, inst, moves, fourth) in MOVABLE.items():
        lv = json.load(open(os.path.join(PKG, "level", level + ".json")))
        seen = {}
        for entry in lv["STATIC_OBJECTS"]:
            (name, spec), = entry.items()
            k = seen.get(name, 0)
            seen[name] = k + 1
            if (name, k) in moves:
                spec["X_POSITION"], spec["Y_POSITION"] = moves[(name, k)]
        if fourth:
            lv["AGENTS"].append(fourth)
        mt = json.load(open(os.path.join(PKG, "meta_files", meta + ".json")))
        for entry in mt:
            if "Agent" in entry:
                entry["Agent"] = 4
        lp, mp = str(d / (level + "_movable.json")), str(d / (meta + "_4agents.json"))
        json.dump(lv, open(lp, "w"))
        json.dump(mt, open(mp, "w"))
        out[level] = (lp, mp, inst)
    return out


def weights(F, C, n_sets=2, seed=0, scale=0.3, scale2=None):
    """n_sets weight sets N(0, scale^2) in torch's layouts, stacked: (w1 [n][64][F], b1 [n][64], w2 [n][C][64], b2 [n][C]) float32 -
    ordinary magnitudes, nothing near NaN, infinity or the subnormals.  `scale2`: the output layer's own scale - a small one keeps
    the logits within a few units of each other, so that sampling has more than one action to choose from"""
    rng = np.random.default_rng(1000 + seed)
    shapes = ((n_sets, policy.HIDDEN, F), (n_sets, policy.HIDDEN), (n_sets, C, policy.HIDDEN), (n_sets, C))
    scales = (scale, scale, scale if scale2 is None else scale2, scale if scale2 is None else scale2)
    return tuple((rng.standard_normal(s) * k).astype(np.float32) for s, k in zip(shapes, scales))


def dense_rows(n, A, F, seed):
    """float32 [n][A][F] standard normal x 0.5 with every entry of magnitude 2^-20 or more and no two entries of a row equal: rows
    in which every feature - every column of W1, the last quad's included - reaches the logits, and in which two columns that
    change places show.  (Observation rows are sparse: about half their features are 0.0 in every row the oracle produces.)"""
    for k in range(16):                                         # (a collision or a tiny draw is rare: the whole array is drawn again)
        x = (np.random.default_rng(2000 + seed + 7919 * k).standard_normal((n, A, F)) * 0.5).astype(np.float32)
        s = np.sort(x, axis=-1)
        if (np.abs(x) >= 2.0 ** -20).all() and (s[..., 1:] != s[..., :-1]).all() and float(np.abs(x).max()) < 8.0:
            return x
    raise AssertionError("dense_rows: no draw without a tiny entry or two equal entries in a row")


def exact_logit_weights(F, L, dead=False):
    """one weight set whose logits are the float32 values `L` [C] in bits for ANY finite row: W1 = 0, b1 = (1, 0, ..., 0), W2[c][0] =
    L_c, the rest 0, b2 = 0 - hidden unit 0 is 1.0, the others 0.0, and the butterfly adds zeros to L_c.  `dead`: b1 = -1 everywhere,
    so every hidden unit is 0.0, with an ordinary W2 and b2 = L: the logits are b2's bits (L must hold no 0.0, whose sign a sum of
    zeros would decide) -> (w1 [64][F], b1 [64], w2 [C][64], b2 [C])"""
    L = np.asarray(L, np.float32)
    Cn = len(L)
    w1, b1 = np.zeros((policy.HIDDEN, F), np.float32), np.zeros(policy.HIDDEN, np.float32)
    w2, b2 = np.zeros((Cn, policy.HIDDEN), np.float32), np.zeros(Cn, np.float32)
    if dead:
        assert (L != 0).all(), "exact_logit_weights: a dead hidden layer cannot give a logit of 0.0 a sign"
        b1[:] = -1.0
        w2[:] = (np.random.default_rng(Cn).standard_normal(w2.shape) * 0.3).astype(np.float32)
        b2[:] = L
    else:
        b1[0] = 1.0
        w2[:, 0] = L
    return w1, b1, w2, b2


def logit_cases(Cn):
    """name -> (L float32 [Cn], dead): the logits the sampling rule is shown on the device - all equal; three tied at the maximum
    (the last action among them); one 70 and one 1000 below the maximum, both beyond the clamp at -64; one overwhelming (50 above
    the rest: the sum of the exponentials is 1.0 exactly, so its log-probability is 0.0); every hidden unit dead, logits from b2"""
    low = np.linspace(-1.5, -0.25, Cn).astype(np.float32)
    tie = low.copy()
    tie[[1, 3, Cn - 1]] = 2.0
    clamp = (low * np.float32(0.25)).astype(np.float32)
    clamp[2], clamp[0], clamp[Cn - 2] = 1.0, -69.0, -999.0
    one = low.copy()
    one[Cn - 2] = 50.0
    dead = np.linspace(0.5, -0.75, Cn).astype(np.float32)
    assert (dead != 0).all(), "logit_cases: b2 holds a zero"
    return {"flat": (np.full(Cn, 0.25, np.float32), False), "tie3": (tie, False), "clamp": (clamp, False), "one": (one, False),
            "dead": (dead, True)}


def stack_sets(sets):
    """weight sets (w1, b1, w2, b2) -> the stacked form `load_policy` and `expected_policy` take"""
    return tuple(np.stack(v) for v in zip(*sets))


def matrix_product_logits(x, w1, b1, w2, b2):
    """the plain float32 matrix-product form of one set's logits: another summation order, other bits"""
    return (np.maximum(x @ w1.T + b1, 0) @ w2.T + b2).astype(np.float32)


def sets_for(A):
    """agent 0 on set 1, the others on set 0, the last agent without a policy where A >= 2"""
    s = [1] + [0] * (A - 1)
    if A >= 2:
        s[-1] = None
    return tuple(s)


class PolicyTraj:
    """the buffers of one cz_rollout_policy launch of T steps, each with a guard row behind row T - 1 (None for those in `skip`):
    rows uint32 [T + 1][n][A][F], act int32 [T + 1][n][A], logits uint32 [T + 1][n][A][C], rew uint64, term / trunc uint8 [T + 1][n][A]"""

    def __init__(self, env, T, skip=(), sharded=False):
        n, A, F, Cn = env.num_envs, env.num_agents, env.F, env.num_actions
        self.T = T
        self.fillers = dict(rows=((A, F), np.uint32, SENTINEL), act=((A,), np.int32, ACT_SENT), logits=((A, Cn), np.uint32, SENTINEL),
                            rew=((A,), np.uint64, NAN64), term=((A,), np.uint8, 0xA5), trunc=((A,), np.uint8, 0xA5))
        alloc = (lambda per, t: env.alloc(per, t, leading=(T + 1,))) if sharded else (lambda per, t: env.alloc((T + 1, n) + per, t))
        self.buf = {k: None if k in skip else alloc(per, t) for k, (per, t, _) in self.fillers.items()}
        self.shape = {k: (T + 1, n) + per for k, (per, _, _) in self.fillers.items()}

    def fill(self):
        for k, b in self.buf.items():
            if b is not None:
                b.from_host(np.full(self.shape[k], self.fillers[k][2], self.fillers[k][1]))

    def get(self):
        """-> {name: [T][n]... or None}; asserts every guard row"""
        out = {}
        for k, b in self.buf.items():
            if b is None:
                out[k] = None
                continue
            got = b.to_host()
            assert (got[self.T] == self.fillers[k][2]).all(), f"{k}: a store went past the last row"
            out[k] = got[:self.T]
        return out

    def launch(self, env, sets, mode, seed, step0):
        b = self.buf
        env.rollout_policy(self.T, b["rows"], b["act"], b["logits"], b["rew"], b["term"], b["trunc"], sets=sets, mode=mode, seed=seed, step0=step0)

    def rollout(self, env, sets, mode, seed, step0=0):
        self.fill()
        self.launch(env, sets, mode, seed, step0)
        env.sync()
        return self.get()


def stream_actions(orc, T, seed, step0):
    """the on-device action stream of (seed, step0) for T steps, [T][n][A] (the oracle's)"""
    err, _, _, _, _, acts = orc.oracle.rollout(orc.records.copy(), T, seed, step0, want_obs=False, want_actions=True)
    assert err == 0, "the oracle's rollout failed"
    return np.ascontiguousarray(acts, dtype=np.int32)


def replay(ctx, orc, got, acts):
    """half 1: the oracle replays `acts` [T][n][A]; rows, rewards and flags of `got` must be exact -> the records after every step"""
    recs = []
    for t in range(len(acts)):
        obs, rew, term, trunc = orc.step(acts[t])
        bad = np.argwhere(got["rows"][t] != want32(obs))
        assert not len(bad), f"{ctx} step {t}: float32 rows differ at (env, agent, feature) {bad[:6].tolist()}"
        if got.get("rew") is not None:
            assert np.array_equal(got["rew"][t], rew.view(np.uint64)), f"{ctx} step {t}: rewards"
        if got.get("term") is not None:
            assert np.array_equal(got["term"][t], term), f"{ctx} step {t}: terminations"
        if got.get("trunc") is not None:
            assert np.array_equal(got["trunc"][t], trunc), f"{ctx} step {t}: truncations"
        recs.append(orc.records.copy())
    return recs


def logits_per_set(rows, W):
    """rows float32 [...][F], W stacked sets -> [host_logits of every row under set s, float32 [...][C], for each s]: what many
    launches over the same rows share"""
    x = np.ascontiguousarray(rows).view(np.float32)
    return [policy.host_logits(x, W[0][s], W[1][s], W[2][s], W[3][s]) for s in range(len(W[0]))]


def swap_columns(w1, f):
    """w1 [64][F] with columns f and f + 1 exchanged"""
    out = w1.copy()
    out[:, [f, f + 1]] = w1[:, [f + 1, f]]
    return out


def dense_conditions(ctx, rows, W, per_set):
    """what makes a comparison on the rows able to fail, from the model alone, for every set of W: the expected logits of EVERY row
    change when the last two columns of W1 change places, when the first two do, and when every column moves one place; the sets'
    logits differ pairwise in every row; and at least 25 % of the logits differ in bits from the matrix-product form -> that share"""
    x = np.ascontiguousarray(rows).view(np.float32)
    F = x.shape[-1]
    x = x.reshape(-1, F)
    base = [np.ascontiguousarray(p).reshape(len(x), -1).view(np.uint32) for p in per_set]
    differ = total = 0
    for s, want in enumerate(base):
        w1, rest = W[0][s], (W[1][s], W[2][s], W[3][s])
        for what, other in (("the last two columns of W1 exchanged", swap_columns(w1, F - 2)), ("the first two columns of W1 exchanged", swap_columns(w1, 0)),
                            ("every column of W1 moved one place", np.roll(w1, 1, axis=1))):
            got = policy.host_logits(x, other, *rest).view(np.uint32)
            same = int((got == want).all(axis=-1).sum())
            assert same == 0, f"{ctx}: set {s} with {what} gives the same logits in {same} of {len(x)} rows: the case shows nothing"
        for t in range(s):
            same = int((base[t] == want).all(axis=-1).sum())
            assert same == 0, f"{ctx}: sets {t} and {s} give the same logits in {same} of {len(x)} rows: the case shows nothing"
        differ += int((matrix_product_logits(x, w1, *rest).view(np.uint32) != want).sum())
        total += want.size
    share = differ / total
    assert share >= 0.25, f"{ctx}: only {share:.1%} of the logits differ from the matrix-product form: the case shows nothing"
    return share


def expected_policy(rows_before, W, sets, mode, seed, step0, stream, env_id_base=0, per_set=None):
    """half 2: rows_before uint32 / float32 [T][n][A][F] - the row before every step - -> (actions int32 [T][n][A], logits float32
    [T][n][A][C] with NaN where no policy wrote, mask [A] of the policy agents); agents without a set take `stream`.
    `per_set`: logits_per_set(rows_before, W), computed once for several calls on the same rows"""
    x = np.ascontiguousarray(rows_before).view(np.float32)
    T, n, A, _ = x.shape
    Cn = W[2].shape[1]
    acts = np.array(stream, dtype=np.int32, copy=True)
    logits = np.full((T, n, A, Cn), np.nan, np.float32)
    mask = np.zeros(A, bool)
    env_ids = (np.arange(n, dtype=np.uint64) + np.uint64(env_id_base))[None, :]
    steps = (np.arange(T, dtype=np.uint64) + np.uint64(step0))[:, None]
    for a in range(A):
        s = sets[a] if a < len(sets) else None
        if s is None or s == policy.NONE:
            continue
        mask[a] = True
        logits[:, :, a] = policy.host_logits(x[:, :, a], W[0][s], W[1][s], W[2][s], W[3][s]) if per_set is None else per_set[s][:, :, a]
        acts[:, :, a] = policy.host_actions(logits[:, :, a], mode, seed, env_ids, steps, a)
    return acts, logits, mask


def check_policy(ctx, got, want_acts, want_logits, mask):
    """the device's actions and logits against half 2's; entries of agents without a policy: the stream's action, the logits' sentinel"""
    if got.get("act") is not None:
        bad = np.argwhere(got["act"] != want_acts)
        assert not len(bad), f"{ctx}: actions differ at (step, env, agent) {bad[:6].tolist()}: {got['act'][tuple(bad[0])]} for {want_acts[tuple(bad[0])]}"
    if got.get("logits") is not None:
        lg = got["logits"]
        bad = np.argwhere(lg[:, :, mask] != want_logits[:, :, mask].view(np.uint32))
        assert not len(bad), f"{ctx}: logits differ in bits at (step, env, policy agent, action) {bad[:6].tolist()}"
        assert (lg[:, :, ~mask] == SENTINEL).all(), f"{ctx}: logits of an agent without a policy were written"


def verify_rollout(ctx, orc, obs0, got, W, sets, mode, seed, step0=0):
    """both halves of a rollout comparison from the oracle's state in front of the launch (`obs0`: its float64 observation there)
    -> the records after every step"""
    stream = stream_actions(orc, len(got["rows"]), seed, step0)
    assert got["act"] is not None, "verify_rollout needs the actions output"
    recs = replay(ctx, orc, got, got["act"])
    before = np.concatenate([want32(obs0)[None], got["rows"][:-1]])
    want_acts, want_logits, mask = expected_policy(before, W, sets, mode, seed, step0, stream, orc.env_id_base)
    check_policy(ctx, got, want_acts, want_logits, mask)
    return recs


def start(env, orc):
    """both reset -> the oracle's first observation (float64)"""
    env.reset(return_obs=False)
    obs0 = orc.reset().copy()
    assert np.array_equal(strip(env.get_state()), orc.records), "records after reset"
    return obs0


def current_obs(orc):
    """the oracle's observation of its current records, float64 [n][A][F]"""
    return np.stack([orc.oracle.observe(rec) for rec in orc.records])
