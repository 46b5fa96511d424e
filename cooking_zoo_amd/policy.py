"""The MLP policy the library evaluates on the device (cz_load_policy_device, cz_policy_device, cz_rollout_policy; the critic:
cz_load_value_device, cz_value_device, cz_rollout_policy_value; device code: csrc/cz_policy.h), as an arithmetic definition numpy
reproduces bit for bit.

A weight set is the parameters of `Sequential(Linear(F, 64), ReLU(), Linear(64, C))` in torch's own layout: W1 float32 [64][F],
b1 float32 [64], W2 float32 [C][64], b2 float32 [C]; F is the handle's row length, C its action count, the hidden width is 64 -
one lane of a wavefront per unit.  For one float32 row x[0..F):

  1. acc_j = b1[j]; for f = 0 .. F-1 ascending: acc_j = fmaf(W1[j][f], x[f], acc_j) - one rounding per feature.
  2. h_j = acc_j > 0 ? acc_j : 0.
  3. per action c: p_j = W2[c][j] * h_j (one float32 rounding), six butterfly levels p_j = p_j + p_(j xor 2^k), k = 0..5, each a
     float32 add - the adjacent-pair tree `p = p[..., 0::2] + p[..., 1::2]` applied six times - and logit_c = p + b2[c].
  3b. A weight set may carry a value head, `Linear(64, 1)` in torch's layout: wv float32 [64] (`weight[0]`) and bv float32 [1].
     With h_j of steps 1-2: p_j = wv[j] * h_j (one float32 rounding), the same six butterfly levels, value = p + bv - exactly the
     arithmetic of one logit (`host_value`).  Every policy-or-value call takes `vsets` beside `sets`, agent a's byte: the weight set
     whose W1, b1 and value head give agent a's value, 0xFF = none (that agent's entries are left untouched).  It is independent of
     `sets`: a shared trunk is vsets == sets, a separate critic is another weight set whose action head is never used, and an agent on
     the action stream may have a value.  Where an agent's two bytes are equal the device computes the hidden vector once, where they
     differ it makes a second pass: the bits are the same either way.
  4. GREEDY: the smallest c with the largest logit.
  5. SAMPLE, in float64 with every operation rounded on its own: z_c = logit_c - max, e_c = cz_exp(max(z_c, -64)), running sums
     S_0 = e_0, S_c = S_(c-1) + e_c, thr = u * S_(C-1); the action is the smallest c with S_c > thr, or C-1 if there is none.
     u = spawn.uniform(seed, global env id, step, 0x300 + agent, 0) - the host's cz_spawn_uniform(seed, g, 0, step, 0x300 + a, 0).
     Agent keys 0..3 are the spawn draws, 0x100 the layout generator, 0x200 the tasks.

NOT pinned: NaN, infinities and subnormal intermediates - weights and rows that produce them may differ between this model and
the device (and between devices).  Keep weights finite and of ordinary scale."""
import numpy as np

from cooking_zoo_amd import spawn

HIDDEN = 64
MAX_SETS = 4
NONE = 0xFF                      # an agent's byte of `sets`: no policy for this agent
AGENT_KEY = 0x300
GREEDY, SAMPLE = 0, 1
MODES = {"greedy": GREEDY, "sample": SAMPLE, GREEDY: GREEDY, SAMPLE: SAMPLE}

_LOG2E = 1.4426950408889634
_LN2_HI = 6.93147180369123816490e-01
_LN2_LO = 1.90821492927058770002e-10
_EXP_COEFFS = []
_fact = 1
for _i in range(14):
    _fact = _fact * _i if _i else 1
    _EXP_COEFFS.append(1.0 / float(_fact))


def pack_sets(sets, num_agents):
    """(s0, s1, ...) per agent, None / 0xFF = no policy -> the uint32 the C API takes (agent a's set in byte a)"""
    word = 0
    sets = tuple(sets)
    for a in range(4):
        s = sets[a] if a < len(sets) and a < num_agents else NONE
        s = NONE if s is None else int(s)
        if not (0 <= s < MAX_SETS or s == NONE):
            raise ValueError(f"set index {s} of agent {a}: not 0..{MAX_SETS - 1} or 0xFF")
        word |= s << (8 * a)
    return word


def fmaf32(a, b, c):
    """float32 fmaf(a, b, c), exactly: the product is exact in float64, the sum is rounded to odd there (TwoSum residual), and 53 bits
    rounded to odd round to the 24-bit nearest-even result.  (The plain `(a64 * b64 + c64).astype(float32)` rounds twice and is wrong
    near float32 midpoints.)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def cz_exp(z):
    """exp on [-64, 64] in plain float64 arithmetic (within 2.2e-16 relative of np.exp there; the sampler and the log-probabilities
    use [-64, 0], the ratio of ppo.py the whole range)"""
    z = np.asarray(z, np.float64)
    k = np.floor(z * _LOG2E + 0.5)
    r = (z - k * _LN2_HI) - k * _LN2_LO
    p = np.full_like(r, _EXP_COEFFS[13])
    for i in range(12, -1, -1):
        p = p * r + _EXP_COEFFS[i]
    return np.ldexp(p, k.astype(np.int64))


def host_hidden(x, w1, b1):
    """steps 1-2: float32 rows x [..., F] -> the float32 hidden vector [..., 64]"""
    F = x.shape[-1]
    acc = np.broadcast_to(b1, x.shape[:-1] + (HIDDEN,)).copy()
    for f in range(F):
        acc = fmaf32(w1[:, f], x[..., f:f + 1], acc)
    return np.where(acc > 0, acc, np.float32(0))


def host_heads(h, w2, b2):
    """step 3: the hidden vector [..., 64] and output rows w2 [C, 64], b2 [C] -> float32 [..., C]"""
    p = w2 * h[..., None, :]                                   # [..., C, 64], one float32 rounding each
    for _ in range(6):
        p = p[..., 0::2] + p[..., 1::2]
    return (p[..., 0] + b2).astype(np.float32)


def host_logits(x, w1, b1, w2, b2):
    """float32 rows x [..., F] -> float32 logits [..., C] of one weight set, bit for bit the device's"""
    x = np.asarray(x, np.float32)
    w1, b1, w2, b2 = (np.asarray(v, np.float32) for v in (w1, b1, w2, b2))
    F = x.shape[-1]
    if w1.shape != (HIDDEN, F) or b1.shape != (HIDDEN,) or w2.ndim != 2 or w2.shape[1] != HIDDEN or b2.shape != (w2.shape[0],):
        raise ValueError(f"weight shapes {w1.shape} {b1.shape} {w2.shape} {b2.shape} for rows of {F} features")
    return host_heads(host_hidden(x, w1, b1), w2, b2)


def host_value(x, w1, b1, wv, bv):
    """float32 rows x [..., F] -> float32 values [...] of one weight set's value head (step 3b), bit for bit the device's: wv [64]
    (or torch's `weight` [1, 64]) and bv [1] (or a scalar)"""
    x = np.asarray(x, np.float32)
    w1, b1 = np.asarray(w1, np.float32), np.asarray(b1, np.float32)
    wv, bv = np.asarray(wv, np.float32).reshape(-1), np.asarray(bv, np.float32).reshape(-1)
    F = x.shape[-1]
    if w1.shape != (HIDDEN, F) or b1.shape != (HIDDEN,) or wv.shape != (HIDDEN,) or bv.shape != (1,):
        raise ValueError(f"weight shapes {w1.shape} {b1.shape} {wv.shape} {bv.shape} for rows of {F} features")
    return host_heads(host_hidden(x, w1, b1), wv[None, :], bv)[..., 0]


def sample_from(logits, u):
    """the SAMPLE rule on logits [..., C] and draws u [...]"""
    lg = np.asarray(logits, np.float32).astype(np.float64)
    z = lg - lg.max(axis=-1, keepdims=True)
    e = cz_exp(np.maximum(z, -64.0))
    S = np.cumsum(e, axis=-1)                                  # sequential: S_c = S_(c-1) + e_c
    thr = np.asarray(u, np.float64) * S[..., -1]
    gt = S > thr[..., None]
    return np.where(gt.any(axis=-1), gt.argmax(axis=-1), lg.shape[-1] - 1).astype(np.int32)


def draw(seed, env_global, step, agent):
    """the SAMPLE draw of (env, step, agent): float64 in [0, 1); arrays broadcast"""
    return spawn.uniform(seed, env_global, step, AGENT_KEY + np.asarray(agent, np.uint64), 0)


def host_actions(logits, mode=GREEDY, seed=0, env_global=0, step=0, agent=0):
    """logits [..., C] -> int32 actions [...]; `env_global`, `step` and `agent` broadcast against the leading shape (SAMPLE only)"""
    mode = MODES[mode]
    logits = np.asarray(logits, np.float32)
    if mode == GREEDY:
        return logits.argmax(axis=-1).astype(np.int32)
    u = np.broadcast_to(draw(seed, env_global, step, agent), logits.shape[:-1])
    return sample_from(logits, u)
