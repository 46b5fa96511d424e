"""Data shared by the tests of cz_gae_device and cz_logprob_device (definition: cooking_zoo_amd/targets.py): the reward / value / done
family of the GAE tests, synthetic logits with ties and clamp cases, the sentinels of guarded float32 outputs.
(pytest rewrites asserts in test modules only: every assert here carries its own message.)"""
import numpy as np

F32_SENT = 0x7FC0BEEF                                           # float32 outputs, as uint32: a quiet NaN no result equals
ACT_OUTSIDE = -7777                                             # policy_common.ACT_SENT: the action of an agent that did not act
GAMMA, LAM = 0.99, 0.95
REWARD_EVENTS = (-0.01, 1.0, 19.9875, -0.5)                     # what replaces the time penalty in 10 % of the steps


DONE_BYTES = (2, 0x80, 0xFF)                                     # flag bytes other than 1: the definition is `!= 0`


def gae_data(T, n, A, seed=0, flags="both", done_share=0.08, byte=None):
    """-> rewards float64 [T, n, A], term uint8 [T, n, A], trunc uint8 [T, n, A], values float32 [T + 1, n, A]: rewards -0.0125 with
    10 % replaced from REWARD_EVENTS, values standard normal, `done_share` of the steps done - `flags`: "term" / "trunc" put every
    done into that array alone, "both" spreads them over term, trunc and both at once.  `byte`: None writes a set flag as 1; a
    sequence of non-zero bytes writes each set flag as one of them, and where both flags are set term = 0x01 with trunc = 0xFE (no
    bit in common).  The same steps are done either way."""
    rng = np.random.default_rng(seed)
    shape = (T, n, A)
    rewards = np.full(shape, -0.0125)
    event = rng.random(shape) < 0.10
    rewards[event] = rng.choice(REWARD_EVENTS, int(event.sum()))
    values = rng.standard_normal((T + 1, n, A)).astype(np.float32)
    done = rng.random(shape) < done_share
    kind = rng.integers(0, 3, shape)
    term, trunc = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    if flags == "term":
        term[done] = 1
    elif flags == "trunc":
        trunc[done] = 1
    else:
        assert flags == "both", f"flags = {flags!r}"
        term[done & (kind != 1)] = 1
        trunc[done & (kind != 0)] = 1
    if byte is not None:
        assert all(0 < int(b) < 256 for b in byte), f"byte = {byte!r}"
        both = (term != 0) & (trunc != 0)
        for arr in (term, trunc):
            arr[arr != 0] = rng.choice(np.array(byte, np.uint8), int((arr != 0).sum()))
        term[both], trunc[both] = 0x01, 0xFE
    return rewards, term, trunc, values


def gae_float32(rewards, term, trunc, values, gamma, lam):
    """the advantages of host_gae's recurrence carried in float32 instead of float64: what the bits of a comparison must tell apart"""
    f = np.float32
    r32, V = np.asarray(rewards).astype(f), np.asarray(values, f)
    done = (np.asarray(term) != 0) | (np.asarray(trunc) != 0)
    g, gl = f(gamma), f(f(gamma) * f(lam))
    A, out = np.zeros(r32.shape[1:], f), np.empty(r32.shape, f)
    for t in range(r32.shape[0] - 1, -1, -1):
        d = (r32[t] + np.where(done[t], f(0), g * V[t + 1])) - V[t]
        A = d + np.where(done[t], f(0), gl * A)
        assert A.dtype == f, "gae_float32: the recurrence left float32"
        out[t] = A
    return out


def scalar_gae(rewards, term, trunc, values, gamma, lam):
    """the definition as Python-float loops, one series at a time: a second model for host_gae"""
    r = np.asarray(rewards, np.float64)
    T = r.shape[0]
    r2, V2 = r.reshape(T, -1), np.asarray(values, np.float32).reshape(T + 1, -1)
    te = np.asarray(term).reshape(T, -1)
    tr = np.zeros_like(te) if trunc is None else np.asarray(trunc).reshape(T, -1)
    adv, ret = np.empty(r2.shape, np.float32), np.empty(r2.shape, np.float32)
    gamma, lam = float(gamma), float(lam)
    gl = gamma * lam
    for i in range(r2.shape[1]):
        A = 0.0
        for t in range(T - 1, -1, -1):
            done = te[t, i] != 0 or tr[t, i] != 0
            v = float(V2[t, i])
            d = (float(r2[t, i]) + (0.0 if done else gamma * float(V2[t + 1, i]))) - v
            A = d + (0.0 if done else gl * A)
            adv[t, i] = np.float32(A)
            ret[t, i] = np.float32(A + v)
    return adv.reshape(r.shape), ret.reshape(r.shape)


def synthetic_logits(rows, A, C, seed=0):
    """float32 [rows, A, C]: standard normal times a scale from 0.1 to 30 per row; every seventh row has its two first logits equal
    and largest (a tie at the maximum), every eleventh one logit 1000 below the maximum (the clamp at -64), every thirteenth all equal"""
    rng = np.random.default_rng(100 + seed)
    scale = rng.choice([0.1, 1.0, 3.0, 10.0, 30.0], (rows, A, 1))
    lg = (rng.standard_normal((rows, A, C)) * scale).astype(np.float32)
    k = np.arange(rows)
    tie = k % 7 == 3
    lg[tie, :, 1] = lg[tie, :, 0] = lg[tie].max(axis=-1) + np.float32(0.5)
    far = k % 11 == 5
    lg[far, :, C - 1] = lg[far].max(axis=-1) - np.float32(1000.0)
    lg[k % 13 == 6] = np.float32(0.25)
    return lg


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
