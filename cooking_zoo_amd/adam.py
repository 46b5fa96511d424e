"""The optimiser on the device (cz_adam_reserve, cz_adam_step_device; device code: k_adam_norm / k_adam_finish / k_adam_update in
csrc/cz_adam.h): global-norm gradient clipping and Adam / AdamW as an arithmetic definition numpy reproduces bit for bit.  One call
updates the caller's parameters in place and writes the packed weight table (csrc/cz_policy.h) with the same new float32, so no
load_policy / load_value follows it.

ARRAYS, all the caller's; the library keeps no optimiser state.  Six parameter tensors P, float32 in torch.nn.Linear's layouts behind
a leading axis of the n loaded sets - w1 [n][64][F], b1 [n][64], w2 [n][C][64], b2 [n][C], wv [n][64], bv [n][1] - and gradients G, first
moments M and second moments V of the same shapes.  The value tensors (wv, bv) may be absent, in all four groups at once.  `set_mask`:
bit k set means set k takes part; every array of a set outside the mask is neither read nor written.

STATE, float64 [8], a fresh one is [0, 1, 1, 0, 0, 0, 0, 0] (fresh_state()):
    [0] steps taken, t          [1] the running product of the beta1 values used      [2] ... of the beta2 values used
    [3] the last call's gradient norm      [4] the last call's clip coefficient       [5] calls skipped
    [6] the learning rate the last call that stepped used                             [7] never written

ARITHMETIC: float64 with every operation rounded on its own; storage is float32.

  Norm.  An element contributes (double)g * (double)g (exact).  Every (tensor, set) segment is cut into chunks of ADAM_CHUNK = 1024
  consecutive elements, the last one padded with +0.0.  Within a chunk lane l of 256 holds s_l = ((sq[l] + sq[l + 256]) + sq[l + 512]) +
  sq[l + 768]; then eight butterfly levels s_l = s_l + s_(l xor 2^k), k = 0 .. 7, after which every lane holds the chunk's partial.
  total = the partials added as ONE serial chain starting from the first, in this order: tensors as listed above, within a tensor the
  masked sets ascending, within a segment the chunks ascending.  The order is part of the definition: independent of grid shape and
  device.  norm = sqrt(total).

  Skip.  If !(total < inf) - an inf or a NaN anywhere in the masked gradients - the call changes nothing in P, M, V and the table; it
  writes [4] = 0.0 and [5] += 1 and leaves [0], [1], [2] and [6] alone.  [3] is not pinned then.

  Clip.  max_norm == 0: coef = 1.0.  Otherwise coef = min(1.0, max_norm / (norm + 1e-6)), torch's clip_grad_norm_.

  Step.  p1 = state[1] * beta1, p2 = state[2] * beta2, bc1 = 1.0 - p1, bc2 = 1.0 - p2; the host computes omb1 = 1.0 - beta1 and omb2 =
  1.0 - beta2 once; lw = lr * weight_decay.  Per element:
      g = coef * (double)G
      m = (float)(beta1 * (double)M + omb1 * g)
      v = (float)(beta2 * (double)V + (omb2 * g) * g)
      mh = (double)m / bc1;  vh = (double)v / bc2
      p = (double)P;  if weight_decay != 0: p = p - lw * p                  (decoupled: AdamW)
      P = (float)(p - lr * (mh / (sqrt(vh) + eps)))
  The stored float32 moments are what the update reads, so a run restarted from saved buffers continues bit for bit.  lr is *d_lr where
  a device pointer is given (a schedule inside a captured graph), the by-value argument otherwise.
  Then state[0 .. 2] = t + 1, p1, p2;  [3] = norm;  [4] = coef;  [6] = lr.

  `/` and sqrt are IEEE's correctly rounded float64 operations (numpy's, math.sqrt's and the device's).

NOT pinned: NaN and subnormal intermediates, an eps so small that a denominator is 0; zeros compare equal whatever their sign."""
import math

import numpy as np

ADAM_CHUNK = 1024
LANES = 256
NAMES = ("w1", "b1", "w2", "b2", "wv", "bv")
_F32, _F64 = np.float32, np.float64


def fresh_state():
    return np.array([0, 1, 1, 0, 0, 0, 0, 0], _F64)


def _group(T):
    """six float32 arrays (the last two None or both present), each [n][...]"""
    T = list(T)
    if len(T) != 6:
        raise ValueError(f"a group holds {len(T)} tensors, not the six of {NAMES}")
    if (T[4] is None) != (T[5] is None):
        raise ValueError("wv and bv are present or absent together")
    return [None if t is None else np.asarray(t, _F32) for t in T]


def _check(P, G, M, V, set_mask):
    n = P[0].shape[0]
    if set_mask <= 0 or set_mask >> n:
        raise ValueError(f"set_mask {set_mask:#x} is empty or names a set past the {n} loaded")
    for grp in (G, M, V):
        for a, b in zip(P, grp):
            if (a is None) != (b is None) or (a is not None and a.shape != b.shape):
                raise ValueError("the four groups differ in shape or in the presence of the value tensors")
    return n, [k for k in range(n) if (set_mask >> k) & 1]


def chunk_partials(seg):
    """the partials of one segment (a flat float32 array), float64 [chunks]"""
    sq = seg.astype(_F64)
    sq = sq * sq
    chunks = -(-sq.size // ADAM_CHUNK)
    pad = np.zeros(chunks * ADAM_CHUNK, _F64)
    pad[:sq.size] = sq
    s = pad.reshape(chunks, ADAM_CHUNK // LANES, LANES)
    lane = s[:, 0]
    for r in range(1, ADAM_CHUNK // LANES):
        lane = lane + s[:, r]
    idx = np.arange(LANES)
    for k in range(8):
        lane = lane + lane[:, idx ^ (1 << k)]
    return lane[:, 0]


def partials_in_order(G, sets):
    """every chunk's partial in the pinned order: tensors as listed, masked sets ascending, chunks ascending"""
    return np.concatenate([chunk_partials(g[k].reshape(-1)) for g in G if g is not None for k in sets])


def grad_total(G, set_mask):
    """the serial chain over partials_in_order"""
    G = _group(G)
    parts = partials_in_order(G, [k for k in range(G[0].shape[0]) if (set_mask >> k) & 1])
    total = parts[0]
    with np.errstate(all="ignore"):
        for p in parts[1:]:
            total = total + p
    return _F64(total)


def host_adam_step(P, G, M, V, state, set_mask, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0):
    """the vectorised model, bit for bit the device's -> (P', M', V', state'), the inputs untouched.  Each group is (w1, b1, w2, b2, wv,
    bv) with the last two None or present; `lr` is the value the call uses (the by-value argument or *d_lr)."""
    P, G, M, V = _group(P), _group(G), _group(M), _group(V)
    _, sets = _check(P, G, M, V, set_mask)
    state = np.array(state, _F64)
    P2, M2, V2 = ([None if t is None else t.copy() for t in grp] for grp in (P, M, V))
    lr, beta1, beta2, eps, wd, max_norm = (_F64(x) for x in (lr, beta1, beta2, eps, weight_decay, max_norm))
    with np.errstate(all="ignore"):
        total = grad_total(G, set_mask)
        norm = np.sqrt(total)
        state[3] = norm
        if not total < np.inf:
            state[4] = 0.0
            state[5] = state[5] + 1.0
            return P2, M2, V2, state
        coef = _F64(1.0) if max_norm == 0 else min(_F64(1.0), max_norm / (norm + _F64(1e-6)))
        p1, p2 = state[1] * beta1, state[2] * beta2
        bc1, bc2 = _F64(1.0) - p1, _F64(1.0) - p2
        omb1, omb2, lw = _F64(1.0) - beta1, _F64(1.0) - beta2, lr * wd
        for i, g32 in enumerate(G):
            if g32 is None:
                continue
            for k in sets:
                g = coef * g32[k].astype(_F64)
                m = (beta1 * M[i][k].astype(_F64) + omb1 * g).astype(_F32)
                v = (beta2 * V[i][k].astype(_F64) + (omb2 * g) * g).astype(_F32)
                mh, vh = m.astype(_F64) / bc1, v.astype(_F64) / bc2
                p = P[i][k].astype(_F64)
                if wd != 0:
                    p = p - lw * p
                P2[i][k] = (p - lr * (mh / (np.sqrt(vh) + eps))).astype(_F32)
                M2[i][k], V2[i][k] = m, v
    state[0], state[1], state[2], state[4], state[6] = state[0] + 1.0, p1, p2, coef, lr
    return P2, M2, V2, state


def _f32(x):
    return float(_F32(x))


def scalar_adam_step(P, G, M, V, state, set_mask, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0):
    """the second model: plain Python floats, one element and one lane at a time; the same signature and result as host_adam_step"""
    P, G, M, V = _group(P), _group(G), _group(M), _group(V)
    _, sets = _check(P, G, M, V, set_mask)
    st = [float(x) for x in np.asarray(state, _F64)]
    P2, M2, V2 = ([None if t is None else t.copy() for t in grp] for grp in (P, M, V))
    lr, beta1, beta2, eps, wd, max_norm = (float(x) for x in (lr, beta1, beta2, eps, weight_decay, max_norm))
    total = None
    for g32 in G:
        if g32 is None:
            continue
        for k in sets:
            seg = [float(x) for x in g32[k].reshape(-1)]
            for c0 in range(0, len(seg), ADAM_CHUNK):
                sq = [x * x for x in seg[c0:c0 + ADAM_CHUNK]]
                sq += [0.0] * (ADAM_CHUNK - len(sq))
                lane = [((sq[l] + sq[l + 256]) + sq[l + 512]) + sq[l + 768] for l in range(LANES)]
                for lvl in range(8):
                    lane = [lane[l] + lane[l ^ (1 << lvl)] for l in range(LANES)]
                total = lane[0] if total is None else total + lane[0]
    st[3] = math.sqrt(total) if total >= 0.0 and total < math.inf else math.nan
    if not total < math.inf:
        st[4] = 0.0
        st[5] = st[5] + 1.0
        return P2, M2, V2, np.array(st, _F64)
    norm = st[3]
    coef = 1.0 if max_norm == 0.0 else min(1.0, max_norm / (norm + 1e-6))
    p1, p2 = st[1] * beta1, st[2] * beta2
    bc1, bc2 = 1.0 - p1, 1.0 - p2
    omb1, omb2, lw = 1.0 - beta1, 1.0 - beta2, lr * wd
    for i, g32 in enumerate(G):
        if g32 is None:
            continue
        for k in sets:
            gs, ms, vs, ps = (t[k].reshape(-1) for t in (g32, M[i], V[i], P[i]))
            om, ov, op = (t[k].reshape(-1) for t in (M2[i], V2[i], P2[i]))          # (views: contiguous copies)
            for e in range(gs.size):
                g = coef * float(gs[e])
                m = _f32(beta1 * float(ms[e]) + omb1 * g)
                v = _f32(beta2 * float(vs[e]) + (omb2 * g) * g)
                mh, vh = m / bc1, v / bc2
                p = float(ps[e])
                if wd != 0.0:
                    p = p - lw * p
                op[e] = _F32(p - lr * (mh / (math.sqrt(vh) + eps)))
                om[e], ov[e] = m, v
    st[0], st[1], st[2], st[4], st[6] = st[0] + 1.0, p1, p2, coef, lr
    return P2, M2, V2, np.array(st, _F64)
