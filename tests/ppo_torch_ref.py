"""The reference of the PPO gradient tests: torch float64 autograd of the loss written the usual way - log_softmax, torch.min, clamp
and mse_loss - over the stacked parameters of `Sequential(Linear(F, 64), ReLU(), Linear(64, C))` and `Linear(64, 1)` per set.

`reference(...)` is imported where torch is already there (the GPU test's child interpreter); as a script it reads an .npz of inputs
and writes an .npz of gradients, for a test whose own interpreter must not import torch (tests/test_ppo_host.py).  No assert here:
the callers compare."""
import sys

VARIANTS = ("loss", "clip ignored", "entropy sign flipped")


def reference(torch, obs, act, lpo, adv, ret, idx, params, sets, vsets, clip, c_value, c_entropy, variant="loss"):
    """numpy inputs (any float type; `sets` / `vsets` ints with -1 = none; `idx` int64 [M]) -> six float64 numpy gradients in the
    stacked layouts.  `variant`: one of VARIANTS - the two wrong ones are what a comparison must tell apart."""
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    P = [f64(p).requires_grad_(True) for p in params]
    w1, b1, w2, b2, wv, bv = P
    obs, lpo, adv, ret = f64(obs), f64(lpo), f64(adv), f64(ret)
    act, idx = torch.tensor(act, dtype=torch.int64), torch.tensor(idx, dtype=torch.int64)
    R, A, _ = obs.shape
    C, M = w2.shape[1], len(idx)
    valid = (idx >= 0) & (idx < R)
    rows = idx[valid]
    n_p, n_v = sum(int(s) >= 0 for s in sets[:A]), sum(int(s) >= 0 for s in vsets[:A])
    total = torch.zeros((), dtype=torch.float64)
    for a in range(A):
        s, vs = int(sets[a]), int(vsets[a])
        x = obs[rows, a]
        if s >= 0:
            acted = (act[rows, a] >= 0) & (act[rows, a] < C)
            xa, aa = x[acted], act[rows, a][acted]
            h = torch.relu(xa @ w1[s].T + b1[s])
            logq = torch.log_softmax(h @ w2[s].T + b2[s], dim=-1)
            ratio = torch.exp(logq.gather(1, aa[:, None])[:, 0] - lpo[rows, a][acted])
            Adv = adv[rows, a][acted]
            s1 = ratio * Adv
            surr = s1 if variant == "clip ignored" else torch.min(s1, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * Adv)
            entropy = -(torch.exp(logq) * logq).sum(dim=-1)
            sign = 1.0 if variant == "entropy sign flipped" else -1.0
            total = total + (-surr.sum() + sign * c_entropy * entropy.sum()) / (M * n_p)
        if vs >= 0:
            v = torch.relu(x @ w1[vs].T + b1[vs]) @ wv[vs].reshape(-1) + bv[vs].reshape(())
            total = total + c_value * 0.5 * torch.nn.functional.mse_loss(v, ret[rows, a], reduction="sum") / (M * n_v)
    total.backward()
    return [torch.zeros_like(p).numpy() if p.grad is None else p.grad.numpy() for p in P]


def main(src, dst):
    import numpy as np
    import torch
    d = np.load(src)
    out = {}
    for k, variant in enumerate(VARIANTS):
        grads = reference(torch, d["obs"], d["act"], d["lpo"], d["adv"], d["ret"], d["idx"], [d[f"p{i}"] for i in range(6)], d["sets"], d["vsets"],
                          float(d["coef"][0]), float(d["coef"][1]), float(d["coef"][2]), variant)
        for i, g in enumerate(grads):
            out[f"v{k}_g{i}"] = g
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
