"""GPU + PyTorch in one process: cz_ppo_grad_device on torch tensors on torch's stream, the gradients written straight into `.grad` of
stacked nn.Parameters.  The device's gradients are the numpy model's in bits and lie within the derived bound of
tests/test_ppo_host.py (ppo_common.grad_bound) of torch float64 autograd of the same loss (ppo_torch_ref.reference); then full
updates - gradient, torch.optim.Adam.step, load_policy, load_value - eagerly and from one torch.cuda.graph leave the parameters
byte for byte equal.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_torch_interop.py (which explains why); the only
skip is "torch is not installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_PPO_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def test_gradients_into_parameter_grads_and_three_updates_from_a_graph():
    if "torch" not in sys.modules and importlib.machinery.PathFinder.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    if not os.environ.get(CHILD_FLAG):
        env = dict(os.environ)
        env[CHILD_FLAG] = "1"
        p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"],
                           env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, f"child pytest failed (rc {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-2000:]}"
        assert "1 passed" in p.stdout, p.stdout[-2000:]
        return
    import torch                                  # first: its bundled HIP runtime then serves the step library too
    torch.cuda.init()
    import numpy as np
    from cooking_zoo_amd import ppo
    from cooking_zoo_amd.vec_env import CookingVecEnv
    from policy_common import weights
    from ppo_common import canon, grad_bound, trajectory
    from ppo_torch_ref import reference
    from value_common import value_weights
    A, R, M = 2, 96, 80
    env = CookingVecEnv(8, "crowded_6x5", "crowded_6x5", A, 4, ["TomatoSalad", "TomatoLettuceSalad"], action_scheme="scheme1", num_layouts=3,
                        auto_reset=True)
    env.reset(return_obs=False)
    F, Cn = env.F, env.num_actions
    coef = dict(clip=0.2, c_value=0.5, c_entropy=0.01)
    sets, vsets = (0, 1), (0, 0)                  # agent 0 on a shared trunk; agent 1's policy on set 1, its critic on set 0
    # inputs whose float64 forward keeps every pre-activation and every ratio clear of the edges by more than the bound (the first such seed)
    for seed in range(40):
        W, V = weights(F, Cn, 2, seed, scale2=0.15), value_weights(2, seed)
        data = trajectory(R, A, F, W, sets, seed)
        index = np.random.default_rng(seed).integers(-1, R + 1, M).astype(np.int32)
        bounds, margin_pre, margin_ratio = grad_bound(data, W, V, sets, vsets, index, **coef)
        if margin_pre > 0 and margin_ratio > 0:
            break
    assert margin_pre > 0 and margin_ratio > 0, "no seed keeps the float64 forward clear of the edges"
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    on = lambda v: torch.tensor(np.ascontiguousarray(v), device=dev)
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        start = [on(p) for p in W + V]
        params = [torch.nn.Parameter(p.clone()) for p in start]
        for p in params:
            p.grad = torch.full_like(p, float("nan"))
        x, act, lp, ad, rt = (on(v) for v in data)
        idx = on(index)
        stats = torch.full((8,), float("nan"), dtype=torch.float64, device=dev)
        env.load_policy(*params[:4])
        env.load_value(*params[4:])
        assert env.ppo_reserve(M) == M

        def gradient():
            env.ppo_grad_device(x, act, lp, ad, rt, [p.grad for p in params], d_index=idx, sets=sets, vsets=vsets, d_stats=stats, rows=R, **coef)

        gradient()
        side.synchronize()
        got = [p.grad.cpu().numpy() for p in params]
        want, want_stats = ppo.host_ppo_grad(*data, W, V, sets, vsets, index=index, **coef)
        for name, g, w in zip("gw1 gb1 gw2 gb2 gwv gbv".split(), got, want):
            assert np.array_equal(canon(g), canon(w)), f"{name}: the device's .grad is not the model's in bits"
        assert np.array_equal(canon(stats.cpu().numpy()), canon(want_stats)) and want_stats[4] > 0 and want_stats[7] > 0
        ref = reference(torch, *data, index.astype(np.int64), list(W + V), [s if s is not None else -1 for s in sets],
                        [s if s is not None else -1 for s in vsets], coef["clip"], coef["c_value"], coef["c_entropy"])
        for name, g, r, b in zip("gw1 gb1 gw2 gb2 gwv gbv".split(), got, ref, bounds):
            err = np.abs(g.astype(np.float64) - r.reshape(g.shape))
            print(f"{name}: largest error / bound {float((err / np.maximum(b, 1e-300)).max()):.3f}, largest bound {b.max():.3g}, largest gradient {np.abs(r).max():.3g}")
            assert (err <= b).all(), f"{name}: {int((err > b).sum())} elements outside the derived bound"
            assert np.abs(r).max() > 0

        # full updates: one eager to create Adam's state, then three - eagerly, and as three replays of one captured update
        perms = [on(np.random.default_rng(100 + k).integers(0, R, M).astype(np.int32)) for k in range(4)]

        def update():
            gradient()
            opt.step()
            env.load_policy(*params[:4])
            env.load_value(*params[4:])

        def restart():
            with torch.no_grad():
                for p, s in zip(params, start):
                    p.copy_(s)
            env.load_policy(*params[:4])
            env.load_value(*params[4:])
            return torch.optim.Adam(params, lr=1e-2, capturable=True, foreach=False)

        opt = restart()
        for k in range(4):
            idx.copy_(perms[k])
            update()
        side.synchronize()
        eager = [p.detach().clone() for p in params]
        assert not any(bool(torch.equal(e, s)) for e, s in zip(eager, start)), "the updates moved nothing"
        opt = restart()
        idx.copy_(perms[0])
        update()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            update()
        for k in range(1, 4):
            idx.copy_(perms[k])
            g.replay()
        side.synchronize()
        for name, p, e in zip("w1 b1 w2 b2 wv bv".split(), params, eager):
            assert bool(torch.equal(p.detach().view(torch.int32), e.view(torch.int32))), f"{name}: the graph's parameters differ from the eager run's"
        del g
        side.synchronize()
    env.set_stream(None)
    env.close()
