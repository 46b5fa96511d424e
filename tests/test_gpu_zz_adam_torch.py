"""GPU + PyTorch in one process: cz_adam_step_device on stacked nn.Parameters, their `.grad`, and torch tensors for the moments and
the state, all on torch's stream.  The device's parameters, moments and state are the numpy model's in bits; they lie within the
derived bound of tests/test_adam_host.py (adam_common.reference_steps) of clip_grad_norm_ + torch.optim.AdamW in float64 on the same
gradients; the largest distance from the same in float32 is printed in float32 ulps of the parameter (no gate: profiles/r36/README.md
records it); and steps replayed from one torch.cuda.graph, with the gradients and *d_lr changed between replays, leave everything
byte for byte the eager run's.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_torch_interop.py (which explains why); the only
skip is "torch is not installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_ADAM_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def test_parameters_grads_and_moments_as_torch_tensors_eagerly_and_from_a_graph():
    if "torch" not in sys.modules and importlib.machinery.PathFinder.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    if not os.environ.get(CHILD_FLAG):
        env = dict(os.environ)
        env[CHILD_FLAG] = "1"
        p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-p", "no:cacheprovider"],
                           env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, f"child pytest failed (rc {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-2000:]}"
        assert "1 passed" in p.stdout, p.stdout[-2000:]
        return
    import torch                                  # first: its bundled HIP runtime then serves the step library too
    torch.cuda.init()
    import numpy as np
    from cooking_zoo_amd import adam
    from cooking_zoo_amd.vec_env import CookingVecEnv
    from adam_common import NAMES, TableProbe, gradients, reference_steps, same, tensors
    A, n, T = 2, 2, 6
    env = CookingVecEnv(8, "crowded_6x5", "crowded_6x5", A, 4, ["TomatoSalad", "TomatoLettuceSalad"], action_scheme="scheme1", num_layouts=3,
                        auto_reset=True)
    env.reset(return_obs=False)
    F, Cn = env.F, env.num_actions
    hyper = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-3, weight_decay=0.01, max_norm=0.5)
    call_kw = dict(betas=(0.9, 0.999), eps=1e-3, weight_decay=0.01, max_norm=0.5)
    P = tensors(F, Cn, n, 21)[0]
    grads = [gradients(F, Cn, n, 300 + t) for t in range(T)]
    lrs = [1e-2 * 0.8 ** t for t in range(T)]
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    on = lambda v: torch.tensor(np.ascontiguousarray(v), device=dev)
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        start = [on(p) for p in P]
        params = [torch.nn.Parameter(p.clone()) for p in start]
        for p in params:
            p.grad = torch.zeros_like(p)
        m, v = [torch.zeros_like(p) for p in start], [torch.zeros_like(p) for p in start]
        state = on(adam.fresh_state())
        d_lr = torch.zeros(1, dtype=torch.float64, device=dev)
        env.load_policy(*params[:4])
        env.load_value(*params[4:])
        env.adam_reserve()

        def restart():
            with torch.no_grad():
                for p, s, a, b in zip(params, start, m, v):
                    p.copy_(s)
                    a.zero_()
                    b.zero_()
                state.copy_(on(adam.fresh_state()))
            env.load_policy(*params[:4])
            env.load_value(*params[4:])

        def feed(t, lr):
            with torch.no_grad():
                for p, g in zip(params, grads[t]):
                    p.grad.copy_(on(g))
                d_lr.fill_(lr)

        def step():
            env.adam_step_device(params, [p.grad for p in params], m, v, state, d_lr=d_lr, lr=0.0, **call_kw)

        # 1. constant learning rate, by value: the model's bits, the bound against float64 torch, the distance from float32 torch
        want = (P, [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P], adam.fresh_state())
        for t in range(T):
            feed(t, 0.0)
            env.adam_step_device(params, [p.grad for p in params], m, v, state, lr=hyper["lr"], **call_kw)
            want = adam.host_adam_step(want[0], grads[t], want[1], want[2], want[3], 3, **hyper)
        side.synchronize()
        host = lambda ts: [x.detach().cpu().numpy() for x in ts]
        got = (host(params), host(m), host(v), state.cpu().numpy())
        same("torch tensors on torch's stream", got, want)
        assert want[3][0] == T and min(float(want[3][4]), 0.99) < 0.99, "the run never clips"
        TableProbe(env, 5).check("torch tensors", want[0])

        def torch_run(dtype):
            ps = [torch.nn.Parameter(s.to(dtype).clone()) for s in start]
            opt = torch.optim.AdamW(ps, lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"],
                                    foreach=False)
            for t in range(T):
                for p, g in zip(ps, grads[t]):
                    p.grad = on(g).to(dtype)
                torch.nn.utils.clip_grad_norm_(ps, hyper["max_norm"])
                opt.step()
            return [p.detach().cpu().numpy() for p in ps]

        ref64, bounds = torch_run(torch.float64), reference_steps(P, grads, 3, **hyper)[1]
        ref32 = torch_run(torch.float32)
        worst_ulps = 0.0
        for name, g, r64, r32, b in zip(NAMES, got[0], ref64, ref32, bounds):
            err = np.abs(g.astype(np.float64) - r64)
            print(f"{name}: largest error / bound against torch float64 {float((err / b).max()):.3f}, largest bound {b.max():.3g}")
            assert (err <= b).all(), f"{name}: {int((err > b).sum())} elements outside the derived bound of torch float64 AdamW + clip_grad_norm_"
            ulps = np.abs(g.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
            worst_ulps = max(worst_ulps, float(ulps.max()))
            at = np.unravel_index(int(ulps.argmax()), ulps.shape)
            print(f"{name}: largest difference from torch float32 AdamW + clip_grad_norm_ after {T} steps: {float(ulps.max()):.2f} float32 ulps of the "
                  f"parameter, at a parameter of {float(r32[at]):.3g} (absolute {abs(float(g[at]) - float(r32[at])):.3g}); median {float(np.median(ulps)):.2f} ulps, "
                  f"largest absolute difference {float(np.abs(g.astype(np.float64) - r32).max()):.3g}")
        print(f"ADAM_TORCH_F32_ULPS {worst_ulps:.2f}")

        # 2. a schedule through *d_lr: eagerly, then as replays of one captured step
        restart()
        want = (P, [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P], adam.fresh_state())
        for t in range(T):
            feed(t, lrs[t])
            step()
            want = adam.host_adam_step(want[0], grads[t], want[1], want[2], want[3], 3, **dict(hyper, lr=lrs[t]))
        side.synchronize()
        eager = [x.detach().clone() for x in params + m + v + [state]]
        same("eager schedule", (host(params), host(m), host(v), state.cpu().numpy()), want)
        restart()
        feed(0, lrs[0])
        step()                                   # (one eager step first, as a learner's warm-up would be)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        for t in range(1, T):
            feed(t, lrs[t])
            g.replay()
        side.synchronize()
        for name, x, e in zip(list(NAMES) * 3 + ["state"], params + m + v + [state], eager):
            assert bool(torch.equal(x.detach().view(torch.int64 if x.dtype == torch.float64 else torch.int32),
                                    e.view(torch.int64 if e.dtype == torch.float64 else torch.int32))), f"{name}: the graph's result differs from the eager run's"
        TableProbe(env, 6).check("after the graph", want[0])
        del g
        side.synchronize()
    env.set_stream(None)
    env.close()
