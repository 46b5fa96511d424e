"""GPU + PyTorch in one process: the parameters of a torch.nn.Sequential(Linear(F, 64), ReLU(), Linear(64, C)) on the device go straight
into load_policy, cz_rollout_policy runs on torch's stream into torch tensors, and the device's logits are the module's: against its
float64 forward on the same rows every element stays within the standard bound of recursive summation in float32 - gamma_(nnz + 1)
through layer 1 (nnz: the row's non-zero features; a zero feature's fmaf changes nothing), propagated through gamma_70 of layer 2,
gamma_k = k u / (1 - k u), u = 2^-24, evaluated in float64 from |W|, |x| and |b|.  A derived bound, not a tuned tolerance.  Greedy
actions are the argmax of the device's own logits wherever the two largest differ; after one SGD step and a reload the second
launch's logits follow the new weights.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_torch_interop.py (which explains why); the only
skip is "torch is not installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_POLICY_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def logits_and_bound(x, w1, b1, w2, b2):
    """float64 logits of the module on float32 rows x [..., F] and the per-element bound on a float32 evaluation of them"""
    import numpy as np
    x, w1, b1, w2, b2 = (np.asarray(v, np.float64) for v in (x, w1, b1, w2, b2))
    nnz = (x != 0).sum(axis=-1, keepdims=True)
    pre = x @ w1.T + b1
    e1 = gamma(nnz + 1) * (np.abs(x) @ np.abs(w1).T + np.abs(b1))          # layer 1, per hidden unit; ReLU is 1-Lipschitz
    h = np.maximum(pre, 0)
    logits = h @ w2.T + b2
    bound = gamma(70) * ((np.abs(h) + e1) @ np.abs(w2).T + np.abs(b2)) + e1 @ np.abs(w2).T
    return logits, bound + np.abs(logits) * 2.0 ** -50                     # (... and the float64 reference's own rounding)


def test_device_logits_are_the_modules_and_follow_an_sgd_step():
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
    from cooking_zoo_amd.vec_env import CookingVecEnv
    n, A, T = 64, 2, 8
    env = CookingVecEnv(n, "coop_test", "example_odd", A, 5, ["TomatoLettuceSalad", "CarrotBanana"], action_scheme="scheme3", num_layouts=8,
                        auto_reset=True)
    env.reset(return_obs=False)
    F, Cn = env.F, env.num_actions
    assert F == 283 and Cn == 5
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    module = torch.nn.Sequential(torch.nn.Linear(F, 64), torch.nn.ReLU(), torch.nn.Linear(64, Cn)).to(dev)
    params = lambda: (module[0].weight, module[0].bias, module[2].weight, module[2].bias)
    host = lambda: [p.detach().cpu().numpy() for p in params()]
    side = torch.cuda.Stream(device=dev)
    rows0 = torch.empty((n, A, F), dtype=torch.float32, device=dev)
    obs32 = torch.full((T + 1, n, A, F), float("nan"), dtype=torch.float32, device=dev)        # (row T: a guard, never written)
    acts = torch.full((T + 1, n, A), -7, dtype=torch.int32, device=dev)
    logits = torch.full((T + 1, n, A, Cn), float("nan"), dtype=torch.float32, device=dev)

    def launch(step0):
        env.observe_device(d_obs32=rows0)
        env.rollout_policy(T, obs32[:T], acts[:T], logits[:T], sets=(0, 0), mode="greedy", seed=1, step0=step0)
        side.synchronize()
        assert bool(torch.isnan(obs32[T]).all()) and bool(torch.isnan(logits[T]).all()) and bool((acts[T] == -7).all()), "guard rows"
        x = torch.cat([rows0[None], obs32[:T - 1]]).cpu().numpy()
        return x, logits[:T].cpu().numpy(), acts[:T].cpu().numpy()

    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        env.load_policy(*params())
        x, got, played = launch(0)
        old = host()
        want, bound = logits_and_bound(x, *old)
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), float(np.max(np.abs(got - want) / bound))
        assert float(bound.max()) < 1e-4                          # (the bound is of float32 size: the comparison means something)
        top = np.sort(got, axis=-1)
        clear = top[..., -1] != top[..., -2]
        assert clear.mean() > 0.9 and np.array_equal(played[clear], got.argmax(-1)[clear])
        # one SGD step on the device, reload with no host trip, second launch
        opt = torch.optim.SGD(module.parameters(), lr=0.5)
        loss = module(torch.from_numpy(x).to(dev)).pow(2).mean()
        loss.backward()
        opt.step()
        env.load_policy(*params())
        x2, got2, _ = launch(T)
        want2, bound2 = logits_and_bound(x2, *host())
        assert (np.abs(got2.astype(np.float64) - want2) <= bound2).all(), "the logits do not follow the new weights"
        stale, _ = logits_and_bound(x2, *old)
        assert (np.abs(got2.astype(np.float64) - stale) > bound2).mean() > 0.9, "the step did not move the logits: the case shows nothing"
        side.synchronize()
    env.set_stream(None)
    env.close()
