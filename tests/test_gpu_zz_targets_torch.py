"""GPU + PyTorch in one process: cz_gae_device and cz_logprob_device on torch tensors on torch's stream.

  * gae_device equals, bit for bit, the recurrence of cooking_zoo_amd/targets.py written op for op in torch float64 and rounded with
    .float(): separate torch ops round separately, so there is no tolerance.
  * logprob_device is within half a float32 ulp plus 1e-14 of torch.log_softmax(logits.double()) gathered at the actions: 1e-14 is the
    float64 definition's distance from the exact value (tests/test_targets_host.py), half an ulp the one rounding to float32 (a value
    that sits within 1e-14 of a float32 midpoint may round the other way; the ulp is taken at the reference, so a little slack covers
    the binade edge).
  * the collection phase of PPO - observe -> rollout_policy -> linear critic -> logprob_device -> gae_device - at 64 envs, T = 16 gives
    identical bytes in every buffer eagerly and from a torch.cuda.graph.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_torch_interop.py (which explains why); the only
skip is "torch is not installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_TARGETS_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def torch_gae(torch, r, te, tr, V, gamma, lam):
    """targets.host_gae in torch float64, one op per rounding"""
    T = r.shape[0]
    V = V.double()
    done = (te != 0) | (tr != 0)
    zero = torch.zeros_like(r[0])
    gl = torch.tensor(gamma, dtype=torch.float64, device=r.device) * torch.tensor(lam, dtype=torch.float64, device=r.device)
    A = torch.zeros_like(r[0])
    adv, ret = torch.empty_like(r, dtype=torch.float32), torch.empty_like(r, dtype=torch.float32)
    for t in range(T - 1, -1, -1):
        d = (r[t] + torch.where(done[t], zero, gamma * V[t + 1])) - V[t]
        A = d + torch.where(done[t], zero, gl * A)
        adv[t] = A.float()
        ret[t] = (A + V[t]).float()
    return adv, ret


def test_targets_on_torch_tensors_and_the_collection_loop_from_a_graph():
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
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from targets_common import gae_data, synthetic_logits
    from cooking_zoo_amd.vec_env import CookingVecEnv
    n, A, T = 64, 2, 16
    env = CookingVecEnv(n, "coop_test", "example", A, 12, ["TomatoLettuceSalad", "CarrotBanana"], action_scheme="scheme3", num_layouts=8,
                        auto_reset=True)
    env.reset(return_obs=False)
    F, Cn = env.F, env.num_actions
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    side = torch.cuda.Stream(device=dev)
    same = lambda a, b: bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())

        # ---- gae_device against the recurrence in torch float64, as bits
        for T_, n_, flags in ((33, 549, "both"), (7, 37, "term")):
            r, te, tr, V = (torch.from_numpy(a).to(dev) for a in gae_data(T_, n_, A, seed=T_, flags=flags))
            adv, ret = (torch.full((T_ + 1, n_, A), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
            env.gae_device(T_, r, te, tr, V, adv[:T_], ret[:T_], gamma=0.99, lam=0.95, env_count=n_)
            want_adv, want_ret = torch_gae(torch, r, te, tr, V, 0.99, 0.95)
            side.synchronize()
            assert bool(torch.isnan(adv[T_]).all()) and bool(torch.isnan(ret[T_]).all()), "guard rows"
            assert same(adv[:T_], want_adv) and same(ret[:T_], want_ret), f"T = {T_}, {n_} envs: not the torch float64 recurrence's bits"
            assert bool(((te | tr) != 0).any())

        # ---- logprob_device against torch.log_softmax in float64
        rows = 549 * 3
        lg = torch.from_numpy(synthetic_logits(rows, A, Cn, seed=2)).to(dev)
        act = torch.randint(0, Cn, (rows, A), dtype=torch.int32, device=dev)
        logp, ent = (torch.full((rows + 1, A), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
        env.logprob_device(lg, act, logp[:rows], ent[:rows], sets=(0, 0), rows=rows)
        ref = torch.log_softmax(lg.double(), dim=-1)
        want = ref.gather(-1, act.long()[..., None])[..., 0]
        side.synchronize()
        assert bool(torch.isnan(logp[rows]).all()) and bool(torch.isnan(ent[rows]).all()), "guard rows"
        ulp = torch.from_numpy(np.spacing(np.abs(want.cpu().numpy()).astype(np.float32)).astype(np.float64)).to(dev)
        err = (logp[:rows].double() - want).abs()
        assert bool((err <= 0.5 * ulp + 1e-14).all()), float((err - 0.5 * ulp).max())
        want_ent = -(ref.exp() * ref).sum(-1)
        assert float((ent[:rows].double() - want_ent).abs().max()) <= 1e-6

        # ---- the collection phase, eagerly and from a torch.cuda.graph: identical bytes in every buffer
        module = torch.nn.Sequential(torch.nn.Linear(F, 64), torch.nn.ReLU(), torch.nn.Linear(64, Cn)).to(dev)
        with torch.no_grad():
            module[2].weight.mul_(0.1)
        critic = torch.nn.Linear(F, 1).to(dev)
        env.load_policy(module[0].weight, module[0].bias, module[2].weight, module[2].bias)
        names = dict(obs=((T + 1, n, A, F), torch.float32), act=((T, n, A), torch.int32), logits=((T, n, A, Cn), torch.float32),
                     rew=((T, n, A), torch.float64), term=((T, n, A), torch.uint8), trunc=((T, n, A), torch.uint8),
                     val=((T + 1, n, A), torch.float32), logp=((T, n, A), torch.float32), ent=((T, n, A), torch.float32),
                     adv=((T, n, A), torch.float32), ret=((T, n, A), torch.float32))
        b = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in names.items()}

        def collect():
            env.observe_device(d_obs32=b["obs"][0])
            env.rollout_policy(T, b["obs"][1:], b["act"], b["logits"], b["rew"], b["term"], b["trunc"], sets=(0, 0), mode="sample", seed=3, step0=0)
            with torch.no_grad():
                torch.Tensor.copy_(b["val"], critic(b["obs"])[..., 0])
            env.logprob_device(b["logits"], b["act"], b["logp"], b["ent"], sets=(0, 0), rows=T * n)
            env.gae_device(T, b["rew"], b["term"], b["trunc"], b["val"], b["adv"], b["ret"])

        state0 = env.get_state()
        collect()                                                     # (also warms the critic's kernels up in front of the capture)
        side.synchronize()
        eager = {k: v.clone() for k, v in b.items()}
        assert bool(((eager["term"] | eager["trunc"]) != 0).any()) and len(torch.unique(eager["act"])) >= 2
        assert bool((eager["logp"] < 0).any()) and bool((eager["adv"] != 0).any())
        want_adv, want_ret = torch_gae(torch, eager["rew"], eager["term"], eager["trunc"], eager["val"], 0.99, 0.95)
        assert same(eager["adv"], want_adv) and same(eager["ret"], want_ret)
        env.set_state(state0)
        for v in b.values():
            v.zero_()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            collect()
        assert all(not bool(v.any()) for v in b.values()), "capturing must not have launched anything"
        g.replay()
        side.synchronize()
        for k, v in b.items():
            assert bool(torch.equal(v.view(torch.uint8), eager[k].view(torch.uint8))), f"{k}: the graph's bytes differ from the eager run's"
        del g
        side.synchronize()
    env.set_stream(None)
    env.close()
