"""GPU + PyTorch in one process: the parameters of a torch.nn.Linear(64, 1) value head on the device go straight into load_value on
torch's stream, cz_value_device and cz_rollout_policy_value write torch tensors, and the device's values are the module's: against
the float64 forward of Sequential(Linear(F, 64), ReLU(), Linear(64, 1)) on the same rows every element stays within the standard
bound of recursive summation in float32 that tests/test_gpu_zz_policy_torch.py uses for logits - gamma_(nnz + 1) through layer 1,
propagated through gamma_70 of layer 2, gamma_k = k u / (1 - k u), u = 2^-24, evaluated in float64 from |W|, |x| and |b|.  A derived
bound, not a tuned tolerance.  Then the collection phase of PPO as four calls - observe -> rollout with values -> logprob_device ->
gae_device - with a shared trunk and with a separate critic network, eagerly and from a torch.cuda.graph: identical bytes in every
buffer.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_torch_interop.py (which explains why); the only
skip is "torch is not installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_VALUE_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def outputs_and_bound(x, w1, b1, w2, b2):
    """float64 outputs of the module on float32 rows x [..., F] and the per-element bound on a float32 evaluation of them"""
    import numpy as np
    x, w1, b1, w2, b2 = (np.asarray(v, np.float64) for v in (x, w1, b1, w2, b2))
    nnz = (x != 0).sum(axis=-1, keepdims=True)
    pre = x @ w1.T + b1
    e1 = gamma(nnz + 1) * (np.abs(x) @ np.abs(w1).T + np.abs(b1))          # layer 1, per hidden unit; ReLU is 1-Lipschitz
    h = np.maximum(pre, 0)
    out = h @ w2.T + b2
    bound = gamma(70) * ((np.abs(h) + e1) @ np.abs(w2).T + np.abs(b2)) + e1 @ np.abs(w2).T
    return out, bound + np.abs(out) * 2.0 ** -50                           # (... and the float64 reference's own rounding)


def test_device_values_are_the_modules_and_the_four_call_collection_phase_from_a_graph():
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
    n, A, T = 64, 2, 7
    env = CookingVecEnv(n, "coop_test", "example_odd", A, 5, ["TomatoLettuceSalad", "CarrotBanana"], action_scheme="scheme3", num_layouts=8,
                        auto_reset=True)
    env.reset(return_obs=False)
    F, Cn = env.F, env.num_actions
    assert F == 283 and Cn == 5
    dev = torch.device("cuda", 0)
    torch.manual_seed(17)
    # set 0: actor and critic on one trunk; set 1: a critic network of its own (its action head is never used)
    trunks = [torch.nn.Sequential(torch.nn.Linear(F, 64), torch.nn.ReLU()).to(dev) for _ in range(2)]
    actors = [torch.nn.Linear(64, Cn).to(dev) for _ in range(2)]
    critics = [torch.nn.Linear(64, 1).to(dev) for _ in range(2)]
    with torch.no_grad():
        for a in actors:
            a.weight.mul_(0.1)
    stack = lambda ps: torch.stack([p.detach() for p in ps]).contiguous()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        env.load_policy(stack([t[0].weight for t in trunks]), stack([t[0].bias for t in trunks]), stack([a.weight for a in actors]),
                        stack([a.bias for a in actors]))
        # one value head straight from the module's own parameters, [1, 64] and [1]; then the stack of both
        env.load_value(critics[0].weight, critics[0].bias)
        assert env.value_sets == 1
        env.load_value(stack([c.weight for c in critics]), stack([c.bias for c in critics]))
        assert env.value_sets == 2 and env.policy_sets == 2
        host = lambda s: [p.detach().cpu().numpy() for p in (trunks[s][0].weight, trunks[s][0].bias, critics[s].weight, critics[s].bias)]

        names = dict(obs=((T + 1, n, A, F), torch.float32), act=((T, n, A), torch.int32), logits=((T, n, A, Cn), torch.float32),
                     rew=((T, n, A), torch.float64), term=((T, n, A), torch.uint8), trunc=((T, n, A), torch.uint8),
                     val=((T + 2, n, A), torch.float32), logp=((T, n, A), torch.float32), ent=((T, n, A), torch.float32),
                     adv=((T, n, A), torch.float32), ret=((T, n, A), torch.float32))
        b = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in names.items()}
        sets = (0, 0)

        def collect(vsets):                                           # the collection phase: four calls, no torch in it
            env.observe_device(d_obs32=b["obs"][0])
            env.rollout_policy_value(T, b["obs"][1:], b["val"][:T + 1], b["act"], b["logits"], b["rew"], b["term"], b["trunc"], sets=sets,
                                     vsets=vsets, mode="sample", seed=3, step0=0)
            env.logprob_device(b["logits"], b["act"], b["logp"], b["ent"], sets=sets, rows=T * n)
            env.gae_device(T, b["rew"], b["term"], b["trunc"], b["val"][:T + 1], b["adv"], b["ret"])

        state0 = env.get_state()
        for vsets in ((0, 0), (1, 1), (0, 1)):                        # shared trunk, separate critic, one of each
            env.set_state(state0)
            for v in b.values():
                v.zero_()
            b["val"].fill_(float("nan"))
            collect(vsets)
            side.synchronize()
            eager = {k: v.clone() for k, v in b.items()}
            assert bool(torch.isnan(eager["val"][T + 1]).all()) and not bool(torch.isnan(eager["val"][:T + 1]).any()), "guard row / every value written"
            assert bool(((eager["term"] | eager["trunc"]) != 0).any()) and len(torch.unique(eager["act"])) >= 2
            x, got = eager["obs"].cpu().numpy(), eager["val"][:T + 1].cpu().numpy()
            for a in range(A):
                want, bound = outputs_and_bound(x[:, :, a], *host(vsets[a]))
                want, bound = want[..., 0], bound[..., 0]
                err = np.abs(got[:, :, a].astype(np.float64) - want)
                print(f"vsets {vsets}, agent {a}: largest error / bound {float((err / bound).max()):.3f}, largest bound {float(bound.max()):.3g}")
                assert (err <= bound).all(), float(np.max(err / bound))
                assert float(bound.max()) < 1e-4                      # (the bound is of float32 size: the comparison means something)
                other, _ = outputs_and_bound(x[:, :, a], *host(1 - vsets[a]))
                assert (np.abs(got[:, :, a].astype(np.float64) - other[..., 0]) > bound).mean() > 0.9, "both critics fit: the case shows nothing"
            # cz_value_device over the whole trajectory, [T + 1] * n rows in one launch: the rollout's own values
            again = torch.full((T + 2, n, A), float("nan"), dtype=torch.float32, device=dev)
            env.value_device(eager["obs"], again[:T + 1], vsets=vsets, rows=(T + 1) * n)
            side.synchronize()
            assert bool(torch.equal(again.view(torch.int32), eager["val"].view(torch.int32))), "value_device on the trajectory differs from the rollout's values"
            # the same phase from a torch.cuda.graph
            env.set_state(state0)
            for v in b.values():
                v.zero_()
            b["val"].fill_(float("nan"))
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                collect(vsets)
            assert all(not bool(v.any()) for k, v in b.items() if k != "val") and bool(torch.isnan(b["val"]).all()), "capturing must not have launched anything"
            g.replay()
            side.synchronize()
            for k, v in b.items():
                assert bool(torch.equal(v.view(torch.uint8), eager[k].view(torch.uint8))), f"vsets {vsets}, {k}: the graph's bytes differ from the eager run's"
            del g
            side.synchronize()
    env.set_stream(None)
    env.close()
