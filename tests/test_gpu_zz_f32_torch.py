"""GPU + PyTorch in one process: a torch.float32 tensor as the buffer of cz_step_device_f32, ordered on torch's current stream - the
rows are what `.float()` makes of the float64 rows of a twin env (torch.equal), step after step, and the handle setting
(cz_set_f32_output) serves the plain step_device call the same way.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_torch_interop.py (which explains why); the only
skip is "torch is not installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_F32_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def test_float32_tensor_on_torchs_stream_equals_float_of_the_float64_rows():
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
    from cooking_zoo_amd.vec_env import CookingVecEnv
    n, A, T = 512, 2, 60
    kw = dict(action_scheme="scheme3", num_layouts=8, auto_reset=True)
    env, twin = (CookingVecEnv(n, "coop_test", "example_odd", A, 25, ["TomatoLettuceSalad", "CarrotBanana"], **kw) for _ in range(2))
    env.reset(return_obs=False)
    twin.reset(return_obs=False)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    F = env.F
    assert F == 283                               # rows of an odd length: agent 1's row starts 4-byte aligned only
    obs32 = torch.full((n, A, F), float("nan"), dtype=torch.float32, device=dev)
    obs64 = torch.empty((n, A, F), dtype=torch.float64, device=dev)
    assert obs32.is_contiguous()
    rew, rew2 = (torch.empty((n, A), dtype=torch.float64, device=dev) for _ in range(2))
    flags = [torch.empty((n, A), dtype=torch.uint8, device=dev) for _ in range(4)]
    table = torch.from_numpy(env.obs_table_f32()).to(dev)
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        twin.set_stream(torch.cuda.current_stream())
        env.observe_device(d_obs32=obs32)
        twin.observe_device(obs64)
        assert torch.equal(obs32, obs64.float())
        for t in range(T):
            if t == T // 2:
                env.set_f32_output(obs32)         # the second half through the handle setting
            acts = torch.randint(0, 5, (n, A), dtype=torch.int32, device=dev, generator=gen)
            if t < T // 2:
                env.step_device_f32(acts, obs32, rew, flags[0], flags[1])
            else:
                env.step_device(acts, None, rew, flags[0], flags[1])
            twin.step_device(acts, obs64, rew2, flags[2], flags[3])
            assert torch.equal(obs32, obs64.float()), t
            assert torch.equal(obs32.view(torch.int32), obs64.float().view(torch.int32)), t
            assert torch.equal(rew.view(torch.int64), rew2.view(torch.int64)) and torch.equal(flags[0], flags[2]) and torch.equal(flags[1], flags[3])
            assert bool(torch.isin(obs32, table).all())          # every value is one of the table's
        side.synchronize()
    env.set_stream(None)
    twin.set_stream(None)
    import numpy as np
    assert np.array_equal(env.get_state(), twin.get_state())
    assert int(env.get_state()[:, 4].min()) >= 1                 # (W_EPISODE) reset passes were encoded too
    env.close()
    twin.close()
