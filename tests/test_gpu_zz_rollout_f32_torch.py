"""GPU + PyTorch in one process: a torch.float32 tensor (T, N, A, F) as the trajectory buffer of cz_rollout_f32 and
cz_rollout_actions_f32, ordered on torch's current stream - it holds what `.float()` makes of the float64 trajectory that cz_rollout /
cz_rollout_actions write on a twin env, compared as int32 views; rewards, flags and the records afterwards are the twin's.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_torch_interop.py (which explains why); the only
skip is "torch is not installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_ROLLOUT_F32_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def test_float32_trajectory_tensor_equals_float_of_the_float64_trajectory():
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
    n, A, T = 100, 2, 12
    kw = dict(action_scheme="scheme3", num_layouts=8, auto_reset=True)
    env, twin = (CookingVecEnv(n, "coop_test", "example_odd", A, 5, ["TomatoLettuceSalad", "CarrotBanana"], **kw) for _ in range(2))
    env.reset(return_obs=False)
    twin.reset(return_obs=False)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    F = env.F
    assert F == 283                               # rows of an odd length: every second row starts 4-byte aligned only
    obs32 = torch.full((T + 1, n, A, F), float("nan"), dtype=torch.float32, device=dev)       # (row T: a guard, never written)
    obs64 = torch.empty((T, n, A, F), dtype=torch.float64, device=dev)
    assert obs32[:T].is_contiguous()
    rew, rew2 = (torch.empty((T, n, A), dtype=torch.float64, device=dev) for _ in range(2))
    flags = [torch.empty((T, n, A), dtype=torch.uint8, device=dev) for _ in range(4)]
    table = torch.from_numpy(env.obs_table_f32()).to(dev)
    acts = torch.randint(0, 5, (T, n, A), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def compare(what):
        assert torch.equal(obs32[:T].view(torch.int32), obs64.float().view(torch.int32)), what
        assert bool(torch.isnan(obs32[T]).all()), f"{what}: a store went past the last row"
        assert bool(torch.isin(obs32[:T], table).all())          # every value is one of the table's
        assert torch.equal(rew.view(torch.int64), rew2.view(torch.int64)) and torch.equal(flags[0], flags[2]) and torch.equal(flags[1], flags[3]), what
        obs32.fill_(float("nan"))

    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        twin.set_stream(torch.cuda.current_stream())
        env.rollout_f32(T, 3, 0, obs32[:T], rew, flags[0], flags[1])
        twin.rollout(T, 3, 0, obs64, rew2, flags[2], flags[3])
        compare("cz_rollout_f32")
        env.rollout_actions_f32(acts, T, obs32[:T], rew, flags[0], flags[1])
        twin.rollout_actions(acts, T, obs64, rew2, flags[2], flags[3])
        compare("cz_rollout_actions_f32")
        side.synchronize()
    env.set_stream(None)
    twin.set_stream(None)
    import numpy as np
    assert np.array_equal(env.get_state(), twin.get_state())
    assert int(env.get_state()[:, 4].min()) >= 3                 # (W_EPISODE) reset passes were encoded too
    assert env.stats() == twin.stats()
    env.close()
    twin.close()
