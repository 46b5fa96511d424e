"""GPU + PyTorch in one process: a torch.float32 tensor (N, W, H, C) as the `d_grid32` buffer of observe_grid_device, ordered on
torch's current stream, equals the host model - and its permute(0, 3, 1, 2) is the channels_last image a convolution takes.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_f32_torch.py; the only skip is "torch is not
installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_GRID_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def test_float32_grid_tensor_is_the_host_model_and_a_channels_last_image():
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
    from cooking_zoo_amd import grid
    from grid_common import checkpoints
    from vec_common import env_of
    n = 6
    tables, points = checkpoints("crowded_6x5", n)                 # 6 x 5: W != H
    env = env_of(tables)
    env.reset(return_obs=False)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    acts = torch.zeros((n, env.num_agents), dtype=torch.int32, device=dev)
    rew = torch.empty((n, env.num_agents), dtype=torch.float64, device=dev)
    term, trunc = (torch.empty((n, env.num_agents), dtype=torch.uint8, device=dev) for _ in range(2))
    for ext in (False, True):
        W, H, C = env.grid_shape(ext)
        assert (W, H) == (6, 5)
        with torch.cuda.stream(side):
            env.set_stream(torch.cuda.current_stream())
            for recs in points:
                env.set_state(recs)
                g = torch.full((n, W, H, C), float("nan"), dtype=torch.float32, device=dev)
                xy = torch.full((n, env.num_agents, 2), -1, dtype=torch.int32, device=dev)
                env.observe_grid_device(d_grid32=g, d_agent_xy=xy, extended=ext)
                want = grid.expand(grid.host_bits(env.dims, recs, ext), np.float32)
                assert torch.equal(g.cpu(), torch.from_numpy(want))
                assert torch.equal(xy.cpu(), torch.from_numpy(grid.agent_xy(env.dims, recs)))
                img = g.permute(0, 3, 1, 2)
                assert img.shape == (n, C, W, H) and img.is_contiguous(memory_format=torch.channels_last)
                assert img.data_ptr() == g.data_ptr()                        # a view, no copy
            # the loop of INTEGRATION.md: a step without observation, then the grid, then the policy's input
            env.step_device(acts, None, rew, term, trunc)
            env.observe_grid_device(d_grid32=g, extended=ext)
            per_cell = g.permute(0, 3, 1, 2).sum(1)                          # what a consumer of the image does first: reads it
            side.synchronize()
            want = grid.expand(grid.host_bits(env.dims, env.get_state(), ext), np.float32)
            assert torch.equal(g.cpu(), torch.from_numpy(want))
            assert torch.equal(per_cell.cpu(), torch.from_numpy(want.sum(-1)))
        env.set_stream(None)
    env.close()
