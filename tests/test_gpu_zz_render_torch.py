"""GPU + PyTorch in one process: frames into torch tensors on torch's stream.  `d_chw32` equals
`d_rgb8.permute(0, 3, 1, 2).float() / 255` bit for bit, both equal the host model, and `d_chw32` goes through a torch.nn.Conv2d as it
is: contiguous NCHW float32, no copy and no layout change in front of the convolution.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_effects_torch.py; the only skip is "torch is not
installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_RENDER_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def in_child(name):
    """True inside the child interpreter; in the parent, runs test `name` of this file there and returns False"""
    if "torch" not in sys.modules and importlib.machinery.PathFinder.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    if os.environ.get(CHILD_FLAG):
        return True
    env = dict(os.environ)
    env[CHILD_FLAG] = "1"
    p = subprocess.run([sys.executable, "-m", "pytest", f"{os.path.abspath(__file__)}::{name}", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"child pytest failed (rc {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-2000:]}"
    assert "1 passed" in p.stdout, p.stdout[-2000:]
    return False


def test_frames_in_torch_tensors_feed_a_convolution():
    if not in_child("test_frames_in_torch_tensors_feed_a_convolution"):
        return
    import torch                                  # first: its bundled HIP runtime then serves the step library too
    torch.cuda.init()
    import numpy as np
    from cooking_zoo_amd import render
    from grid_common import checkpoints
    from render_common import random_sheet
    from vec_common import env_of
    n, P, vis = 6, 8, 0b01
    dev = torch.device("cuda", 0)
    tables, points = checkpoints("coop_test", n)
    env = env_of(tables)
    env.reset(return_obs=False)
    env.set_state(points[-1])
    sheet = random_sheet(8)
    env.load_sprites(sheet)
    h, w, _ = env.frame_shape(P)
    rgb = torch.full((n, h, w, 3), 0xAB, dtype=torch.uint8, device=dev)
    chw = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=dev)
    act = torch.zeros((n, env.num_agents), dtype=torch.int32, device=dev)
    rew = torch.empty((n, env.num_agents), dtype=torch.float64, device=dev)
    term = torch.empty((n, env.num_agents), dtype=torch.uint8, device=dev)
    trunc = torch.empty((n, env.num_agents), dtype=torch.uint8, device=dev)
    conv = torch.nn.Conv2d(3, 4, kernel_size=3, padding=1).to(dev)
    side = torch.cuda.Stream(device=dev)
    env.sync()
    torch.cuda.synchronize()
    with torch.cuda.stream(side), torch.no_grad():
        env.set_stream(torch.cuda.current_stream())
        env.render_device(rgb, chw, P=P, vis=vis)
        ptr = chw.data_ptr()
        assert chw.is_contiguous() and chw.dtype == torch.float32 and tuple(chw.shape) == (n, 3, h, w)
        out = conv(chw)                                                   # the tensor as written: no .contiguous(), .to() or permute
        assert chw.data_ptr() == ptr and tuple(out.shape) == (n, 4, h, w)
        same = torch.equal(chw.view(torch.int32), (rgb.permute(0, 3, 1, 2).float() / 255).contiguous().view(torch.int32))
        env.step_device(act, None, rew, term, trunc)                      # a step behind it on the same stream, then the next frame
        rgb2 = torch.empty_like(rgb)
        env.render_device(rgb2, None, P=P, vis=vis)
        side.synchronize()
    env.set_stream(None)
    assert same, "d_chw32 is not d_rgb8.permute(0, 3, 1, 2).float() / 255 bit for bit"
    want = render.host_frame(env.dims, points[-1], P, sheet, vis)
    assert np.array_equal(rgb.cpu().numpy(), want), "rgb8 differs from the host model"
    assert np.array_equal(chw.cpu().numpy().view(np.uint32), render.to_chw32(want).view(np.uint32)), "chw32 differs from the host model"
    ref = torch.nn.functional.conv2d(torch.from_numpy(render.to_chw32(want)).to(dev), conv.weight, conv.bias, padding=1)
    assert torch.equal(out, ref), "the convolution of the frame as written differs from the convolution of the host model's frame"
    assert np.array_equal(rgb2.cpu().numpy(), render.host_frame(env.dims, env.get_state(), P, sheet, vis)), "the frame behind the step"
    env.close()
