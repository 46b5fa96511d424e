"""GPU + PyTorch in one process: torch tensors as the buffers of partner_device, ordered on torch's current stream - a learner's
actions for agent 0 and the scripted partner's for agent 1 in ONE int32 [N, A] tensor that step_device takes - equal the host model.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_grid_torch.py; the only skip is "torch is not
installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_PARTNER_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def test_partner_and_learner_share_one_action_tensor():
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
    from cooking_zoo_amd import partner
    from grid_common import checkpoints
    from partner_common import book_of
    from vec_common import env_of, oracle_for, strip
    n = 6
    tables, points = checkpoints("coop_test", n)
    env = env_of(tables)
    orc = oracle_for(env)
    env.reset(return_obs=False)
    orc.reset()
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    book = book_of(tables)
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        recs = points[1]
        env.set_state(recs)
        orc.records[:] = recs
        acts = torch.full((n, 2), 3, dtype=torch.int32, device=dev)          # the learner's action for everybody
        tg = torch.full((n, 2, 2), -7, dtype=torch.int32, device=dev)
        st = torch.full((n, 2), 99, dtype=torch.uint8, device=dev)
        rew = torch.empty((n, 2), dtype=torch.float64, device=dev)
        term, trunc = (torch.empty((n, 2), dtype=torch.uint8, device=dev) for _ in range(2))
        env.partner_device(acts, tg, st, agents=0b10)                         # agent 1 is the partner
        env.step_device(acts, None, rew, term, trunc)
        side.synchronize()
        want = partner.host_partner(env.dims, tables.layouts, recs, book, agents=0b10)
        a = acts.cpu().numpy()
        assert (a[:, 0] == 3).all() and np.array_equal(a[:, 1], want[0][:, 1])
        assert (tg.cpu().numpy()[:, 0] == -7).all() and np.array_equal(tg.cpu().numpy()[:, 1], want[1][:, 1])
        assert (st.cpu().numpy()[:, 0] == 99).all() and np.array_equal(st.cpu().numpy()[:, 1], want[2][:, 1])
        orc.step(a, want_obs=False)
        assert np.array_equal(strip(env.get_state()), strip(orc.records)), "the records behind the step differ from the oracle's"
    env.set_stream(None)
    env.close()
