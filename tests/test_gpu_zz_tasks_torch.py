"""GPU + PyTorch in one process: the multi-task loop with torch tensors on torch's stream - step_device_f32 -> reset_device ->
set_tasks_device(list) -> infos_device(goal32) -> a small linear policy over torch.cat([obs32, goal32], -1) - run eagerly and from a
torch.cuda.graph: the same actions, and the records of the oracle loop that replays them with tasks.task_draw.

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_effects_torch.py; the only skip is "torch is not
installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_TASKS_TORCH_CHILD"

pytestmark = pytest.mark.gpu


def test_task_conditioned_policy_eager_and_graph_agree():
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
    from cooking_zoo_amd import soa, tasks
    from vec_common import COOP, env_of, oracle_for, oracle_reset, strip, tables_of
    n, A, T, seed = 32, 2, 40, 9
    dev = torch.device("cuda", 0)
    tables = tables_of(n, **dict(COOP, max_steps=8))
    F, G = tables.F, tables.num_goals
    task_list = np.array([[0, 1, 0, 0], [3, 2, 0, 0], [1, 5, 0, 0]], dtype=np.uint8)
    rng = np.random.default_rng(23)
    weights = torch.from_numpy((0.05 * rng.standard_normal((5, F + G))).astype(np.float32)).to(dev)
    noise = torch.from_numpy(rng.standard_normal((T, n, A, 5)).astype(np.float32)).to(dev)      # exploration: the policy does not sit still

    def make():
        env = env_of(tables, auto_reset=False)
        env.reset(return_obs=False)
        b = dict(obs=torch.zeros((n, A, F), dtype=torch.float32, device=dev), goal=torch.full((n, A, G), 7.0, dtype=torch.float32, device=dev),
                 act=torch.zeros((n, A), dtype=torch.int32, device=dev), log=torch.full((T, n, A), -1, dtype=torch.int32, device=dev),
                 goals=torch.full((T, n, A, G), -1.0, dtype=torch.float32, device=dev), rew=torch.empty((n, A), dtype=torch.float64, device=dev),
                 term=torch.empty((n, A), dtype=torch.uint8, device=dev), trunc=torch.empty((n, A), dtype=torch.uint8, device=dev),
                 list=torch.from_numpy(task_list).to(dev))
        return env, b

    def loop(env, b):
        for t in range(T):
            env.step_device_f32(b["act"], b["obs"], b["rew"], b["term"], b["trunc"])
            env.reset_device(d_obs32=b["obs"])
            env.set_tasks_device(d_task_list=b["list"], seed=seed)
            env.infos_device(d_goal32=b["goal"])
            x = torch.cat([b["obs"], b["goal"]], -1)                                     # [n, A, F + G]
            b["act"].copy_(((x.unsqueeze(-2) * weights).sum(-1) + noise[t]).argmax(-1).to(torch.int32))
            b["log"][t].copy_(b["act"])
            b["goals"][t].copy_(b["goal"])

    eager, be = make()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        eager.set_stream(torch.cuda.current_stream())
        loop(eager, be)
        side.synchronize()
    eager.set_stream(None)
    graphed, bg = make()
    cap = torch.cuda.Stream(device=dev)
    graphed.sync()
    torch.cuda.synchronize()
    graphed.set_stream(cap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        loop(graphed, bg)
    assert (bg["log"].cpu().numpy() == -1).all(), "capturing executed something"
    graph.replay()
    torch.cuda.synchronize()
    graphed.set_stream(None)
    acts = be["log"].cpu().numpy()
    assert np.array_equal(acts, bg["log"].cpu().numpy()), "eager and replay take different actions"
    assert np.array_equal(be["goals"].cpu().numpy(), bg["goals"].cpu().numpy())
    assert len(np.unique(acts)) == 5, "the policy never takes some action: the loop shows little"
    # the oracle loop that replays the logged actions: step, reset of the finished envs, the keyed task call
    orc = oracle_for(tables, auto_reset=0)
    orc.reset()
    prev, words = np.zeros((n, A), np.int32), set()
    goals = be["goals"].cpu().numpy()
    for t in range(T):
        orc.step(prev, want_obs=False)
        for e in np.nonzero(orc.records[:, soa.W_STATUS] & 1)[0]:
            oracle_reset(orc, int(e))
        fresh = orc.records[:, soa.W_T] == 0
        new, refused = tasks.host_set_tasks(tables, orc.records, fresh, task_list=task_list, seed=seed)
        assert not refused.any()
        orc.records[:] = new
        words |= set(new[fresh][:, soa.W_RECIPES].tolist())
        assert np.array_equal(goals[t], tasks.host_infos(tables, orc.records)[0].astype(np.float32)), f"step {t}: goal32"
        prev = acts[t]
    assert len(words) == 3 and int(orc.records[:, soa.W_EPISODE].min()) >= 3, "every task is drawn, over several episodes"
    for name, env in (("eager", eager), ("graph", graphed)):
        assert np.array_equal(strip(env.get_state()), strip(orc.records)), f"{name}: the final records differ from the oracle's"
    eager.close()
    graphed.close()
