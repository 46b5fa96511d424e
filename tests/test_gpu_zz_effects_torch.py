"""GPU + PyTorch in one process: a masked policy with no host in it - action_effects_device(mask) -> argmax of seeded random logits
with the masked-out entries at -inf -> step_device, torch tensors on torch's stream - run eagerly, from a torch.cuda.graph, and on
the oracle with the host model's masks: the same actions and final records.  And the property of every action the masked policy
took on a single-agent env: action 0, or the record it left differs from the record action 0 leaves from the same state (a fork).

Runs in a fresh child interpreter that imports torch first, like tests/test_gpu_zz_partner_torch.py; the only skip is "torch is not
installed"."""
import importlib.machinery
import os
import subprocess
import sys

import pytest

CHILD_FLAG = "CZ_EFFECTS_TORCH_CHILD"

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
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, f"child pytest failed (rc {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-2000:]}"
    assert "1 passed" in p.stdout, p.stdout[-2000:]
    return False


def test_masked_policy_eager_graph_and_oracle_agree():
    if not in_child("test_masked_policy_eager_graph_and_oracle_agree"):
        return
    import torch                                  # first: its bundled HIP runtime then serves the step library too
    torch.cuda.init()
    import numpy as np
    import effects_common as ec
    from cooking_zoo_amd import effects, soa
    from vec_common import TWO, make_env, oracle_for, strip
    n, A, T = 64, 2, 100
    dev = torch.device("cuda", 0)
    logits_host = np.random.default_rng(17).standard_normal((T, n, A, 5)).astype(np.float32)
    logits = torch.from_numpy(logits_host).to(dev)

    def make():
        env = make_env(n, "coop_test", "example", A, TWO, "scheme3", max_steps=40, num_layouts=8)
        env.reset(return_obs=False)
        b = dict(mask=torch.full((n, A, 5), 7, dtype=torch.uint8, device=dev), act=torch.zeros((n, A), dtype=torch.int32, device=dev),
                 log=torch.full((T, n, A), -1, dtype=torch.int32, device=dev), rew=torch.empty((n, A), dtype=torch.float64, device=dev),
                 term=torch.empty((n, A), dtype=torch.uint8, device=dev), trunc=torch.empty((n, A), dtype=torch.uint8, device=dev))
        return env, b

    def loop(env, b):
        for t in range(T):
            env.action_effects_device(b["mask"])
            b["act"].copy_(logits[t].masked_fill(~b["mask"].bool(), float("-inf")).argmax(-1).to(torch.int32))
            b["log"][t].copy_(b["act"])
            env.step_device(b["act"], None, b["rew"], b["term"], b["trunc"])

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
    # the oracle with the host model's masks and the same logits
    orc = oracle_for(eager)
    orc.reset()
    want_acts = np.empty((T, n, A), np.int32)
    for t in range(T):
        mask = effects.mask_of(ec.model(eager, orc.records))
        want_acts[t] = np.where(mask != 0, logits_host[t], -np.inf).argmax(-1)
        orc.step(want_acts[t], want_obs=False)
    assert (want_acts != 0).mean() > 0.5, "the masked policy mostly idles: the loop shows nothing"
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 1, "no env finished an episode: the finished-env rows were never met"
    for name, env, b in (("eager", eager, be), ("graph", graphed, bg)):
        got = b["log"].cpu().numpy()
        bad = np.argwhere(got != want_acts)
        assert not len(bad), f"{name}: the actions differ from the oracle loop's first at (step, env, agent) {bad[0].tolist()}"
        assert np.array_equal(strip(env.get_state()), strip(orc.records)), f"{name}: the final records differ from the oracle's"
    eager.close()
    graphed.close()


def test_every_action_the_masked_policy_takes_changes_something():
    if not in_child("test_every_action_the_masked_policy_takes_changes_something"):
        return
    import torch
    torch.cuda.init()
    import numpy as np
    from cooking_zoo_amd import effects, soa
    from vec_common import DENSE_RECIPES, make_env
    n, T = 32, 30
    dev = torch.device("cuda", 0)
    env = make_env(2 * n, "dense_8x8", "dense_8x8", 1, DENSE_RECIPES[:1], "scheme3", max_steps=500, num_layouts=8)
    env.reset(return_obs=False)
    d = env.dims
    words = np.r_[soa.AGENT_WORD0:soa.AGENT_WORD0 + 1, d.cells_word0:d.cells_word0 + d.CW, d.dyn0_word0:d.dyn1_word0 + d.D]
    src = torch.cat([torch.full((n,), -1, dtype=torch.int32), torch.arange(n, dtype=torch.int32)]).to(dev)       # env n + e forks env e
    mask = torch.zeros((n, 1, 5), dtype=torch.uint8, device=dev)
    act = torch.zeros((2 * n, 1), dtype=torch.int32, device=dev)
    rew = torch.empty((2 * n, 1), dtype=torch.float64, device=dev)
    term, trunc = (torch.empty((2 * n, 1), dtype=torch.uint8, device=dev) for _ in range(2))
    gen = torch.Generator(device=dev).manual_seed(3)
    taken = np.zeros(5, np.int64)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        for t in range(T):
            env.fork_device(src)
            env.action_effects_device(mask, ignore=effects.TURNED if t % 2 else 0, env_count=n)
            logits = torch.randn((n, 1, 5), device=dev, generator=gen)
            act[:n].copy_(logits.masked_fill(~mask.bool(), float("-inf")).argmax(-1).to(torch.int32))      # (the forks play 0)
            env.step_device(act, None, rew, term, trunc)
            side.synchronize()
            recs, a = env.get_state(), act.cpu().numpy()[:n, 0]
            same = (recs[:n][:, words] == recs[n:][:, words]).all(axis=1)
            turned_only = ((recs[:n, soa.AGENT_WORD0] ^ recs[n:, soa.AGENT_WORD0]) & 0xFF00FFFF) == 0
            others = np.delete(words, 0)
            turned_only &= (recs[:n][:, others] == recs[n:][:, others]).all(axis=1)
            assert (act.cpu().numpy()[n:, 0] == 0).all()
            bad = np.nonzero((a != 0) & (same | (turned_only if t % 2 else False)))[0]
            assert not len(bad), f"step {t}: envs {bad[:6].tolist()} took actions {a[bad][:6].tolist()} that left what action 0 leaves"
            taken += np.bincount(a, minlength=5)
    env.set_stream(None)
    assert (taken[1:] > 0).all(), f"the masked policy never took some walk code: {taken.tolist()}"
    env.close()
