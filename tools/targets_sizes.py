#!/usr/bin/env python3
"""What the two PPO targets cost (cz_gae_device, cz_logprob_device; cooking_zoo_amd/targets.py) next to the same work in torch, at
config 2's shape (coop_test, 2 agents, scheme3, F = 278, 5 actions), 4096 and 65 536 envs, T = 32 and 128; medians per call between
device events on one stream:

  gae_device                      cz_gae_device over [T, n, 2] (the library's default k_gae instance)
  gae torch loop                  the same recurrence in torch float64, T iterations of elementwise ops, eager
  gae torch loop from a graph     that loop captured once into a torch.cuda.graph and replayed
  logprob_device                  cz_logprob_device over T * n rows, log-probability and entropy
  logprob torch                   log_softmax + gather + entropy in torch float32, eager
  collect: library                observe + rollout_policy + a linear critic in torch + logprob_device + gae_device
  collect: torch forms            the same phase with the two torch forms instead (eager), and from a torch.cuda.graph
  k_gae DxW                       cz_gae_device under CZ_GAE_SHAPE=DxW: D rows loaded ahead, W threads per workgroup

    python3 tools/targets_sizes.py                          # -> profiles/r30/targets_sizes.txt
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r30", "targets_sizes.txt"), timeout=900)
ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--T", type=int, nargs="+", default=[32, 128])
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--shapes", nargs="*", default=[f"{d}x{w}" for w in (64, 256) for d in (2, 4, 8, 16)])
A = measure.A
GAMMA, LAM = 0.99, 0.95


def torch_gae(torch, r, done, V32, adv, ret):
    V = V32.double()
    zero = torch.zeros_like(r[0])
    acc = torch.zeros_like(r[0])
    for t in range(r.shape[0] - 1, -1, -1):
        d = (r[t] + torch.where(done[t], zero, GAMMA * V[t + 1])) - V[t]
        acc = d + torch.where(done[t], zero, (GAMMA * LAM) * acc)
        adv[t] = acc.float()
        ret[t] = (acc + V[t]).float()


def torch_logprob(torch, logits, actions, logp, ent):
    ls = torch.log_softmax(logits, dim=-1)
    torch.Tensor.copy_(logp, ls.gather(-1, actions.long()[..., None])[..., 0])
    torch.Tensor.copy_(ent, -(ls.exp() * ls).sum(-1))


def legs(args, report):
    torch = measure.torch_first()
    K = args.launches
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)

    def timed(name, n, body, note, k=K):
        measure.times(body, 2)()
        side.synchronize()
        return report.row(name, n, "call", measure.torch_events(measure.times(body, k), k, args.reps), note)

    def graphed(name, n, body, note, k=K):
        body(0)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            body(0)
        timed(name, n, lambda i: g.replay(), note, k)
        del g

    for n in args.envs:
        env = measure.make_env(n, max_steps=100)
        F, Cn = env.F, env.num_actions
        torch.manual_seed(0)
        module = torch.nn.Sequential(torch.nn.Linear(F, 64), torch.nn.ReLU(), torch.nn.Linear(64, Cn)).to(dev)
        critic = torch.nn.Linear(F, 1).to(dev)
        with torch.cuda.stream(side):
            env.set_stream(torch.cuda.current_stream())
            env.load_policy(module[0].weight, module[0].bias, module[2].weight, module[2].bias)
            for T in args.T:
                note = f"T={T} K={K}"
                obs = torch.zeros((T + 1, n, A, F), dtype=torch.float32, device=dev)
                act = torch.zeros((T, n, A), dtype=torch.int32, device=dev)
                logits = torch.zeros((T, n, A, Cn), dtype=torch.float32, device=dev)
                rew = torch.zeros((T, n, A), dtype=torch.float64, device=dev)
                term, trunc = (torch.zeros((T, n, A), dtype=torch.uint8, device=dev) for _ in range(2))
                val = torch.zeros((T + 1, n, A), dtype=torch.float32, device=dev)
                logp, ent, adv, ret = (torch.zeros((T, n, A), dtype=torch.float32, device=dev) for _ in range(4))

                def rollout(i):
                    env.observe_device(d_obs32=obs[0])
                    env.rollout_policy(T, obs[1:], act, logits, rew, term, trunc, sets=(0, 0), mode="sample", seed=1, step0=i * T)
                    with torch.no_grad():
                        torch.Tensor.copy_(val, critic(obs)[..., 0])

                def lib_targets(i):
                    env.logprob_device(logits, act, logp, ent, sets=(0, 0), rows=T * n)
                    env.gae_device(T, rew, term, trunc, val, adv, ret, gamma=GAMMA, lam=LAM)

                def torch_targets(i):
                    with torch.no_grad():
                        torch_logprob(torch, logits, act, logp, ent)
                        torch_gae(torch, rew, (term | trunc) != 0, val, adv, ret)

                rollout(0)                                             # a real trajectory under every leg below
                side.synchronize()
                timed("gae_device", n, lambda i: env.gae_device(T, rew, term, trunc, val, adv, ret, gamma=GAMMA, lam=LAM), note)
                with torch.no_grad():
                    gae_loop = lambda i: torch_gae(torch, rew, (term | trunc) != 0, val, adv, ret)
                    timed("gae torch loop", n, gae_loop, note, 2)
                    graphed("gae torch loop from a graph", n, gae_loop, note, 2)
                    timed("logprob_device", n, lambda i: env.logprob_device(logits, act, logp, ent, sets=(0, 0), rows=T * n), note)
                    timed("logprob torch", n, lambda i: torch_logprob(torch, logits, act, logp, ent), note)
                timed("collect: rollout_policy + critic alone", n, rollout, note, 2)
                timed("collect: library", n, lambda i: (rollout(i), lib_targets(i)), note, 2)
                timed("collect: torch forms", n, lambda i: (rollout(i), torch_targets(i)), note, 2)
                graphed("collect: torch forms from a graph", n, lambda i: (rollout(i), torch_targets(i)), note, 2)
                graphed("collect: library from a graph", n, lambda i: (rollout(i), lib_targets(i)), note, 2)
                del obs, logits
            side.synchronize()
        env.set_stream(None)
        env.close()

    # the k_gae instances: a small handle each (CZ_GAE_SHAPE is read when a handle is made), the extents are the caller's
    with torch.cuda.stream(side):
        for n in args.envs:
            for T in args.T:
                rew = torch.randn((T, n, A), dtype=torch.float64, device=dev)
                term = (torch.rand((T, n, A), device=dev) < 0.04).to(torch.uint8)
                trunc = (torch.rand((T, n, A), device=dev) < 0.04).to(torch.uint8)
                val = torch.randn((T + 1, n, A), dtype=torch.float32, device=dev)
                adv, ret = (torch.zeros((T, n, A), dtype=torch.float32, device=dev) for _ in range(2))
                for shape in args.shapes:
                    os.environ["CZ_GAE_SHAPE"] = shape
                    env = measure.make_env(64)
                    env.set_stream(torch.cuda.current_stream())
                    timed(f"k_gae {shape}", n, lambda i: env.gae_device(T, rew, term, trunc, val, adv, ret, gamma=GAMMA, lam=LAM, env_count=n),
                          f"T={T} K={K}")
                    side.synchronize()
                    env.set_stream(None)
                    env.close()
                os.environ.pop("CZ_GAE_SHAPE", None)


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
