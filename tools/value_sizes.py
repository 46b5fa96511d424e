#!/usr/bin/env python3
"""What the critic on the device costs (cz_rollout_policy_value, cz_value_device; cooking_zoo_amd/policy.py step 3b) next to the
launch without it and next to a torch critic of the same architecture, at config 2's shape (coop_test, 2 agents, scheme3, F = 278,
5 actions), 4096 and 65 536 envs, T = 32 and 128; medians per call between device events on one stream:

  rollout_policy                  cz_rollout_policy, two policy agents on set 0, "sample"          (parent and change)
  rollout + values, shared trunk  cz_rollout_policy_value with vsets == sets: one more output row per agent and step
  rollout + values, own critic    ... with vsets = (1, 1): a second hidden pass per agent and step
  value_device                    cz_value_device over the whole trajectory, (T + 1) * n rows in one launch
  collect: device critic          observe + rollout with values (shared / own critic) + logprob_device + gae_device: four calls
  collect: torch critic           observe + rollout_policy + Sequential(Linear(F, 64), ReLU(), Linear(64, 1)) in torch over the
                                  [T + 1, n, A, F] trajectory + logprob_device + gae_device                (parent and change)
  ... from a graph                the same phase captured once into a torch.cuda.graph and replayed

Rows that need an entry point the measured library lacks are left out (the parent of this change has no value heads).

    python3 tools/value_sizes.py --alternate PARENT          # -> profiles/r32/value_sizes.txt
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r32", "value_sizes.txt"), timeout=900)
ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--T", type=int, nargs="+", default=[32, 128])
ap.add_argument("--launches", type=int, default=2)
A = measure.A
GAMMA, LAM = 0.99, 0.95


def legs(args, report):
    torch = measure.torch_first()
    K = args.launches
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    with_values = measure.has_entry("cz_rollout_policy_value")

    def timed(name, n, body, note, k=K):
        measure.times(body, 2)()
        side.synchronize()
        # (T is part of the row's name: the driver's summary pairs rows by name and env count)
        return report.row(f"{name}, {note.split()[0]}", n, "call", measure.torch_events(measure.times(body, k), k, args.reps), note)

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
        trunks = [torch.nn.Sequential(torch.nn.Linear(F, 64), torch.nn.ReLU()).to(dev) for _ in range(2)]
        actors = [torch.nn.Linear(64, Cn).to(dev) for _ in range(2)]
        heads = [torch.nn.Linear(64, 1).to(dev) for _ in range(2)]
        critic = torch.nn.Sequential(trunks[1][0], trunks[1][1], heads[1])         # the torch critic: the network of set 1
        stack = lambda ps: torch.stack([p.detach() for p in ps]).contiguous()
        with torch.cuda.stream(side):
            env.set_stream(torch.cuda.current_stream())
            env.load_policy(stack([t[0].weight for t in trunks]), stack([t[0].bias for t in trunks]), stack([a.weight for a in actors]),
                            stack([a.bias for a in actors]))
            if with_values:
                env.load_value(stack([h.weight for h in heads]), stack([h.bias for h in heads]))
            for T in args.T:
                note = f"T={T} K={K}"
                obs = torch.zeros((T + 1, n, A, F), dtype=torch.float32, device=dev)
                act = torch.zeros((T, n, A), dtype=torch.int32, device=dev)
                logits = torch.zeros((T, n, A, Cn), dtype=torch.float32, device=dev)
                rew = torch.zeros((T, n, A), dtype=torch.float64, device=dev)
                term, trunc = (torch.zeros((T, n, A), dtype=torch.uint8, device=dev) for _ in range(2))
                val = torch.zeros((T + 1, n, A), dtype=torch.float32, device=dev)
                logp, ent, adv, ret = (torch.zeros((T, n, A), dtype=torch.float32, device=dev) for _ in range(4))
                sets = (0, 0)

                def rollout(i):
                    env.rollout_policy(T, obs[1:], act, logits, rew, term, trunc, sets=sets, mode="sample", seed=1, step0=i * T)

                def rollout_values(vsets):
                    return lambda i: env.rollout_policy_value(T, obs[1:], val, act, logits, rew, term, trunc, sets=sets, vsets=vsets, mode="sample",
                                                              seed=1, step0=i * T)

                def targets(i):
                    env.logprob_device(logits, act, logp, ent, sets=sets, rows=T * n)
                    env.gae_device(T, rew, term, trunc, val, adv, ret, gamma=GAMMA, lam=LAM)

                def collect_device(vsets):
                    launch = rollout_values(vsets)
                    return lambda i: (env.observe_device(d_obs32=obs[0]), launch(i), targets(i))

                def collect_torch(i):
                    env.observe_device(d_obs32=obs[0])
                    rollout(i)
                    with torch.no_grad():
                        torch.Tensor.copy_(val, critic(obs)[..., 0])
                    targets(i)

                timed("rollout_policy", n, rollout, note)
                if with_values:
                    timed("rollout + values, shared trunk", n, rollout_values((0, 0)), note)
                    timed("rollout + values, own critic", n, rollout_values((1, 1)), note)
                    timed("value_device", n, lambda i: env.value_device(obs, val, vsets=(1, 1), rows=(T + 1) * n), note)
                    timed("collect: device critic, shared trunk", n, collect_device((0, 0)), note)
                    timed("collect: device critic, own critic", n, collect_device((1, 1)), note)
                    graphed("collect: device critic, own critic, from a graph", n, collect_device((1, 1)), note)
                timed("collect: torch critic", n, collect_torch, note)
                graphed("collect: torch critic from a graph", n, collect_torch, note)
                del obs, logits
            side.synchronize()
        env.set_stream(None)
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
