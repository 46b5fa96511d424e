#!/usr/bin/env python3
"""What a policy-driven step costs, by the way the policy reaches the step (config 2's shape: coop_test, 2 agents, scheme3, F = 278;
4096 and 65 536 envs, T = 32), medians per step between device events on one stream.  The policy is the library's MLP
(cooking_zoo_amd/policy.py: Linear(F, 64), ReLU, Linear(64, 5)), both agents on set 0:

  rollout_policy greedy        cz_rollout_policy, one launch per T steps
  rollout_policy sample        the same with softmax sampling
  rollout_f32                  cz_rollout_f32: the same launch without the policy - the difference is the policy's own cost
  step_f32 + policy_device     the closed loop of two launches per step: cz_policy_device on the last rows, cz_step_device_f32
  ... from a graph             that loop, T steps captured once into a graph and replayed
  step_f32 + torch MLP graph   cz_step_device_f32 + the same network and argmax in torch, T steps from a torch.cuda.graph
  policy_device alone          cz_policy_device on fixed rows

    python3 tools/policy_sizes.py                          # -> profiles/r29/policy_sizes.txt
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r29", "policy_sizes.txt"), timeout=600)
ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--T", type=int, default=32)
ap.add_argument("--launches", type=int, default=10)
A = measure.A


def legs(args, report):
    torch = measure.torch_first()
    T, K = args.T, args.launches
    dev = torch.device("cuda", 0)
    for n in args.envs:
        env = measure.make_env(n)
        F, Cn = env.F, env.num_actions
        torch.manual_seed(0)
        module = torch.nn.Sequential(torch.nn.Linear(F, 64), torch.nn.ReLU(), torch.nn.Linear(64, Cn)).to(dev)
        obs32 = torch.empty((T, n, A, F), dtype=torch.float32, device=dev)
        rows = [torch.zeros((n, A, F), dtype=torch.float32, device=dev) for _ in range(2)]
        acts = torch.zeros((T, n, A), dtype=torch.int32, device=dev)
        act1 = torch.zeros((n, A), dtype=torch.int32, device=dev)
        rew = torch.empty((T, n, A), dtype=torch.float64, device=dev)
        term, trunc = (torch.empty((T, n, A), dtype=torch.uint8, device=dev) for _ in range(2))
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            env.set_stream(torch.cuda.current_stream())
            env.load_policy(module[0].weight, module[0].bias, module[2].weight, module[2].bias)
            env.observe_device(d_obs32=rows[0])

            def loop_step(i):
                env.policy_device(rows[i & 1], act1, sets=(0, 0), mode="greedy")
                env.step_device_f32(act1, rows[(i + 1) & 1], rew[0], term[0], trunc[0])

            def torch_step(i):
                with torch.no_grad():
                    torch.Tensor.copy_(act1, module(rows[i & 1]).argmax(-1))
                env.step_device_f32(act1, rows[(i + 1) & 1], rew[0], term[0], trunc[0])

            todo = {
                "rollout_policy greedy": (lambda k: env.rollout_policy(T, obs32, acts, None, rew, term, trunc, sets=(0, 0), mode="greedy", step0=k * T), T),
                "rollout_policy sample": (lambda k: env.rollout_policy(T, obs32, acts, None, rew, term, trunc, sets=(0, 0), mode="sample", seed=1,
                                                                       step0=k * T), T),
                "rollout_f32": (lambda k: env.rollout_f32(T, 1, k * T, obs32, rew, term, trunc), T),
                "step_f32 + policy_device": (lambda k: measure.times(loop_step, T)(), T),
                "policy_device alone": (lambda k: env.policy_device(rows[0], act1, sets=(0, 0), mode="greedy"), 1),
            }
            for name, (leg, units) in todo.items():
                measure.times(leg, 2)()
                side.synchronize()
                report.row(name, n, "step", measure.torch_events(measure.times(leg, K), K * units, args.reps), f"T={T} K={K}")
            for name, step in (("step_f32 + policy_device from a graph", loop_step), ("step_f32 + torch MLP graph", torch_step)):
                measure.times(step, 2)()                      # (T is even: the rows end where they began, a replay goes on from there)
                side.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    measure.times(step, T)()
                report.row(name, n, "step", measure.torch_events(measure.times(lambda k: g.replay(), K), K * T, args.reps), f"T={T} K={K}")
                del g
            side.synchronize()
        env.set_stream(None)
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
