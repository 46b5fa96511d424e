#!/usr/bin/env python3
"""What a float32 trajectory [T][N][A][F] costs per step, by the way it is made (config 2's shape: coop_test, 2 agents, scheme3,
F = 278; 4096 envs, T = 32 by default), timed with device events around K launches on one stream:

  rollout f64              cz_rollout with a float64 trajectory
  rollout_actions f64      cz_rollout_actions with a float64 trajectory
  rollout codes            cz_rollout_compact, codes only
  f64 + convert            cz_rollout, then obs32.copy_(obs64) (what `.float()` into the consumer's tensor costs)
  codes + gather           cz_rollout_compact, then table32[codes[..., :F].to(int32)] (torch indexes with int32 / int64 only, so the
                           pass widens the codes first) copied into the consumer's tensor
  rollout_f32              cz_rollout_f32                           } only where the library has the entry points
  rollout_actions_f32      cz_rollout_actions_f32                   }

One process measures one library (`--lib`, default: this tree's).  `--alternate OTHER_LIB` is the driver (tools/measure.py): it
runs fresh child processes, OTHER and this tree's library alternately, `--pairs` times, then once more with the order inside the
pair reversed, and writes every line plus the summary and the band rows to `--out` (default profiles/r14/rollout_f32.txt).

    python3 tools/rollout_f32_sizes.py --alternate /path/to/the/parent/libcookingzoo_hip.so
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r14", "rollout_f32.txt"), timeout=400)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--T", type=int, default=32)
ap.add_argument("--launches", type=int, default=40)
A = measure.A


def legs(args, report):
    torch = measure.torch_first()
    n, T, K = args.envs, args.T, args.launches
    dev = torch.device("cuda", 0)
    env = measure.make_env(n)
    F, Fp = env.F, env.codes_pitch
    obs64 = torch.empty((T, n, A, F), dtype=torch.float64, device=dev)
    obs32 = torch.empty((T, n, A, F), dtype=torch.float32, device=dev)
    codes = torch.empty((T, n, A, Fp), dtype=torch.uint8, device=dev)
    rew = torch.empty((T, n, A), dtype=torch.float64, device=dev)
    term, trunc = (torch.empty((T, n, A), dtype=torch.uint8, device=dev) for _ in range(2))
    acts = torch.randint(0, 5, (T, n, A), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    table32 = torch.from_numpy(env.obs_table_f32()).to(dev)

    def gather():
        torch.Tensor.copy_(obs32, table32[codes[..., :F].to(torch.int32)])

    todo = {
        "rollout f64": lambda k: env.rollout(T, 1, k * T, obs64, rew, term, trunc),
        "rollout_actions f64": lambda k: env.rollout_actions(acts, T, obs64, rew, term, trunc),
        "rollout codes": lambda k: env.rollout_compact(T, 1, k * T, codes, None, rew, term, trunc),
        "f64 + convert": lambda k: (env.rollout(T, 1, k * T, obs64, rew, term, trunc), torch.Tensor.copy_(obs32, obs64)),
        "codes + gather": lambda k: (env.rollout_compact(T, 1, k * T, codes, None, rew, term, trunc), gather()),
    }
    if measure.has_entry("cz_rollout_f32"):
        todo["rollout_f32"] = lambda k: env.rollout_f32(T, 1, k * T, obs32, rew, term, trunc)
        todo["rollout_actions_f32"] = lambda k: env.rollout_actions_f32(acts, T, obs32, rew, term, trunc)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        for name, leg in todo.items():
            measure.times(leg, 4)()
            side.synchronize()
            report.row(name, n, "step", measure.torch_events(measure.times(leg, K), K * T, args.reps), f"T={T} K={K}")
        side.synchronize()
    env.set_stream(None)
    env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
