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

One process measures one library (`--lib`, default: this tree's).  `--alternate OTHER_LIB` is the driver: it runs fresh child
processes, OTHER and this tree's library alternately, `--pairs` times, then once more with the order inside the pair reversed, and
writes every line plus a summary (per leg and library: every run's median, and the spread between the runs of the same library) to
`--out` (default profiles/r14/rollout_f32.txt).

    python3 tools/rollout_f32_sizes.py --alternate /path/to/the/parent/libcookingzoo_hip.so
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(REPO, "cooking_zoo_amd", "csrc", "libcookingzoo_hip.so"))
ap.add_argument("--label", default="change")
ap.add_argument("--alternate", metavar="OTHER_LIB")
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r14", "rollout_f32.txt"))
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--T", type=int, default=32)
ap.add_argument("--launches", type=int, default=40)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
A, RECIPES = 2, ["TomatoLettuceSalad", "CarrotBanana"]
LEGS = ["rollout f64", "rollout_actions f64", "rollout codes", "f64 + convert", "codes + gather", "rollout_f32", "rollout_actions_f32"]


def measure():
    os.environ["CZ_LIB"] = args.lib
    import torch                                  # first: its bundled HIP runtime then serves the step library too
    torch.cuda.init()
    sys.path.insert(0, REPO)
    from cooking_zoo_amd.vec_env import CookingVecEnv
    has_f32 = hasattr(C.CDLL(args.lib), "cz_rollout_f32")
    n, T, K = args.envs, args.T, args.launches
    dev = torch.device("cuda", 0)
    env = CookingVecEnv(n, "coop_test", "example", A, 400, RECIPES, action_scheme="scheme3", num_layouts=64, auto_reset=True)
    env.reset(return_obs=False)
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

    legs = {
        "rollout f64": lambda k: env.rollout(T, 1, k * T, obs64, rew, term, trunc),
        "rollout_actions f64": lambda k: env.rollout_actions(acts, T, obs64, rew, term, trunc),
        "rollout codes": lambda k: env.rollout_compact(T, 1, k * T, codes, None, rew, term, trunc),
        "f64 + convert": lambda k: (env.rollout(T, 1, k * T, obs64, rew, term, trunc), torch.Tensor.copy_(obs32, obs64)),
        "codes + gather": lambda k: (env.rollout_compact(T, 1, k * T, codes, None, rew, term, trunc), gather()),
    }
    if has_f32:
        legs["rollout_f32"] = lambda k: env.rollout_f32(T, 1, k * T, obs32, rew, term, trunc)
        legs["rollout_actions_f32"] = lambda k: env.rollout_actions_f32(acts, T, obs32, rew, term, trunc)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        for name in LEGS:
            if name not in legs:
                continue
            for k in range(4):
                legs[name](k)
            side.synchronize()
            us = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(K):
                    legs[name](k)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / (K * T))
            print(f"{args.label:7s} {name:20s} {n} envs T={T} K={K}: us per step  min {min(us):7.3f}  median {sorted(us)[len(us) // 2]:7.3f}  "
                  f"max {max(us):7.3f}   runs " + " ".join(f"{u:.3f}" for u in us), flush=True)
        side.synchronize()
    env.set_stream(None)
    env.close()


def alternate():
    order = [("parent", args.alternate), ("change", args.lib)]
    runs = order * args.pairs + order[::-1]
    lines, medians = [], {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for i, (label, lib) in enumerate(runs):
        cmd = [sys.executable, os.path.abspath(__file__), "--lib", lib, "--label", label, "--envs", str(args.envs), "--T", str(args.T),
               "--launches", str(args.launches), "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        lines.append(f"# run {i}: {label}")
        lines += p.stdout.rstrip().split("\n")
        if p.returncode != 0:
            lines.append(f"# run {i} ended with status {p.returncode}: nothing more is started\n{p.stderr[-2000:]}")
            break
        for l in p.stdout.split("\n"):
            for leg in LEGS:
                if l.startswith(f"{label:7s} {leg:20s} "):
                    medians.setdefault((leg, label), []).append(float(l.split("median")[1].split()[0]))
    lines.append("# summary: medians of the runs, in run order, and the spread (max - min) between the runs of the same library")
    for leg in LEGS:
        for label in ("parent", "change"):
            m = medians.get((leg, label))
            if m:
                lines.append(f"{leg:20s} {label:7s} " + " ".join(f"{x:.3f}" for x in m) + f"   spread {max(m) - min(m):.3f}  mean {sum(m) / len(m):.3f}")
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if len(medians) else 1


if __name__ == "__main__":
    sys.exit(alternate()) if args.alternate else measure()
