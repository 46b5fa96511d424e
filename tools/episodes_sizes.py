#!/usr/bin/env python3
"""What the per-env episode records cost (config 2's shape: coop_test, 2 agents, scheme3, F = 278), timed with the handle's own device
events (cz_timer_start / cz_timer_stop) on its stream:

  step lean / step generic   one-step launches of k_step_lean<1,1,2,3> and, in a handle made under CZ_LEAN=0, k_step<1,1,2,3,0>:
                             --launches of them between two events, us per launch; max_steps = 400, so nearly every wave takes the
                             common path - the path this measurement is about
  collect all / dense        ONE collect_episodes call between two events - every output, or the dense arrays alone (one kernel
                             instead of two) - with 0 %, 1 % and 100 % of the envs found, next to ONE step launch timed the same way (`one step ... launch`).
                             A handle with auto_reset off and max_steps = 2 is armed for each call: reset_device restarts the chosen
                             envs (all, or every hundredth) and two steps finish them, while the others stay frozen.

One process measures one checkout (`--tree`, default: this one; package and built library are taken from it, so a
library goes with the package it was built for; the collect legs need the entry point).  `--alternate OTHER_TREE` is the driver: fresh child
processes, OTHER's library and this tree's alternately, `--pairs` times, then once more with the order inside the pair reversed;
every line and a summary (per step leg and library every run's median, the spread between runs of the same library and the
difference of the means) go to `--out` (default profiles/r16/episodes_sizes.txt).

    python3 tools/episodes_sizes.py --alternate /path/to/a/built/checkout/of/the/parent
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=REPO)
ap.add_argument("--label", default="change")
ap.add_argument("--alternate", metavar="OTHER_TREE")
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r16", "episodes_sizes.txt"))
ap.add_argument("--sizes", default="4096,65536")
ap.add_argument("--launches", type=int, default=400)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
A, RECIPES = 2, ["TomatoLettuceSalad", "CarrotBanana"]


def report(label, leg, n, us, what):
    print(f"{label:7s} {leg:26s} {n:6d} envs: us per {what}  min {min(us):8.3f}  median {sorted(us)[len(us) // 2]:8.3f}  max {max(us):8.3f}   runs "
          + " ".join(f"{u:.3f}" for u in us), flush=True)


def measure():
    os.environ.pop("CZ_LIB", None)
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    from cooking_zoo_amd import _native
    from cooking_zoo_amd.vec_env import CookingVecEnv
    L = _native.lib()
    has_collect = hasattr(C.CDLL(_native.LIB_PATH), "cz_episodes_collect")

    def timed(env, fn):
        ms = C.c_float()
        _native.check(env._h, L.cz_timer_start(env._h))
        fn()
        _native.check(env._h, L.cz_timer_stop(env._h, C.byref(ms)))
        return ms.value * 1e3

    def step_bufs(env, n, obs=True):
        b = dict(act=env.alloc((n, A), np.int32), rew=env.alloc((n, A), np.float64), term=env.alloc((n, A), np.uint8),
                 trunc=env.alloc((n, A), np.uint8), obs=env.alloc((n, A, env.F), np.float64) if obs else None)
        b["act"].from_host(np.random.default_rng(1).integers(0, env.n_actions, (n, A)).astype(np.int32))
        return b

    for n in [int(s) for s in args.sizes.split(",")]:
        # ---- the one-step launches, common path
        for leg, lean in (("step lean", "1"), ("step generic", "0")):
            os.environ["CZ_LEAN"] = lean
            env = CookingVecEnv(n, "coop_test", "example", A, 400, RECIPES, action_scheme="scheme3", num_layouts=64, auto_reset=True)
            os.environ.pop("CZ_LEAN")
            env.reset(return_obs=False)
            b = step_bufs(env, n)
            one = lambda: env.step_device(b["act"], b["obs"], b["rew"], b["term"], b["trunc"])
            for _ in range(20):
                one()
            env.sync()
            K = args.launches
            report(args.label, leg, n, [timed(env, lambda: [one() for _ in range(K)]) / K for _ in range(args.reps)], "launch")
            report(args.label, f"one {leg} launch", n, [timed(env, one) for _ in range(args.reps)], "call")
            env.close()
        if not has_collect:
            continue
        # ---- one collect call, next to one step launch
        env = CookingVecEnv(n, "coop_test", "example", A, 2, RECIPES, action_scheme="scheme3", num_layouts=64, auto_reset=False)
        env.reset(return_obs=False)
        b = step_bufs(env, n)
        one = lambda: env.step_device(b["act"], b["obs"], b["rew"], b["term"], b["trunc"])
        mask, ret = env.alloc((n,), np.uint8), env.alloc((n, A), np.float64)
        length, flags = env.alloc((n,), np.int32), env.alloc((n,), np.uint32)
        lst, cnt = env.alloc((n,), _native.EPISODE_DTYPE), env.alloc((1,), np.int32)
        every100 = env.alloc((n,), np.uint8)
        every100.from_host((np.arange(n) % 100 == 0).astype(np.uint8))
        one(); one()                                        # everybody has finished and is frozen
        env.collect_episodes()
        nobody = object()
        for pct, chosen in ((0, nobody), (1, every100), (100, None)):
            for leg, call in (("collect all", lambda: env.collect_episodes(mask, ret, length, flags, lst, n, cnt)),
                              ("collect dense", lambda: env.collect_episodes(mask, ret, length, flags))):
                us, found = [], 0
                for _ in range(args.reps):
                    if chosen is not nobody:
                        env.reset_device(chosen)
                        one(); one()
                    env.sync()
                    us.append(timed(env, call))
                    found = int(mask.to_host().sum())
                report(args.label, f"{leg} {pct:3d} % ({found} found)", n, us, "call")
        env.close()


def alternate():
    order = [("parent", args.alternate), ("change", args.tree)]
    runs = order * args.pairs + order[::-1]
    lines, medians = [], {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for i, (label, lib) in enumerate(runs):
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", lib, "--label", label, "--sizes", args.sizes,
               "--launches", str(args.launches), "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        lines.append(f"# run {i}: {label}")
        lines += p.stdout.rstrip().split("\n")
        if p.returncode != 0:
            lines.append(f"# run {i} ended with status {p.returncode}: nothing more is started\n{p.stderr[-2000:]}")
            break
        for l in p.stdout.split("\n"):
            if l.startswith(f"{label:7s} step ") or l.startswith(f"{label:7s} one step "):
                key = (l[8:34].strip(), int(l[35:41]))
                medians.setdefault(key + (label,), []).append(float(l.split("median")[1].split()[0]))
    lines.append("# summary (step legs): medians of the runs, in run order; spread = max - min between the runs of the same library")
    for key in sorted({k[:2] for k in medians}):
        mean = {}
        for label in ("parent", "change"):
            m = medians.get(key + (label,))
            if m:
                mean[label] = sum(m) / len(m)
                lines.append(f"{key[0]:14s} {key[1]:6d} envs {label:7s} " + " ".join(f"{x:.3f}" for x in m) +
                             f"   spread {max(m) - min(m):.3f}  mean {mean[label]:.3f}")
        if len(mean) == 2:
            lines.append(f"{key[0]:14s} {key[1]:6d} envs change - parent (means): {mean['change'] - mean['parent']:+.3f} us")
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if len(medians) and not any("ended with status" in l for l in lines) else 1


if __name__ == "__main__":
    sys.exit(alternate()) if args.alternate else measure()
