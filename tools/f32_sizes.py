#!/usr/bin/env python3
"""Launch time of the one-step kernel by observation form (float64 rows: cz::k_step<..., STEP> / k_step_lean; float32 rows:
cz::k_step<..., STEP_F32>), batch size and store flavour (CZ_WT), config 2's shape (coop_test, 2 agents, scheme3, F = 278).
HIP events around K launches of a ring run (graph replay, graphs built before the timed region), `--reps` timed runs per size: every
run's figure is printed, so that the run-to-run spread can be read off.  The float64 form needs nothing of the float32 API, so the
same file measures an older checkout (run it with that checkout's package on PYTHONPATH).

    python3 tools/f32_sizes.py --form f64 --reps 5 512 2048 4096 8192 16384 32768 65536 131072
    python3 tools/f32_sizes.py --form f32 --wt 0 --wt 1 --wt 2 8192 12288 24576        # the CZ_WT sweep for float32 rows
    python3 tools/f32_sizes.py --closed-loop 4096 32768                                  # torch: [step, .float()] against [step_f32]
"""
import argparse
import ctypes as C
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--form", choices=["f64", "f32"], default="f32")
ap.add_argument("--wt", action="append", choices=["auto", "0", "1", "2"])
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default="")
ap.add_argument("--closed-loop", action="store_true")
ap.add_argument("sizes", type=int, nargs="+")
args = ap.parse_args()
if args.closed_loop:
    import torch                                  # first: its bundled HIP runtime then serves the step library too
    torch.cuda.init()
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cooking_zoo_amd import _native  # noqa: E402
from cooking_zoo_amd.vec_env import CookingVecEnv  # noqa: E402

A, RECIPES, P = 2, ["TomatoLettuceSalad", "CarrotBanana"], 16


def make(n):
    env = CookingVecEnv(n, "coop_test", "example", A, 400, RECIPES, action_scheme="scheme3", num_layouts=64, auto_reset=True)
    env.reset(return_obs=False)
    return env


def sweep():
    L = _native.lib()
    for n in args.sizes:
        for wt in args.wt or ["auto"]:
            if wt == "auto":
                os.environ.pop("CZ_WT", None)
            else:
                os.environ["CZ_WT"] = wt
            env = make(n)
            d_act = env.alloc((P, n, A), np.int32)
            d_act.from_host(np.random.default_rng(0).integers(0, 5, size=(P, n, A), dtype=np.int32))
            outs = [env.alloc((n, A), np.float64).ptr, env.alloc((n, A), np.uint8).ptr, env.alloc((n, A), np.uint8).ptr]
            if args.form == "f32":
                env.set_f32_output(env.alloc((n, A, env.F), np.float32))
                d_obs = None
            else:
                d_obs = env.alloc((n, A, env.F), np.float64).ptr
            K = args.steps
            run = lambda: _native.check(env._h, L.cz_step_device_ring(env._h, K, d_act.ptr, n * A, P, 0, d_obs, *outs))
            run()                                                             # builds the graphs, warms everything
            env.sync()
            us = []
            for _ in range(args.reps):
                ms = C.c_float()
                L.cz_timer_start(env._h)
                run()
                L.cz_timer_stop(env._h, C.byref(ms))
                us.append(ms.value * 1e3 / K)
            mib = n * A * env.F * (4 if args.form == "f32" else 8) / (1 << 20)
            env.close()
            print(f"{args.label or args.form:12s} {args.form} wt={wt:4s} {n:7d} envs ({mib:7.1f} MiB obs/launch) K={K}: us per launch  "
                  f"min {min(us):8.3f}  median {sorted(us)[len(us) // 2]:8.3f}  max {max(us):8.3f}   runs " + " ".join(f"{u:.3f}" for u in us), flush=True)


def closed_loop():
    """what a torch training loop pays per step for a float32 observation: float64 rows + .float(), against float32 rows"""
    dev = torch.device("cuda", 0)
    K = args.steps
    for n in args.sizes:
        res = {}
        for form in ("f64+float()", "f32"):
            env = make(n)
            acts = torch.randint(0, 5, (P, n, A), dtype=torch.int32, device=dev)
            rew = torch.empty((n, A), dtype=torch.float64, device=dev)
            term, trunc = (torch.empty((n, A), dtype=torch.uint8, device=dev) for _ in range(2))
            obs64 = torch.empty((n, A, env.F), dtype=torch.float64, device=dev)
            obs32 = torch.empty((n, A, env.F), dtype=torch.float32, device=dev)
            side = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(side):
                env.set_stream(torch.cuda.current_stream())

                def loop(k):
                    for t in range(k):
                        if form == "f32":
                            env.step_device_f32(acts[t % P], obs32, rew, term, trunc)
                        else:
                            env.step_device(acts[t % P], obs64, rew, term, trunc)
                            torch.Tensor.copy_(obs32, obs64)                 # obs64.float() into the consumer's tensor
                loop(100)
                side.synchronize()
                us = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    loop(K)
                    e1.record()
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3 / K)
            env.set_stream(None)
            env.close()
            res[form] = us
            print(f"closed loop {form:12s} {n:7d} envs K={K} (eager launches from Python, one stream): us per step  min {min(us):8.3f}  "
                  f"median {sorted(us)[len(us) // 2]:8.3f}  max {max(us):8.3f}   runs " + " ".join(f"{u:.3f}" for u in us), flush=True)


if __name__ == "__main__":
    closed_loop() if args.closed_loop else sweep()
