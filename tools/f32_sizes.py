#!/usr/bin/env python3
"""Launch time of the one-step kernel by observation form (float64 rows: cz::k_step<..., STEP> / k_step_lean; float32 rows:
cz::k_step<..., STEP_F32>), batch size and store flavour (CZ_WT), config 2's shape (coop_test, 2 agents, scheme3, F = 278).
HIP events around K launches of a ring run (graph replay, graphs built before the timed region), `--reps` timed runs per size: every
run's figure is printed, so that the run-to-run spread can be read off.  The float64 form needs nothing of the float32 API, so the
same file measures an older checkout (`--tree`).

    python3 tools/f32_sizes.py --form f64 --reps 5 512 2048 4096 8192 16384 32768 65536 131072
    python3 tools/f32_sizes.py --form f32 --wt 0 --wt 1 --wt 2 8192 12288 24576        # the CZ_WT sweep for float32 rows
    python3 tools/f32_sizes.py --closed-loop 4096 32768                                  # torch: [step, .float()] against [step_f32]
"""
import os

import measure

ap = measure.parser(__doc__, reps=5)
ap.add_argument("--form", choices=["f64", "f32"], default="f32")
ap.add_argument("--wt", action="append", choices=["auto", "0", "1", "2"])
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--closed-loop", action="store_true")
ap.add_argument("sizes", type=int, nargs="+")
A, P = measure.A, 16


def sweep(args, report):
    K = args.steps
    for n in args.sizes:
        for wt in args.wt or ["auto"]:
            if wt == "auto":
                os.environ.pop("CZ_WT", None)
            else:
                os.environ["CZ_WT"] = wt
            env = measure.make_env(n)
            b = measure.step_buffers(env, P, 0, ("rew", "term", "trunc", "obs32" if args.form == "f32" else "obs"))
            if args.form == "f32":
                env.set_f32_output(b["obs32"])
            run = lambda: env.step_device_ring(K, b["act"], n * A, P, 0, b.get("obs"), b["rew"], b["term"], b["trunc"])
            run()                                                             # builds the graphs, warms everything
            env.sync()
            us = measure.handle_events(env, run, K, args.reps)
            mib = n * A * env.F * (4 if args.form == "f32" else 8) / (1 << 20)
            env.close()
            report.row(f"{args.form} wt={wt}", n, "launch", us, f"{mib:.1f} MiB obs/launch, K={K}")


def closed_loop(args, report):
    """what a torch training loop pays per step for a float32 observation: float64 rows + .float(), against float32 rows"""
    import torch
    dev, K = torch.device("cuda", 0), args.steps
    for n in args.sizes:
        for form in ("f64+float()", "f32"):
            env = measure.make_env(n)
            acts = torch.randint(0, 5, (P, n, A), dtype=torch.int32, device=dev)
            rew = torch.empty((n, A), dtype=torch.float64, device=dev)
            term, trunc = (torch.empty((n, A), dtype=torch.uint8, device=dev) for _ in range(2))
            obs64 = torch.empty((n, A, env.F), dtype=torch.float64, device=dev)
            obs32 = torch.empty((n, A, env.F), dtype=torch.float32, device=dev)

            def step(t):
                if form == "f32":
                    env.step_device_f32(acts[t % P], obs32, rew, term, trunc)
                else:
                    env.step_device(acts[t % P], obs64, rew, term, trunc)
                    torch.Tensor.copy_(obs32, obs64)                 # obs64.float() into the consumer's tensor

            side = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(side):
                env.set_stream(torch.cuda.current_stream())
                measure.times(step, 100)()
                side.synchronize()
                us = measure.torch_events(measure.times(step, K), K, args.reps)
            env.set_stream(None)
            env.close()
            report.row(f"closed loop {form} (eager launches from Python, one stream)", n, "step", us, f"K={K}")


def legs(args, report):
    if args.closed_loop:
        measure.torch_first()
    (closed_loop if args.closed_loop else sweep)(args, report)


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
