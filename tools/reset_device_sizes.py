#!/usr/bin/env python3
"""What `reset_device` (cz_reset_device) costs, timed with device events on the handle's stream (config 2's shape: coop_test, 2 agents,
scheme3, F = 278; 4096 envs by default):

  one call      K calls of reset_device between two events, with a mask that chooses 0 %, 1 %, 10 % and 100 % of the envs (the same envs
                in every call: a chosen env is restarted whatever its state, so every call does the same work), without output rows and
                with float32 rows; next to each the one-step launch of the same handle (step_device with float64 rows /
                step_device_f32), K launches between two events, every env alive
  loop          the loop step_device_f32 + reset_device() (no mask: the finished envs; float32 rows) on a handle with auto_reset off,
                against step_device_f32 alone on a handle with auto_reset on, both over the same action buffer and with short episodes
                (--max-steps), per launch and per LIVE env-step: the env-steps counted by cz_get_stats, which leave reset passes out

Writes every line to --out (default profiles/r15/reset_device.txt).  Needs a GPU; nothing is estimated without one.

    python3 tools/reset_device_sizes.py
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r15", "reset_device.txt"))
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--max-steps", type=int, default=50, help="episode length of the loop legs")
A = measure.A


def buffers(env):
    import numpy as np
    b = measure.step_buffers(env, 8, 1, ("obs", "obs32", "rew", "term", "trunc"))
    b["mask"] = env.alloc((env.num_envs,), np.uint8)
    return b


def one_call(args, report):
    import numpy as np
    env = measure.make_env(args.envs, auto_reset=False)
    n, b, K = env.num_envs, buffers(env), args.launches
    act = lambda k: b["act"].ptr + (k % 8) * n * A * 4
    ones = np.ones(n, dtype=np.uint8)

    def everybody():                  # every env alive and young: the step legs never meet a frozen env
        b["mask"].from_host(ones)
        env.reset_device(b["mask"])

    for rows, step in (("no rows", lambda k: env.step_device(act(k), b["obs"], b["rew"], b["term"], b["trunc"])),
                       ("float32 rows", lambda k: env.step_device_f32(act(k), b["obs32"], b["rew"], b["term"], b["trunc"]))):
        report.row(f"one step ({'float64 rows' if rows == 'no rows' else rows})", n, "launch",
                   measure.handle_events(env, measure.times(step, K), K, args.reps, everybody, warm=args.reps))
        for percent in (0, 1, 10, 100):
            mask = np.zeros(n, dtype=np.uint8)
            mask[np.random.default_rng(2).permutation(n)[:n * percent // 100]] = 1
            call = lambda k: env.reset_device(b["mask"], None, None, b["obs32"] if rows == "float32 rows" else None)
            b["mask"].from_host(mask)
            report.row(f"reset_device {rows} {percent} % chosen ({int(mask.sum())})", n, "call",
                       measure.handle_events(env, measure.times(call, K), K, args.reps, warm=args.reps))
    env.close()


def loop(args, report):
    K = args.launches
    for name, auto in (("step_device_f32 + reset_device(), auto_reset off", False), ("step_device_f32 alone, auto_reset on", True)):
        env = measure.make_env(args.envs, args.max_steps, auto_reset=auto)
        n, b = env.num_envs, buffers(env)

        def it(k):
            env.step_device_f32(b["act"].ptr + (k % 8) * n * A * 4, b["obs32"], b["rew"], b["term"], b["trunc"])
            if not auto:
                env.reset_device(None, None, None, b["obs32"])

        measure.handle_events(env, measure.times(it, K), K, args.reps)               # warm-up: one whole pass, dropped
        env.sync()
        s0 = env.stats()["env_steps"]
        us = measure.handle_events(env, measure.times(it, K), K, args.reps)
        live, steps = env.stats()["env_steps"] - s0, K * args.reps
        total_us = measure.median(us) * steps                  # (median region time x regions: the regions are alike)
        report.row(f"loop: {name}", n, "iteration", us, f"episodes of {args.max_steps}; {live} live env-steps in {steps} iterations "
                   f"({live / (steps * n):.4f} per env and iteration), {total_us * 1e3 / live:.4f} ns per live env-step")
        env.close()


def legs(args, report):
    one_call(args, report)
    loop(args, report)


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
