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
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r15", "reset_device.txt"))
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--max-steps", type=int, default=50, help="episode length of the loop legs")
args = ap.parse_args()
A, RECIPES = 2, ["TomatoLettuceSalad", "CarrotBanana"]
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(env, fn, before=None):
    """us per call of fn over --launches calls, --reps times: (min, median, max)"""
    from cooking_zoo_amd import _native
    L, us, ms = _native.lib(), [], C.c_float()
    for _ in range(args.reps):
        if before:
            before()
        _native.check(env._h, L.cz_timer_start(env._h))
        for k in range(args.launches):
            fn(k)
        _native.check(env._h, L.cz_timer_stop(env._h, C.byref(ms)))
        us.append(ms.value * 1e3 / args.launches)
    us.sort()
    return us[0], us[len(us) // 2], us[-1]


def make(max_steps, auto_reset):
    from cooking_zoo_amd.vec_env import CookingVecEnv
    env = CookingVecEnv(args.envs, "coop_test", "example", A, max_steps, RECIPES, action_scheme="scheme3", num_layouts=64, auto_reset=auto_reset)
    env.reset(return_obs=False)
    return env


def buffers(env):
    import numpy as np
    n, F = env.num_envs, env.F
    b = dict(act=env.alloc((8, n, A), np.int32), obs=env.alloc((n, A, F), np.float64), obs32=env.alloc((n, A, F), np.float32),
             rew=env.alloc((n, A), np.float64), term=env.alloc((n, A), np.uint8), trunc=env.alloc((n, A), np.uint8), mask=env.alloc((n,), np.uint8))
    b["act"].from_host(np.random.default_rng(1).integers(0, 5, size=(8, n, A), dtype=np.int32))
    return b


def one_call():
    import numpy as np
    env = make(400, False)
    n, b = env.num_envs, buffers(env)
    act = lambda k: b["act"].ptr + (k % 8) * n * A * 4
    ones = np.ones(n, dtype=np.uint8)

    def everybody():                  # every env alive and young: the step legs never meet a frozen env
        b["mask"].from_host(ones)
        env.reset_device(b["mask"])

    for rows, step in (("no rows", lambda k: env.step_device(act(k), b["obs"], b["rew"], b["term"], b["trunc"])),
                       ("float32 rows", lambda k: env.step_device_f32(act(k), b["obs32"], b["rew"], b["term"], b["trunc"]))):
        timed(env, step, everybody)                                                    # warm-up of the leg's kernels
        lo, med, hi = timed(env, step, everybody)
        say(f"one step ({'float64 rows' if rows == 'no rows' else rows:12s})            {n} envs: us per launch  min {lo:7.3f}  median {med:7.3f}  max {hi:7.3f}")
        for percent in (0, 1, 10, 100):
            mask = np.zeros(n, dtype=np.uint8)
            mask[np.random.default_rng(2).permutation(n)[:n * percent // 100]] = 1
            call = lambda k: env.reset_device(b["mask"], None, None, b["obs32"] if rows == "float32 rows" else None)
            b["mask"].from_host(mask)
            timed(env, call)
            lo, med, hi = timed(env, call)
            say(f"reset_device {rows:12s} {percent:3d} % chosen ({int(mask.sum()):4d}) {n} envs: us per call    min {lo:7.3f}  median {med:7.3f}  max {hi:7.3f}")
    env.close()


def loop():
    steps = args.launches * args.reps
    for name, auto in (("step_device_f32 + reset_device(), auto_reset off", False), ("step_device_f32 alone, auto_reset on", True)):
        env = make(args.max_steps, auto)
        n, b = env.num_envs, buffers(env)

        def it(k):
            env.step_device_f32(b["act"].ptr + (k % 8) * n * A * 4, b["obs32"], b["rew"], b["term"], b["trunc"])
            if not auto:
                env.reset_device(None, None, None, b["obs32"])

        timed(env, it)
        env.sync()
        s0 = env.stats()["env_steps"]
        lo, med, hi = timed(env, it)
        live = env.stats()["env_steps"] - s0
        total_us = med * steps                                # (median region time x regions: the regions are alike)
        say(f"loop: {name:50s} {n} envs, episodes of {args.max_steps}: us per iteration  min {lo:7.3f}  median {med:7.3f}  max {hi:7.3f};  "
            f"{live} live env-steps in {steps} iterations ({live / (steps * n):.4f} per env and iteration), {total_us * 1e3 / live:.4f} ns per live env-step")
        env.close()


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    one_call()
    loop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(LINES) + "\n")
