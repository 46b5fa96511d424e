#!/usr/bin/env python3
"""What `save_device`, `restore_device` and `fork_device` (cz_save_device, cz_restore_device) cost, on config 2's shape (coop_test, 2
agents, scheme3, F = 278) at 4096 and 65 536 envs:

  on the stream   K calls between two device events on the handle's stream, --reps times (min / median / max per call): one identity
                  save_device; restore_device with a slot array that chooses 0 %, 1 %, 10 % and 100 % of the envs (the same envs in
                  every call, each taking its own row, so every call does the same work); fork_device with a permutation; each
                  without output rows and with float32 rows; next to them the one-step launch of the same handle (step_device with
                  float64 rows / step_device_f32), every env alive
  to the host     the same end by the only way there was before: get_state + set_state + observe_device over the same envs (the whole
                  batch; 1 % of it as one contiguous range, the host way's best case), against save_device + restore_device + sync,
                  both by the host's clock around the calls, the two ways alternated rep by rep in one process

Writes every line to --out (default profiles/r17/state_device.txt).  Needs a GPU; nothing is estimated without one.

    python3 tools/state_device_sizes.py
"""
import argparse
import ctypes as C
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17", "state_device.txt"))
ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--launches", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
A, RECIPES = 2, ["TomatoLettuceSalad", "CarrotBanana"]
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def spread(us):
    us = sorted(us)
    return f"min {us[0]:9.3f}  median {us[len(us) // 2]:9.3f}  max {us[-1]:9.3f}"


def timed(env, fn, before=None):
    """us per call of fn over --launches calls between two device events, --reps times"""
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
    return us


def on_the_stream(env, n, b):
    import numpy as np
    act = lambda k: b["act"].ptr + (k % 8) * n * A * 4
    everybody = lambda: env.restore_device(b["fresh"])                     # every env alive and young: the step legs never meet a frozen env
    for rows, step in (("no rows", lambda k: env.step_device(act(k), b["obs"], b["rew"], b["term"], b["trunc"])),
                       ("float32 rows", lambda k: env.step_device_f32(act(k), b["obs32"], b["rew"], b["term"], b["trunc"]))):
        obs32 = b["obs32"] if rows == "float32 rows" else None
        timed(env, step, everybody)                                         # warm-up of the leg's kernels
        say(f"{n:6d} envs  one step ({'float64 rows' if rows == 'no rows' else rows:12s})                     us per launch  {spread(timed(env, step, everybody))}")
        everybody()
        for k in range(20):                                                 # a state that is not the reset state
            env.step_device(act(k), b["obs"], b["rew"], b["term"], b["trunc"])
        if rows == "no rows":
            timed(env, lambda k: env.save_device(b["arch"]))
            say(f"{n:6d} envs  save_device, identity                             us per call    {spread(timed(env, lambda k: env.save_device(b['arch'])))}")
        for percent in (0, 1, 10, 100):
            slots = np.full(n, -1, dtype=np.int32)
            chosen = np.random.default_rng(2).permutation(n)[:n * percent // 100]
            slots[chosen] = chosen
            b["slot"].from_host(slots)
            call = lambda k: env.restore_device(b["arch"], b["slot"], None, obs32)
            timed(env, call)
            say(f"{n:6d} envs  restore_device {rows:12s} {percent:3d} % chosen ({len(chosen):5d})  us per call    {spread(timed(env, call))}")
        b["slot"].from_host(((np.arange(n, dtype=np.int64) * 7 + 3) % n).astype(np.int32))
        call = lambda k: env.fork_device(b["slot"], None, obs32)
        timed(env, call)
        say(f"{n:6d} envs  fork_device    {rows:12s} a permutation (2 launches)  us per call    {spread(timed(env, call))}")


def to_the_host(env, n, b):
    import numpy as np
    for what, lo, count in (("the whole batch", 0, n), ("1 % as one range", n // 3, max(1, n // 100))):
        slots = np.full(n, -1, dtype=np.int32)
        slots[lo:lo + count] = np.arange(lo, lo + count)
        b["slot"].from_host(slots)
        host, dev = [], []
        for rep in range(args.reps + 1):                                    # (the first rep of each way is its warm-up)
            env.sync()
            t0 = time.perf_counter()
            recs = env.get_state(lo, count)
            env.set_state(recs, lo)
            env.observe_device(d_obs32=b["obs32"].ptr + lo * A * env.F * 4, env_begin=lo, env_count=count)
            env.sync()
            t1 = time.perf_counter()
            env.save_device(b["arch"], b["slot"])
            env.restore_device(b["arch"], b["slot"], None, b["obs32"])
            env.sync()
            t2 = time.perf_counter()
            if rep:
                host.append((t1 - t0) * 1e6); dev.append((t2 - t1) * 1e6)
        say(f"{n:6d} envs  {what:16s} ({count:5d} envs)  get_state + set_state + observe_device + sync   us, host clock  {spread(host)}")
        say(f"{n:6d} envs  {what:16s} ({count:5d} envs)  save_device + restore_device (f32 rows) + sync  us, host clock  {spread(dev)}")


def main():
    import numpy as np
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for n in args.envs:
        env = CookingVecEnv(n, "coop_test", "example", A, 400, RECIPES, action_scheme="scheme3", num_layouts=64, auto_reset=False)
        env.reset(return_obs=False)
        F, RW = env.F, env.dims.RW
        b = dict(act=env.alloc((8, n, A), np.int32), obs=env.alloc((n, A, F), np.float64), obs32=env.alloc((n, A, F), np.float32),
                 rew=env.alloc((n, A), np.float64), term=env.alloc((n, A), np.uint8), trunc=env.alloc((n, A), np.uint8),
                 slot=env.alloc((n,), np.int32), arch=env.alloc((n, RW), np.uint32), fresh=env.alloc((n, RW), np.uint32))
        b["act"].from_host(np.random.default_rng(1).integers(0, 5, size=(8, n, A), dtype=np.int32))
        env.save_device(b["fresh"])
        env.save_device(b["arch"])
        say(f"{n:6d} envs  record: {RW} words ({RW * 4} bytes); float32 rows: {A * F * 4} bytes per env")
        on_the_stream(env, n, b)
        to_the_host(env, n, b)
        assert env.restore_device_refused() == 0
        env.close()


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    main()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(LINES) + "\n")
