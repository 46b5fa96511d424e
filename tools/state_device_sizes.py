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
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r17", "state_device.txt"))
ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--launches", type=int, default=100)
A = measure.A


def on_the_stream(args, report, env, n, b):
    import numpy as np

    def timed(leg, unit, fn, before=None):                                  # one whole pass warms the leg's kernels and is dropped
        report.row(leg, n, unit, measure.handle_events(env, measure.times(fn, args.launches), args.launches, args.reps, before, warm=args.reps))

    act = lambda k: b["act"].ptr + (k % 8) * n * A * 4
    everybody = lambda: env.restore_device(b["fresh"])                     # every env alive and young: the step legs never meet a frozen env
    for rows, step in (("no rows", lambda k: env.step_device(act(k), b["obs"], b["rew"], b["term"], b["trunc"])),
                       ("float32 rows", lambda k: env.step_device_f32(act(k), b["obs32"], b["rew"], b["term"], b["trunc"]))):
        obs32 = b["obs32"] if rows == "float32 rows" else None
        timed(f"one step ({'float64 rows' if rows == 'no rows' else rows})", "launch", step, everybody)
        everybody()
        for k in range(20):                                                 # a state that is not the reset state
            env.step_device(act(k), b["obs"], b["rew"], b["term"], b["trunc"])
        if rows == "no rows":
            timed("save_device, identity", "call", lambda k: env.save_device(b["arch"]))
        for percent in (0, 1, 10, 100):
            slots = np.full(n, -1, dtype=np.int32)
            chosen = np.random.default_rng(2).permutation(n)[:n * percent // 100]
            slots[chosen] = chosen
            b["slot"].from_host(slots)
            timed(f"restore_device {rows} {percent} % chosen ({len(chosen)})", "call", lambda k: env.restore_device(b["arch"], b["slot"], None, obs32))
        b["slot"].from_host(((np.arange(n, dtype=np.int64) * 7 + 3) % n).astype(np.int32))
        timed(f"fork_device {rows} a permutation (2 launches)", "call", lambda k: env.fork_device(b["slot"], None, obs32))


def to_the_host(args, report, env, n, b):
    import numpy as np
    for what, lo, count in (("the whole batch", 0, n), ("1 % as one range", n // 3, max(1, n // 100))):
        slots = np.full(n, -1, dtype=np.int32)
        slots[lo:lo + count] = np.arange(lo, lo + count)
        b["slot"].from_host(slots)

        def host_way():
            recs = env.get_state(lo, count)
            env.set_state(recs, lo)
            env.observe_device(d_obs32=b["obs32"].ptr + lo * A * env.F * 4, env_begin=lo, env_count=count)

        def device_way():
            env.save_device(b["arch"], b["slot"])
            env.restore_device(b["arch"], b["slot"], None, b["obs32"])

        host, dev = measure.host_clock(env, (host_way, device_way), 1, args.reps, warm=1)       # (each way's first run is its warm-up)
        report.row(f"{what} ({count} envs) get_state + set_state + observe_device + sync", n, "call", host, "host clock")
        report.row(f"{what} ({count} envs) save_device + restore_device (f32 rows) + sync", n, "call", dev, "host clock")


def legs(args, report):
    import numpy as np
    for n in args.envs:
        env = measure.make_env(n, auto_reset=False)
        RW = env.dims.RW
        b = measure.step_buffers(env, 8, 1, ("obs", "obs32", "rew", "term", "trunc"))
        b.update(slot=env.alloc((n,), np.int32), arch=env.alloc((n, RW), np.uint32), fresh=env.alloc((n, RW), np.uint32))
        env.save_device(b["fresh"])
        env.save_device(b["arch"])
        report.say(f"{n:6d} envs  record: {RW} words ({RW * 4} bytes); float32 rows: {A * env.F * 4} bytes per env")
        on_the_stream(args, report, env, n, b)
        to_the_host(args, report, env, n, b)
        assert env.restore_device_refused() == 0
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
