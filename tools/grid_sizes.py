#!/usr/bin/env python3
"""What the grid observation costs (cz_observe_grid_device, k_observe_grid), config 2's shape (coop_test, 2 agents, scheme3):

  * one call per form - bits, grid8, grid32, each plain (32 channels) and extended (48) - next to the one-step launch (float64
    rows, and no observation at all) and step_device_f32 of the same process;
  * per step: step_device without an observation + observe_grid_device(d_grid32), against step_device_f32;
  * the host route to the same tensor: get_state + grid.host_bits + expand + upload, by the host's clock.

Device figures: K calls captured once into a graph on a stream of the caller and replayed; the time between two device events
around the replays, per call, median of `--reps` timed runs (min and max beside it).  Writes profiles/r20/grid_sizes.txt.

    python3 tools/grid_sizes.py 4096 65536
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r20", "grid_sizes.txt"))
ap.add_argument("--calls", type=int, default=200, help="calls per captured graph")
ap.add_argument("--replays", type=int, default=5, help="graph launches per timed run")
ap.add_argument("--host-envs", type=int, default=4096, help="largest batch the host route is timed at (a Python loop over records)")
ap.add_argument("sizes", type=int, nargs="*", default=[4096, 65536])


def legs(args, report):
    import numpy as np
    from cooking_zoo_amd import grid
    A = measure.A
    report.say(f"grid observation, coop_test / example, {A} agents, scheme3; {args.calls} calls per graph, {args.replays} launches per run, "
               f"{args.reps} runs; us per call between two device events")
    for n in args.sizes:
        env = measure.make_env(n)
        W, H, _ = env.grid_shape()
        report.say(f"\n{n} envs, {W} x {H} cells")
        b = measure.step_buffers(env, 1, 0, ("rew", "term", "trunc", "obs", "obs32"))
        act, rew, term, trunc = b["act"], b["rew"], b["term"], b["trunc"]
        bufs = {ext: dict(bits=env.alloc((n, W, H, 2 if ext else 1), np.uint32), grid8=env.alloc((n,) + env.grid_shape(ext), np.uint8),
                          grid32=env.alloc((n,) + env.grid_shape(ext), np.float32)) for ext in (False, True)}
        xy = env.alloc((n, A, 2), np.int32)

        def timed(leg, body, note=""):
            return report.row(leg, n, "call", replay(body, args.calls, args.replays, args.reps), note)

        with measure.graph_replay(env) as replay:
            timed("step_device, float64 rows", lambda: env.step_device(act, b["obs"], rew, term, trunc), f"{n * A * env.F * 8 / 2**20:.1f} MiB of rows")
            step0 = timed("step_device, no observation", lambda: env.step_device(act, None, rew, term, trunc))
            f32 = timed("step_device_f32", lambda: env.step_device_f32(act, b["obs32"], rew, term, trunc), f"{n * A * env.F * 4 / 2**20:.1f} MiB of rows")
            for ext in (False, True):
                for form in ("bits", "grid8", "grid32"):
                    d = bufs[ext][form]
                    timed(f"observe_grid_device {form}{' extended' if ext else ''}", lambda: env.observe_grid_device(extended=ext, **{"d_" + form: d}),
                          f"{d.nbytes / 2**20:.2f} MiB written")
            timed("observe_grid_device agent_xy only", lambda: env.observe_grid_device(d_agent_xy=xy))

            def pair():
                env.step_device(act, None, rew, term, trunc)
                env.observe_grid_device(d_grid32=bufs[False]["grid32"])

            both = timed("step_device, no observation + observe_grid_device grid32", pair, "per step")
        report.say(f"  per step: step + grid32 {both:.3f} us  against  step_device_f32 {f32:.3f} us  (step alone {step0:.3f} us)")
        # the host route, by the host's clock: three runs of its three parts in turn
        if n <= args.host_envs:
            d_grid, got = bufs[False]["grid32"], {}
            parts = (lambda: got.update(recs=env.get_state()),
                     lambda: got.update(grid32=grid.expand(grid.host_bits(env.dims, got["recs"]), np.float32)),
                     lambda: d_grid.from_host(got["grid32"]))
            us = measure.host_clock(env, parts, 1, 3)
            for leg, part in zip(("get_state", "numpy model (grid.host_bits + expand)", "upload"), us):
                report.row(f"host route: {leg}", n, "call", part, "host clock")
            report.row("host route: get_state + grid.host_bits + expand + upload", n, "call", [sum(p) for p in zip(*us)], "host clock")
        else:
            report.say(f"  host route: unmeasured at {n} envs (timed up to --host-envs {args.host_envs}; the Python model is linear in the envs)")
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
