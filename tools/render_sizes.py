#!/usr/bin/env python3
"""What a frame costs (cz_render_device, k_render), config 2's shape (coop_test 7 x 7, 2 agents, scheme3), builtin sprites M = 16:

  * one call per output form - rgb8, chw32, both - at P = 8, 16 and 80, for each batch size and for a single env of it, next
    to the one-step launch without an observation and observe_grid_device(d_grid32) of the same process; bytes written per
    call over the time beside every row;
  * per step: step_device without an observation + render_device(d_chw32, P = 8);
  * the host route to the same frames: get_state + render.host_frame + upload, by the host's clock.

Device figures: K calls captured once into a graph on a stream of the caller and replayed; the time between two device events
around the replays, per call, median of `--reps` timed runs (min and max beside it).  K shrinks with the bytes a call writes, so
that one timed run stays near --run-bytes.  An output above --max-bytes is not allocated: the row says it does not fit.  With a
library that lacks cz_render_device (the parent of --alternate) only the step and grid rows are measured.  Writes
profiles/r24/render_sizes.txt.

    python3 tools/render_sizes.py 4096 65536
"""
import os

import measure

ap = measure.parser(__doc__, reps=5, out=os.path.join(measure.REPO, "profiles", "r24", "render_sizes.txt"))
ap.add_argument("--calls", type=int, default=100, help="most calls per captured graph")
ap.add_argument("--replays", type=int, default=3, help="graph launches per timed run")
ap.add_argument("--run-bytes", type=float, default=2e11, help="bytes one timed run may write (bounds the calls per graph)")
ap.add_argument("--max-bytes", type=float, default=48 * 2**30, help="largest output buffer that is allocated")
ap.add_argument("--host-envs", type=int, default=64, help="envs the host route is timed at (a Python loop over records)")
ap.add_argument("--tiles", type=int, nargs="*", default=[8, 16, 80])
ap.add_argument("sizes", type=int, nargs="*", default=[4096, 65536])


def legs(args, report):
    import numpy as np
    from cooking_zoo_amd import render
    A = measure.A
    has_render = measure.has_entry("cz_render_device")
    report.say(f"frames, coop_test / example, {A} agents, scheme3, builtin sprites M = 16; up to {args.calls} calls per graph, "
               f"{args.replays} launches per run, {args.reps} runs; us per call between two device events")
    if not has_render:
        report.say("this library has no cz_render_device: the render rows are unmeasured")
    for n in args.sizes:
        env = measure.make_env(n)
        W, H, _ = env.grid_shape()
        report.say(f"\n{n} envs, {W} x {H} cells")
        b = measure.step_buffers(env, 1, 0, ("rew", "term", "trunc"))
        act, rew, term, trunc = b["act"], b["rew"], b["term"], b["trunc"]
        grid32 = env.alloc((n,) + env.grid_shape(), np.float32)
        if has_render:
            env.load_sprites(M=16)

        def timed(replay, leg, body, nbytes=0, note="", count=n):
            calls = max(2, min(args.calls, int(args.run_bytes / args.replays / nbytes))) if nbytes else args.calls
            us = report.row(leg, count, "call", replay(body, calls, args.replays, args.reps), note)
            if nbytes:
                report.say(f"      {nbytes / 2**20:.2f} MiB written per call, {nbytes / us / 1e3:.1f} GB/s")
            return us

        with measure.graph_replay(env) as replay:
            timed(replay, "step_device, no observation", lambda: env.step_device(act, None, rew, term, trunc))
            timed(replay, "observe_grid_device grid32", lambda: env.observe_grid_device(d_grid32=grid32), grid32.nbytes)
            for P in args.tiles if has_render else ():
                h, w, _ = env.frame_shape(P)
                for count in (n, 1):
                    size = dict(rgb8=count * h * w * 3, chw32=count * h * w * 12)
                    if size["chw32"] > args.max_bytes:
                        report.say(f"  render_device P = {P}, {count} envs: chw32 would take {size['chw32'] / 2**30:.1f} GiB: does not fit (unmeasured)")
                    if size["rgb8"] > args.max_bytes:
                        report.say(f"  render_device P = {P}, {count} envs: rgb8 would take {size['rgb8'] / 2**30:.1f} GiB: does not fit (unmeasured)")
                        continue
                    d_rgb = env.alloc((count, h, w, 3), np.uint8)
                    d_chw = env.alloc((count, 3, h, w), np.float32) if size["chw32"] <= args.max_bytes else None
                    timed(replay, f"render_device P = {P} rgb8", lambda: env.render_device(d_rgb8=d_rgb, P=P, env_count=count), size["rgb8"], count=count)
                    if d_chw is not None:
                        timed(replay, f"render_device P = {P} chw32", lambda: env.render_device(d_chw32=d_chw, P=P, env_count=count), size["chw32"], count=count)
                        timed(replay, f"render_device P = {P} rgb8 + chw32", lambda: env.render_device(d_rgb, d_chw, P=P, env_count=count),
                              size["rgb8"] + size["chw32"], count=count)
                        d_chw.free()
                    d_rgb.free()
            if has_render:
                h, w, _ = env.frame_shape(8)
                d_chw = env.alloc((n, 3, h, w), np.float32)

                def pair():
                    env.step_device(act, None, rew, term, trunc)
                    env.render_device(d_chw32=d_chw, P=8)

                timed(replay, "step_device, no observation + render_device chw32 P = 8", pair, d_chw.nbytes, "per step")
        if has_render:
            m = min(n, args.host_envs)
            sheet, got = render.builtin_sprites(16), {}
            d_small = env.alloc((m,) + env.frame_shape(8), np.uint8)
            parts = (lambda: got.update(recs=env.get_state()),
                     lambda: got.update(frames=render.host_frame(env.dims, got["recs"][:m], 8, sheet)),
                     lambda: d_small.from_host(got["frames"]))
            us = measure.host_clock(env, parts, 1, 3)
            for leg, part, count in zip(("get_state", "numpy model (render.host_frame, P = 8)", "upload"), us, (n, m, m)):
                report.row(f"host route: {leg}", count, "call", part, "host clock")
            if m < n:
                report.say(f"  host route: the model and the upload are timed at {m} envs (a Python loop, linear in the envs); at {n} envs unmeasured")
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
