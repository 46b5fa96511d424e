#!/usr/bin/env python3
"""Launch duration of the one-step kernel under different action streams (boundary-ordered launches, HIP events around
400 back-to-back launches): stay (nobody acts: every wave runs the same path), random (the bench workload),
rich (random actions, episodes never end: after 3000 warm-up steps most agents carry something and the worlds are full of
chopped / plated objects).
    python3 tools/mode_timing.py [N]"""
import measure

ap = measure.parser(__doc__, reps=5)
ap.add_argument("N", type=int, nargs="?", default=4096)


def legs(args, report):
    import numpy as np
    N, P, K = args.N, 64, 400
    rng = np.random.default_rng(0)                       # one generator: each mode's ring is the next draw from it
    for mode in ("stay", "random", "rich"):
        env = measure.make_env(N, (1 << 30) if mode == "rich" else 400, num_layouts=256)
        b = measure.step_buffers(env, P, rng)
        if mode == "stay":
            b["act"].from_host(np.zeros((P, N, 2), dtype=np.int32))
        ring = lambda k: env.step_device_ring(k, b["act"], N * 2, P, 0, b["obs"], b["rew"], b["term"], b["trunc"])
        ring(3000 if mode == "rich" else 300)
        env.sync()
        report.row(mode, N, "launch", measure.handle_events(env, lambda: ring(K), K, args.reps))
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
