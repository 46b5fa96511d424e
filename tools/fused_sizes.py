#!/usr/bin/env python3
"""Fused rollouts by batch size (bench workload, 32 steps per launch): on-device actions with a float64 trajectory (cz_rollout),
with a compact trajectory (cz_rollout_compact), and ring runs fused with the float64 rows
written in place (cz_set_ring_fused).  env-steps/s and ns per env-step.
    python3 tools/fused_sizes.py [N ...]"""
import measure

ap = measure.parser(__doc__, reps=3)
ap.add_argument("sizes", type=int, nargs="*", default=[4096, 8192, 16384, 32768, 65536])
T = 32


def legs(args, report):
    import numpy as np

    def row(leg, N, us):
        b = min(us) * 1e-6
        report.row(leg, N, "step", us, f"{N / b / 1e9:5.2f} G env-steps/s ({b * 1e9 / N:.3f} ns per env-step)")

    for N in args.sizes:
        env = measure.make_env(N, num_layouts=256)
        for compact in (False, True):
            if compact:
                buf = env.alloc((T, N, 2, env.codes_pitch), np.uint8)
                run = lambda r: env.rollout_compact(T, 1, r * T, buf)
            else:
                if T * N * 2 * env.F * 8 > (6 << 30):
                    report.say(f"float64 trajectory: n/a at {N} envs")
                    continue
                buf = env.alloc((T, N, 2, env.F), np.float64)
                rew, te, tr = env.alloc((T, N, 2), np.float64), env.alloc((T, N, 2), np.uint8), env.alloc((T, N, 2), np.uint8)
                run = lambda r: env.rollout(T, 1, r * T, buf, rew, te, tr)
            run(0); env.sync()
            K = max(3, 2000 // T // max(1, N // 4096))
            row("compact trajectory" if compact else "float64 trajectory", N,
                measure.host_clock(env, measure.times(lambda r: run(r + 1), K), K * T, args.reps))
            buf.free()
        # ring runs fused, outputs in place (cz_set_ring_fused): 64-slot ring, runs of 512 steps
        period, K = 64, 512
        b = measure.step_buffers(env, period, 1)
        env.set_ring_fused(True)
        ring = lambda: env.step_device_ring(K, b["act"], N * 2, period, 0, b["obs"], b["rew"], b["term"], b["trunc"])
        ring(); env.sync()
        row("ring run fused, float64 rows in place", N, measure.host_clock(env, ring, K, args.reps))
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
