#!/usr/bin/env python3
"""Host-array step (cz_step: actions from host memory, observations / rewards / flags copied back) at BASELINE config 2's
size, with fresh pageable output arrays and with the env's pinned output buffers.  PCIe-inclusive: never the bench value.
    python3 tools/host_step_latency.py [N]"""
import measure

ap = measure.parser(__doc__, reps=1)
ap.add_argument("N", type=int, nargs="?", default=4096)


def legs(args, report):
    import numpy as np
    N, K = args.N, 200
    acts = np.random.default_rng(0).integers(0, 5, size=(64, N, 2), dtype=np.int32)
    out = {}                     # every leg's last outputs stay alive until the leg runs again, as a caller's variables would
    for pinned in (False, True):
        env = measure.make_env(N, num_layouts=256, pinned_outputs=pinned)

        def timed(leg, call, warm, note=lambda dt: ""):
            for i in range(warm):
                call(i)

            def body():
                for i in range(K):
                    out[leg] = call(i % 64)

            us = measure.host_clock(env, body, K, args.reps)
            report.row(f"pinned_outputs={pinned}, {leg}", N, "step", us, f"{N / min(us):.1f} M env-steps/s" + note(min(us)))
            return out[leg]

        obs = timed("host-array step", lambda i: env.step(acts[i]), 10,
                    lambda dt: f", {sum(a.nbytes for a in out['host-array step']) / dt / 1e3:.1f} GB/s of outputs")[0]
        timed("COMPACT observation (uint8 codes)", lambda i: env.step_compact(acts[i]), 10,
              lambda dt: f", {out['COMPACT observation (uint8 codes)'][0].nbytes / 1e6:.1f} MB instead of {obs.nbytes / 1e6:.1f} MB")
        timed("no observation copy", lambda i: env.step(acts[i], return_obs=False), 0)
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
