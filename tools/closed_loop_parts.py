#!/usr/bin/env python3
"""Where a closed-loop step's time goes (4096 envs, bench workload): the step kernel alone writing float64 rows / codes only /
nothing, issued back to back from Python (direct launches), and the two closed loops of bench.py.
    python3 tools/closed_loop_parts.py [N]"""
import ctypes as C
import os

import measure

ap = measure.parser(__doc__, reps=3)
ap.add_argument("N", type=int, nargs="?", default=4096)


def legs(args, report):
    from cooking_zoo_amd import _native
    L, N = _native.lib(), args.N
    env = measure.make_env(N, num_layouts=256)
    h = env._h
    d_act, d_obs, d_codes, d_rew, d_t, d_u = measure.step_buffers(env, 1, 0, ("obs", "codes", "rew", "term", "trunc")).values()

    def timed(leg, fn, n=3000):
        for _ in range(200):
            fn(0)
        env.sync()
        report.row(leg, N, "launch", measure.handle_events(env, measure.times(fn, n), n, args.reps))

    timed("step, float64 rows (direct launches from Python)", lambda i: L.cz_step_device(h, d_act.ptr, d_obs.ptr, d_rew.ptr, d_t.ptr, d_u.ptr))
    timed("step, codes only", lambda i: L.cz_step_device_compact(h, d_act.ptr, d_codes.ptr, None, d_rew.ptr, d_t.ptr, d_u.ptr))
    timed("step, codes + float64", lambda i: L.cz_step_device_compact(h, d_act.ptr, d_codes.ptr, d_obs.ptr, d_rew.ptr, d_t.ptr, d_u.ptr))
    timed("step, no observation", lambda i: L.cz_step_device(h, d_act.ptr, None, d_rew.ptr, d_t.ptr, d_u.ptr))

    def probes(rows, codes_row):
        """the library's own closed-loop probe (graph of 200 steps, 10 replays), float64 rows and codes, twice in turn"""
        us, runs = C.c_float(), ([], [])
        for rep in range(2):
            _native.check(h, L.cz_probe_closed_loop(h, 200, 10, d_act.ptr, d_obs.ptr, d_rew.ptr, d_t.ptr, d_u.ptr, C.byref(us)))
            runs[0].append(us.value)
            _native.check(h, L.cz_probe_closed_loop_compact(h, 200, 10, d_act.ptr, d_codes.ptr, d_rew.ptr, d_t.ptr, d_u.ptr, C.byref(us)))
            runs[1].append(us.value)
        report.row(rows, N, "step", runs[0])
        report.row(codes_row, N, "step", runs[1])

    os.environ["CZ_PROBE_NO_POLICY"] = "1"
    probes("graph of 200 step kernels WITHOUT the policy kernel: float64 rows", "graph of 200 step kernels WITHOUT the policy kernel: codes only")
    del os.environ["CZ_PROBE_NO_POLICY"]
    probes("closed loop: float64", "closed loop: codes")
    env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
