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
import argparse
import contextlib
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cooking_zoo_amd import _native, grid  # noqa: E402
from cooking_zoo_amd.vec_env import CookingVecEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200, help="calls per captured graph")
ap.add_argument("--replays", type=int, default=5, help="graph launches per timed run")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-envs", type=int, default=4096, help="largest batch the host route is timed at (a Python loop over records)")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r20", "grid_sizes.txt"))
ap.add_argument("sizes", type=int, nargs="*", default=[4096, 65536])
args = ap.parse_args()

A, RECIPES = 2, ["TomatoLettuceSalad", "CarrotBanana"]
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


class Graph:
    """K calls captured on a stream of the caller, replayed between two events"""

    def __init__(self, env):
        rccl, hip = C.create_string_buffer(512), C.create_string_buffer(512)
        _native.lib().cz_runtime_paths(rccl, hip, 512)
        self.hip, self.env = C.CDLL(hip.value.decode()), env
        self.stream, self.ev = C.c_void_p(), [C.c_void_p(), C.c_void_p()]
        self.ck(self.hip.hipStreamCreateWithFlags(C.byref(self.stream), 1))
        for e in self.ev:
            self.ck(self.hip.hipEventCreate(C.byref(e)))
        env.set_stream(self.stream)

    def ck(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    @contextlib.contextmanager
    def capture(self):
        self.graph, self.gexec = C.c_void_p(), C.c_void_p()
        self.ck(self.hip.hipStreamBeginCapture(self.stream, 0))
        yield
        self.ck(self.hip.hipStreamEndCapture(self.stream, C.byref(self.graph)))
        self.ck(self.hip.hipGraphInstantiate(C.byref(self.gexec), self.graph, None, None, C.c_size_t(0)))

    def time_us(self, calls):
        """us per call: `--reps` runs of `--replays` launches each, after one warming launch"""
        out = []
        for r in range(args.reps + 1):
            self.ck(self.hip.hipEventRecord(self.ev[0], self.stream))
            for _ in range(args.replays):
                self.ck(self.hip.hipGraphLaunch(self.gexec, self.stream))
            self.ck(self.hip.hipEventRecord(self.ev[1], self.stream))
            self.ck(self.hip.hipEventSynchronize(self.ev[1]))
            ms = C.c_float()
            self.ck(self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]))
            if r:
                out.append(ms.value * 1e3 / (args.replays * calls))
        self.hip.hipGraphExecDestroy(self.gexec)
        self.hip.hipGraphDestroy(self.graph)
        return sorted(out)


def report(label, us, note=""):
    say(f"  {label:58s} median {us[len(us) // 2]:9.3f} us   min {us[0]:9.3f}   max {us[-1]:9.3f}   {note}")
    return us[len(us) // 2]


def main():
    say(f"grid observation, coop_test / example, {A} agents, scheme3; {args.calls} calls per graph, {args.replays} launches per run, "
        f"{args.reps} runs; us per call between two device events")
    for n in args.sizes:
        env = CookingVecEnv(n, "coop_test", "example", A, 400, RECIPES, action_scheme="scheme3", num_layouts=64, auto_reset=True)
        env.reset(return_obs=False)
        W, H, _ = env.grid_shape()
        say(f"\n{n} envs, {W} x {H} cells")
        act = env.alloc((n, A), np.int32)
        act.from_host(np.random.default_rng(0).integers(0, 5, size=(n, A), dtype=np.int32))
        rew, term, trunc = env.alloc((n, A), np.float64), env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)
        obs64, obs32 = env.alloc((n, A, env.F), np.float64), env.alloc((n, A, env.F), np.float32)
        bufs = {ext: dict(bits=env.alloc((n, W, H, 2 if ext else 1), np.uint32), grid8=env.alloc((n,) + env.grid_shape(ext), np.uint8),
                          grid32=env.alloc((n,) + env.grid_shape(ext), np.float32)) for ext in (False, True)}
        xy = env.alloc((n, A, 2), np.int32)
        g = Graph(env)
        K = args.calls

        def timed(label, body, note=""):
            with g.capture():
                for _ in range(K):
                    body()
            return report(label, g.time_us(K), note)

        timed("step_device, float64 rows", lambda: env.step_device(act, obs64, rew, term, trunc), f"{n * A * env.F * 8 / 2**20:.1f} MiB of rows")
        step0 = timed("step_device, no observation", lambda: env.step_device(act, None, rew, term, trunc))
        f32 = timed("step_device_f32", lambda: env.step_device_f32(act, obs32, rew, term, trunc), f"{n * A * env.F * 4 / 2**20:.1f} MiB of rows")
        for ext in (False, True):
            for form in ("bits", "grid8", "grid32"):
                b = bufs[ext][form]
                timed(f"observe_grid_device {form}{' extended' if ext else ''}", lambda: env.observe_grid_device(extended=ext, **{"d_" + form: b}),
                      f"{b.nbytes / 2**20:.2f} MiB written")
        timed("observe_grid_device agent_xy only", lambda: env.observe_grid_device(d_agent_xy=xy))

        def pair():
            env.step_device(act, None, rew, term, trunc)
            env.observe_grid_device(d_grid32=bufs[False]["grid32"])

        both = timed("step_device, no observation + observe_grid_device grid32", pair, "per step")
        say(f"  per step: step + grid32 {both:.3f} us  against  step_device_f32 {f32:.3f} us  (step alone {step0:.3f} us)")
        env.set_stream(None)
        # the host route, by the host's clock
        if n <= args.host_envs:
            d_grid = bufs[False]["grid32"]
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                recs = env.get_state()
                t1 = time.perf_counter()
                grid32 = grid.expand(grid.host_bits(env.dims, recs), np.float32)
                t2 = time.perf_counter()
                d_grid.from_host(grid32)
                t3 = time.perf_counter()
                t.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
            tot, get, model, up = sorted(t)[1]
            say(f"  host route (get_state + grid.host_bits + expand + upload), host clock, median of 3: {tot * 1e3:.1f} ms "
                f"(get_state {get * 1e3:.2f} ms, numpy model {model * 1e3:.1f} ms, upload {up * 1e3:.2f} ms)")
        else:
            say(f"  host route: unmeasured at {n} envs (timed up to --host-envs {args.host_envs}; the Python model is linear in the envs)")
        env.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
