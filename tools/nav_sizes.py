#!/usr/bin/env python3
"""What the navigation call costs (cz_navigate_device, k_navigate), config 2's shape (coop_test, 2 agents, scheme3):

  * one call with T = 1 and with T = 8 targets per agent (seeded targets over all cells), writing action and steps, and the same
    with the distance field as well, next to the one-step launch (no observation) and observe_grid_device(bits) of the same process;
  * per step: navigate_device(d_action) + step_device(d_action), the closed loop of a scripted partner;
  * the host route to the same answers: get_state + nav.host_navigate (+ upload of the actions), by the host's clock.

Device figures: K calls captured once into a graph on a stream of the caller and replayed; the time between two device events
around the replays, per call, median of `--reps` timed runs (min and max beside it).  Writes profiles/r21/nav_sizes.txt.

    python3 tools/nav_sizes.py 4096 65536
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r21", "nav_sizes.txt"))
ap.add_argument("--calls", type=int, default=200, help="calls per captured graph")
ap.add_argument("--replays", type=int, default=5, help="graph launches per timed run")
ap.add_argument("--host-envs", type=int, default=4096, help="largest batch the host route is timed at (a Python loop over records)")
ap.add_argument("sizes", type=int, nargs="*", default=[4096, 65536])


def legs(args, report):
    import numpy as np
    from cooking_zoo_amd import nav
    A = measure.A
    report.say(f"navigation, coop_test / example, {A} agents, scheme3; {args.calls} calls per graph, {args.replays} launches per run, "
               f"{args.reps} runs; us per call between two device events")
    for n in args.sizes:
        env = measure.make_env(n)
        W, H, _ = env.grid_shape()
        C = W * H
        report.say(f"\n{n} envs, {W} x {H} cells")
        b = measure.step_buffers(env, 1, 0, ("rew", "term", "trunc"))
        act, rew, term, trunc = b["act"], b["rew"], b["term"], b["trunc"]
        bits = env.alloc((n, W, H, 1), np.uint32)
        rng = np.random.default_rng(1)
        bufs = {}
        for T in (1, 8):
            tg = np.stack([rng.integers(0, W, (n, A, T)), rng.integers(0, H, (n, A, T))], axis=-1).astype(np.int32)
            bufs[T] = dict(host=tg, target=env.alloc((n, A, T, 2), np.int32), action=env.alloc((n, A, T), np.int32),
                           steps=env.alloc((n, A, T), np.int32), field=env.alloc((n, A, T, C), np.uint16))
            bufs[T]["target"].from_host(tg)

        def timed(leg, body, note=""):
            return report.row(leg, n, "call", replay(body, args.calls, args.replays, args.reps), note)

        with measure.graph_replay(env) as replay:
            step0 = timed("step_device, no observation", lambda: env.step_device(act, None, rew, term, trunc))
            timed("observe_grid_device bits", lambda: env.observe_grid_device(d_bits=bits), f"{bits.nbytes / 2**20:.2f} MiB written")
            for T in (1, 8):
                d = bufs[T]
                timed(f"navigate_device T={T}, action + steps", lambda: env.navigate_device(d["target"], d["action"], d["steps"]),
                      f"{A * T} fills per env")
                timed(f"navigate_device T={T}, action + steps + field", lambda: env.navigate_device(d["target"], d["action"], d["steps"], d["field"]),
                      f"{d['field'].nbytes / 2**20:.2f} MiB of field")
            d = bufs[1]

            def pair():
                env.navigate_device(d["target"], d["action"])
                env.step_device(d["action"], None, rew, term, trunc)

            both = timed("navigate_device T=1 (action) + step_device, no observation", pair, "per step")
        report.say(f"  per step: navigate + step {both:.3f} us  (step alone {step0:.3f} us)")
        # the host route, by the host's clock: three runs of its three parts in turn
        if n <= args.host_envs:
            got = {}
            parts = (lambda: got.update(recs=env.get_state()),
                     lambda: got.update(act=nav.host_navigate(env.dims, got["recs"], d["host"])[0]),
                     lambda: d["action"].from_host(got["act"]))
            us = measure.host_clock(env, parts, 1, 3)
            for leg, part in zip(("get_state", "Python model (nav.host_navigate, T=1)", "upload of the actions"), us):
                report.row(f"host route: {leg}", n, "call", part, "host clock")
            report.row("host route: get_state + nav.host_navigate + upload", n, "call", [sum(p) for p in zip(*us)], "host clock")
        else:
            report.say(f"  host route: unmeasured at {n} envs (timed up to --host-envs {args.host_envs}; the Python model is linear in the envs)")
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
