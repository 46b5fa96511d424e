#!/usr/bin/env python3
"""What the per-env episode records cost (config 2's shape: coop_test, 2 agents, scheme3, F = 278), timed with the handle's own device
events on its stream (measure.handle_events):

  step lean / step generic   one-step launches of k_step_lean<1,1,2,3> and, in a handle made under CZ_LEAN=0, k_step<1,1,2,3,0>:
                             --launches of them between two events, us per launch; max_steps = 400, so nearly every wave takes the
                             common path - the path this measurement is about
  collect all / dense        ONE collect_episodes call between two events - every output, or the dense arrays alone (one kernel
                             instead of two) - with 0 %, 1 % and 100 % of the envs found, next to ONE step launch timed the same way (`one step ... launch`).
                             A handle with auto_reset off and max_steps = 2 is armed for each call: reset_device restarts the chosen
                             envs (all, or every hundredth) and two steps finish them, while the others stay frozen.

One process measures one checkout (`--tree`, default: this one; package and built library are taken from it, so a
library goes with the package it was built for; the collect legs need the entry point).  `--alternate OTHER_TREE` is the driver
(tools/measure.py): fresh child processes, OTHER's library and this tree's alternately, `--pairs` times, then once more with the
order inside the pair reversed; every line, the summary and the band rows go to `--out` (default profiles/r16/episodes_sizes.txt).

    python3 tools/episodes_sizes.py --alternate /path/to/a/built/checkout/of/the/parent
"""
import os

import measure

ap = measure.parser(__doc__, reps=9, out=os.path.join(measure.REPO, "profiles", "r16", "episodes_sizes.txt"), timeout=300)
ap.add_argument("--sizes", default="4096,65536")
ap.add_argument("--launches", type=int, default=400)


def legs(args, report):
    import numpy as np
    from cooking_zoo_amd import _native
    K = args.launches
    for n in [int(s) for s in args.sizes.split(",")]:
        # ---- the one-step launches, common path
        for leg, lean in (("step lean", "1"), ("step generic", "0")):
            os.environ["CZ_LEAN"] = lean
            env = measure.make_env(n)
            os.environ.pop("CZ_LEAN")
            b = measure.step_buffers(env, 1, 1, ("rew", "term", "trunc", "obs"))
            one = lambda k=0: env.step_device(b["act"], b["obs"], b["rew"], b["term"], b["trunc"])
            measure.times(one, 20)()
            env.sync()
            report.row(leg, n, "launch", measure.handle_events(env, measure.times(one, K), K, args.reps))
            report.row(f"one {leg} launch", n, "call", measure.handle_events(env, one, 1, args.reps))
            env.close()
        if not measure.has_entry("cz_episodes_collect"):
            continue
        # ---- one collect call, next to one step launch
        env = measure.make_env(n, 2, auto_reset=False)
        b = measure.step_buffers(env, 1, 1, ("rew", "term", "trunc", "obs"))
        one = lambda: env.step_device(b["act"], b["obs"], b["rew"], b["term"], b["trunc"])
        mask, ret = env.alloc((n,), np.uint8), env.alloc((n, measure.A), np.float64)
        length, flags = env.alloc((n,), np.int32), env.alloc((n,), np.uint32)
        lst, cnt = env.alloc((n,), _native.EPISODE_DTYPE), env.alloc((1,), np.int32)
        every100 = env.alloc((n,), np.uint8)
        every100.from_host((np.arange(n) % 100 == 0).astype(np.uint8))
        one(); one()                                        # everybody has finished and is frozen
        env.collect_episodes()
        nobody = object()
        for pct, chosen in ((0, nobody), (1, every100), (100, None)):

            def arm():
                mask.to_host()                              # (the read-back that follows every timed call)
                if chosen is not nobody:
                    env.reset_device(chosen)
                    one(); one()
                env.sync()

            for leg, call in (("collect all", lambda: env.collect_episodes(mask, ret, length, flags, lst, n, cnt)),
                              ("collect dense", lambda: env.collect_episodes(mask, ret, length, flags))):
                us = measure.handle_events(env, call, 1, args.reps, arm)
                report.row(f"{leg} {pct} % ({int(mask.to_host().sum())} found)", n, "call", us)
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
