#!/usr/bin/env python3
"""What the scripted partner costs (cz_partner_device, k_partner), config 2's shape (coop_test, 2 agents, scheme3):

  * one call for one agent (agents=0b10) and for all agents, writing the actions alone and all three outputs, next to
    navigate_device (T = 1), the one-step launch (no observation) and observe_grid_device(bits) of the same process;
  * per step: partner_device(d_action) + step_device(d_action), the closed loop of a scripted partner - and, to tell the cost of
    the interleaving from the cost of what the partner's play makes the two kernels do, the same two launches in turn with the
    partner writing into a spare buffer and the step playing a fixed action array;
  * the host route to the same answers: get_state + partner.host_partner (+ upload of the actions), by the host's clock.

The states are those a few steps of the partner's own play leave behind (the loop above runs on them: the envs are in different
phases of their recipes, auto-reset on).  Device figures: K calls captured once into a graph on a stream of the caller and
replayed; the time between two device events around the replays, per call, median of `--reps` timed runs (min and max beside it).
Writes profiles/r22/partner_sizes.txt.

    python3 tools/partner_sizes.py 4096 65536
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r22", "partner_sizes.txt"))
ap.add_argument("--calls", type=int, default=200, help="calls per captured graph")
ap.add_argument("--replays", type=int, default=5, help="graph launches per timed run")
ap.add_argument("--host-envs", type=int, default=4096, help="largest batch the host route is timed at (a Python loop over records)")
ap.add_argument("--warm-steps", type=int, default=40, help="steps of the partner's own play before anything is timed")
ap.add_argument("sizes", type=int, nargs="*", default=[4096, 65536])


def legs(args, report):
    import numpy as np
    from cooking_zoo_amd import partner
    A = measure.A
    report.say(f"scripted partner, coop_test / example, {A} agents, scheme3; {args.calls} calls per graph, {args.replays} launches per run, "
               f"{args.reps} runs; us per call between two device events")
    for n in args.sizes:
        env = measure.make_env(n)
        W, H, _ = env.grid_shape()
        report.say(f"\n{n} envs, {W} x {H} cells")
        b = measure.step_buffers(env, 1, 0, ("rew", "term", "trunc"))
        act, rew, term, trunc = b["act"], b["rew"], b["term"], b["trunc"]
        bits = env.alloc((n, W, H, 1), np.uint32)
        target, status, steps = env.alloc((n, A, 2), np.int32), env.alloc((n, A), np.uint8), env.alloc((n, A), np.int32)
        act.from_host(np.zeros((n, A), np.int32))
        act2 = env.alloc((n, A), np.int32)
        for _ in range(args.warm_steps):
            env.partner_device(act)
            env.step_device(act, None, rew, term, trunc)
        env.partner_device(act, target, status)
        st = status.to_host()
        report.say("  status of the timed states: " + ", ".join(f"{name} {int((st == k).sum())}" for k, name in enumerate(partner.STATUS_NAMES)))

        def timed(leg, body, note=""):
            return report.row(leg, n, "call", replay(body, args.calls, args.replays, args.reps), note)

        with measure.graph_replay(env) as replay:
            step0 = timed("step_device, no observation", lambda: env.step_device(act, None, rew, term, trunc))
            timed("observe_grid_device bits", lambda: env.observe_grid_device(d_bits=bits), f"{bits.nbytes / 2**20:.2f} MiB written")
            timed("navigate_device T=1, action + steps", lambda: env.navigate_device(target, act, steps, T=1), "the partner's own targets")
            timed("partner_device agents=0b10, action", lambda: env.partner_device(act, agents=0b10), "one agent per env")
            timed("partner_device all agents, action", lambda: env.partner_device(act), f"{A} agents per env")
            timed("partner_device all agents, action + target + status", lambda: env.partner_device(act, target, status), f"{A} agents per env")

            def apart():                                               # the same two launches in turn, the step on a FIXED action buffer
                env.partner_device(act2)
                env.step_device(act, None, rew, term, trunc)

            timed("partner_device (into a spare buffer) + step_device on fixed actions", apart, "per step; the partner's actions are not played")

            def pair():
                env.partner_device(act)
                env.step_device(act, None, rew, term, trunc)

            both = timed("partner_device (action) + step_device, no observation", pair, "per step")
        report.say(f"  per step: partner + step {both:.3f} us  (step alone {step0:.3f} us)")
        if n <= args.host_envs:
            got = {}
            book = env.recipe_graphs
            parts = (lambda: got.update(recs=env.get_state()),
                     lambda: got.update(act=partner.host_partner(env.dims, env.layouts, got["recs"], book)[0]),
                     lambda: act.from_host(got["act"]))
            us = measure.host_clock(env, parts, 1, 3)
            for leg, part in zip(("get_state", "Python model (partner.host_partner)", "upload of the actions"), us):
                report.row(f"host route: {leg}", n, "call", part, "host clock")
            report.row("host route: get_state + partner.host_partner + upload", n, "call", [sum(p) for p in zip(*us)], "host clock")
        else:
            report.say(f"  host route: unmeasured at {n} envs (timed up to --host-envs {args.host_envs}; the Python model is linear in the envs)")
        env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
