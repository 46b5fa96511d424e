#!/usr/bin/env python3
"""What an action mask costs (cz_action_effects_device, k_action_effects):

  * config 2's shape (coop_test, 2 agents, scheme3): one call for one agent (agents=0b10) and for all agents, the mask alone and
    mask + effects, next to the one-step launch without an observation and navigate_device with one target per agent;
  * one scheme1 case (switch_test, 2 agents: 8 codes, 7 trials per agent) at the same sizes;
  * per step: action_effects_device(mask) -> masked argmax of random logits in torch -> step_device, the closed loop of a masked
    policy, captured with torch.cuda.graph;
  * the host route to the same answer: get_state + a host model (effects.host_effects over this project's test oracle) + upload of
    the mask, by the host's clock.

The states are those a few dozen steps of uniformly random play leave behind (auto-reset on).  Device figures: K calls captured
once into a graph on a stream of the caller and replayed; the time between two device events around the replays, per call, median
of `--reps` timed runs (min and max beside it).  A library without the entry point (the parent under --alternate) gives the step
and navigation rows only.  Writes profiles/r23/effects_sizes.txt.

    python3 tools/effects_sizes.py 4096 65536
"""
import os
import sys

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r23", "effects_sizes.txt"))
ap.add_argument("--calls", type=int, default=200, help="calls per captured graph")
ap.add_argument("--replays", type=int, default=5, help="graph launches per timed run")
ap.add_argument("--host-envs", type=int, default=4096, help="largest batch the host route is timed at")
ap.add_argument("--warm-steps", type=int, default=40, help="steps of random play before anything is timed")
ap.add_argument("--no-torch", action="store_true", help="leave the masked torch loop out (torch is then not loaded)")
ap.add_argument("sizes", type=int, nargs="*", default=[4096, 65536])


def legs(args, report):
    torch = None if args.no_torch else measure.torch_first()
    import numpy as np
    from cooking_zoo_amd import effects
    from cooking_zoo_amd.vec_env import CookingVecEnv
    A = measure.A
    have = measure.has_entry("cz_action_effects_device")
    report.say(f"action masks; {args.calls} calls per graph, {args.replays} launches per run, {args.reps} runs; us per call between two device "
               f"events" + ("" if have else "; this library has no cz_action_effects_device: step and navigation rows only"))
    cases = [("coop_test scheme3", lambda n: measure.make_env(n), 5),
             ("switch_test scheme1", lambda n: CookingVecEnv(n, "switch_test", "example", A, 400, ["MashedCarrotBanana", "TomatoSalad"],
                                                             action_scheme="scheme1", num_layouts=64, auto_reset=True), 8)]
    for n in args.sizes:
        for name, make, n_act in cases:
            env = make(n)
            env.reset(return_obs=False)
            report.say(f"\n{n} envs, {name}, {A} agents, {n_act} codes")
            act = env.alloc((n, A), np.int32)
            rew, term, trunc = env.alloc((n, A), np.float64), env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)
            mask, eff = env.alloc((n, A, n_act), np.uint8), env.alloc((n, A, n_act), np.uint8)
            target, steps = env.alloc((n, A, 2), np.int32), env.alloc((n, A), np.int32)
            rng = np.random.default_rng(1)
            for _ in range(args.warm_steps):
                act.from_host(rng.integers(0, n_act, size=(n, A), dtype=np.int32))
                env.step_device(act, None, rew, term, trunc)
            target.from_host(rng.integers(0, 7, size=(n, A, 2), dtype=np.int32))
            if have:
                env.action_effects_device(mask, eff)
                m, e = mask.to_host(), eff.to_host()
                report.say(f"  the timed states: {100 * (1 - m[:, :, 1:].mean()):.1f} % of the (agent, code >= 1) pairs are masked out; bits set in "
                           + ", ".join(f"{nm} {100 * ((e[:, :, 1:] & b) != 0).mean():.1f} %" for b, nm in effects.BIT_NAMES.items()))
            tag = f"{name}: "

            def timed(leg, body, note=""):
                return report.row(tag + leg, n, "call", replay(body, args.calls, args.replays, args.reps), note)

            with measure.graph_replay(env) as replay:
                step0 = timed("step_device, no observation", lambda: env.step_device(act, None, rew, term, trunc))
                timed("navigate_device T=1, action + steps", lambda: env.navigate_device(target, act, steps, T=1), "random targets")
                if have:
                    timed("action_effects_device agents=0b10, mask", lambda: env.action_effects_device(mask, agents=0b10), "one agent per env")
                    timed("action_effects_device agents=0b10, mask + effects", lambda: env.action_effects_device(mask, eff, agents=0b10), "one agent per env")
                    timed("action_effects_device all agents, mask", lambda: env.action_effects_device(mask), f"{A} agents per env")
                    timed("action_effects_device all agents, mask + effects", lambda: env.action_effects_device(mask, eff), f"{A} agents per env")
            if have and torch is not None and name.startswith("coop_test"):
                dev = torch.device("cuda", 0)
                K = 50
                logits = torch.randn((K, n, A, n_act), device=dev)
                t_mask = torch.ones((n, A, n_act), dtype=torch.uint8, device=dev)
                t_act = torch.zeros((n, A), dtype=torch.int32, device=dev)
                t_rew = torch.empty((n, A), dtype=torch.float64, device=dev)
                t_term, t_trunc = (torch.empty((n, A), dtype=torch.uint8, device=dev) for _ in range(2))
                cap = torch.cuda.Stream(device=dev)
                env.sync()
                torch.cuda.synchronize()
                env.set_stream(cap)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=cap):
                    for k in range(K):
                        env.action_effects_device(t_mask)
                        t_act.copy_(logits[k].masked_fill(~t_mask.bool(), float("-inf")).argmax(-1).to(torch.int32))
                        env.step_device(t_act, None, t_rew, t_term, t_trunc)
                with torch.cuda.stream(cap):
                    us = measure.torch_events(lambda: [graph.replay() for _ in range(args.replays)], K * args.replays, args.reps, warm=1)
                torch.cuda.synchronize()
                env.set_stream(None)
                both = report.row(tag + "action_effects_device + masked argmax (torch) + step_device", n, "step", us, f"{K} steps per torch.cuda.graph")
                report.say(f"  per step: mask + torch policy + step {both:.3f} us  (step alone, fixed actions {step0:.3f} us)")
                del graph
            if have and n <= args.host_envs:
                sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "tests"))
                import effects_common as ec                      # (the oracle's step as world_step: test infrastructure, not the package)
                got = {}
                parts = (lambda: got.update(recs=env.get_state()),
                         lambda: got.update(mask=effects.mask_of(ec.model(env, got["recs"]))),
                         lambda: mask.from_host(got["mask"]))
                us = measure.host_clock(env, parts, 1, 3)
                for leg, part in zip(("get_state", "host model (effects.host_effects over the C oracle)", "upload of the mask"), us):
                    report.row(tag + f"host route: {leg}", n, "call", part, "host clock")
                report.row(tag + "host route: get_state + host model + upload", n, "call", [sum(p) for p in zip(*us)], "host clock")
            elif have:
                report.say(f"  host route: unmeasured at {n} envs (timed up to --host-envs {args.host_envs})")
            env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
