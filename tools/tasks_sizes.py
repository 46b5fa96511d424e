#!/usr/bin/env python3
"""What the task calls cost, timed with device events on the handle's stream (config 2's shape: coop_test, 2 agents, scheme3, F = 278):

  one call      K calls between two events of `set_tasks_device` with a mask that chooses 0 %, 1 %, 10 % and 100 % of the envs (the same
                envs in every call: a chosen env is re-evaluated whatever its state, so every call does the same work), with the ids in
                an array and drawn from a 3-row task list, and of `infos_device` with `goal32` alone and with all five outputs; next to
                them, on the same handle, the one-step launch without an observation, `reset_device` with the same masks' 100 % row and
                `observe_grid_device(bits)`
  loop          step_device_f32 + reset_device() + set_tasks_device(list) + infos_device(goal32) per step on a handle with auto_reset off
                and short episodes (--max-steps), against the same loop without the two new calls
  host route    get_state + tasks.host_set_tasks + tasks.host_infos + set_state for the envs at t == 0 of a fresh batch, by the host's clock
                (--host-envs, default the smallest size; the Python model dominates)

Writes every line to --out (default profiles/r27/tasks_sizes.txt).  Needs a GPU; nothing is estimated without one.

    python3 tools/tasks_sizes.py 4096 65536
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r27", "tasks_sizes.txt"))
ap.add_argument("envs", type=int, nargs="*", default=[4096, 65536])
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--max-steps", type=int, default=50, help="episode length of the loop legs")
ap.add_argument("--host-envs", type=int, default=None, help="batch size of the host route (default: the smallest of `envs`; 0: leave it out)")
A = measure.A
TASK_LIST = [[0, 1, 255, 255], [3, 2, 255, 255], [1, 5, 255, 255]]


def buffers(env):
    import numpy as np
    n = env.num_envs
    b = measure.step_buffers(env, 8, 1, ("obs32", "rew", "term", "trunc"))
    b.update(mask=env.alloc((n,), np.uint8), ids=env.alloc((n, 4), np.uint8), list=env.alloc((len(TASK_LIST), 4), np.uint8),
             goal8=env.alloc((n, A, env.num_goals), np.uint8), goal32=env.alloc((n, A, env.num_goals), np.float32),
             done=env.alloc((n, A), np.uint8), task=env.alloc((n, A), np.int32), t=env.alloc((n,), np.int32),
             bits=env.alloc((n,) + env.grid_shape()[:2] + (1,), np.uint32))
    b["list"].from_host(np.array(TASK_LIST, dtype=np.uint8))
    ids = np.full((n, 4), 0xFF, dtype=np.uint8)
    ids[:, :A] = np.random.default_rng(3).integers(0, len(env.book_names), (n, A))
    b["ids"].from_host(ids)
    return b


def one_call(n, args, report):
    import numpy as np
    env = measure.make_env(n, auto_reset=False)
    b, K = buffers(env), args.launches
    act = lambda k: b["act"].ptr + (k % 8) * n * A * 4
    ones = np.ones(n, dtype=np.uint8)

    def everybody():                  # every env alive and young: the step leg never meets a frozen env
        b["mask"].from_host(ones)
        env.reset_device(b["mask"])

    timed = lambda call, before=None: measure.handle_events(env, measure.times(call, K), K, args.reps, before, warm=args.reps)
    report.row("one step, no observation", n, "launch", timed(lambda k: env.step_device(act(k), None, b["rew"], b["term"], b["trunc"]), everybody))
    report.row("observe_grid_device bits", n, "call", timed(lambda k: env.observe_grid_device(d_bits=b["bits"])))
    if not measure.has_entry("cz_set_tasks_device"):            # (the parent's library in an --alternate run: the rows above only)
        env.close()
        return
    report.row("infos_device goal32", n, "call", timed(lambda k: env.infos_device(d_goal32=b["goal32"])))
    report.row("infos_device all five outputs", n, "call",
               timed(lambda k: env.infos_device(b["goal8"], b["goal32"], b["done"], b["task"], b["t"])))
    for percent in (0, 1, 10, 100):
        mask = np.zeros(n, dtype=np.uint8)
        mask[np.random.default_rng(2).permutation(n)[:n * percent // 100]] = 1
        b["mask"].from_host(mask)
        chosen = f"{percent} % chosen ({int(mask.sum())})"
        report.row(f"set_tasks_device ids {chosen}", n, "call", timed(lambda k: env.set_tasks_device(b["mask"], b["ids"])))
        report.row(f"set_tasks_device list {chosen}", n, "call", timed(lambda k: env.set_tasks_device(b["mask"], None, b["list"], seed=5)))
        if percent == 100:
            report.row(f"reset_device no rows {chosen}", n, "call", timed(lambda k: env.reset_device(b["mask"])))
    env.close()


def loop(n, args, report):
    K = args.launches
    for name, with_tasks in (("step_device_f32 + reset_device() + set_tasks_device(list) + infos_device(goal32)", True),
                             ("step_device_f32 + reset_device()", False)):
        if with_tasks and not measure.has_entry("cz_set_tasks_device"):
            continue
        env = measure.make_env(n, args.max_steps, auto_reset=False)
        b = buffers(env)

        def it(k):
            env.step_device_f32(b["act"].ptr + (k % 8) * n * A * 4, b["obs32"], b["rew"], b["term"], b["trunc"])
            env.reset_device(None, None, None, b["obs32"])
            if with_tasks:
                env.set_tasks_device(None, None, b["list"], seed=5)
                env.infos_device(d_goal32=b["goal32"])

        measure.handle_events(env, measure.times(it, K), K, args.reps)               # warm-up: one whole pass, dropped
        report.row(f"loop: {name}", n, "iteration", measure.handle_events(env, measure.times(it, K), K, args.reps), f"episodes of {args.max_steps}")
        env.close()


def host_route(n, args, report):
    import numpy as np
    from cooking_zoo_amd import soa, tasks
    env = measure.make_env(n, auto_reset=False)
    task_list = np.array(TASK_LIST, dtype=np.uint8)

    def route():
        recs = env.get_state()
        new, _ = tasks.host_set_tasks(env.tables, recs, recs[:, soa.W_T] == 0, task_list=task_list, seed=5)
        tasks.host_infos(env.tables, new)
        env.set_state(new)

    report.row("host route: get_state + tasks.host_set_tasks + tasks.host_infos + set_state", n, "call", measure.host_clock(env, route, 1, 3, warm=1))
    env.close()


def legs(args, report):
    for n in args.envs:
        one_call(n, args, report)
        loop(n, args, report)
    host_n = min(args.envs) if args.host_envs is None else args.host_envs
    if host_n and measure.has_entry("cz_set_tasks_device"):
        host_route(host_n, args, report)


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
