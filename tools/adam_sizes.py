#!/usr/bin/env python3
"""What the optimiser on the device costs (cz_adam_step_device; cooking_zoo_amd/adam.py) next to the route the library offered
before it - clip_grad_norm_ + torch.optim.Adam(capturable=True).step() + load_policy + load_value - at config 2's shape (coop_test, 2
agents, scheme3, F = 278, 5 actions) with 1 and 4 loaded weight sets; medians per call between device events on one stream.  The legs
of one table are ALTERNATED run by run in one process (run r of every leg before run r + 1 of any), so that a drift of the box
moves them alike:

  adam_step_device                     one call, no clipping
  adam_step_device, clipped            ... with max_norm = 0.5
  ... from a graph                     the same captured once into a torch.cuda.graph and replayed
  torch: Adam + loads                  Adam.step + load_policy + load_value
  torch: clip + Adam + loads           clip_grad_norm_ + Adam.step + load_policy + load_value, eager and from a graph
  update: device                       ppo_grad_device + Adam.step + load_policy + load_value (profiles/r35's leg, measured again here)
  update: device + adam_step_device    ppo_grad_device + adam_step_device: the two-call minibatch step
  ... clipped                          either update with clipping to 0.5

    python3 tools/adam_sizes.py                              # -> profiles/r36/adam_sizes.txt
"""
import os

import measure

ap = measure.parser(__doc__, reps=9, out=os.path.join(measure.REPO, "profiles", "r36", "adam_sizes.txt"), timeout=900)
ap.add_argument("--positions", type=int, nargs="+", default=[4096, 16384, 65536])
ap.add_argument("--sets", type=int, nargs="+", default=[1, 4])
ap.add_argument("--launches", type=int, default=4)
A = measure.A
COEF = dict(clip=0.2, c_value=0.5, c_entropy=0.01)
ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-5)


def legs(args, report):
    torch = measure.torch_first()
    K = args.launches
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    if not measure.has_entry("cz_adam_step_device"):
        report.say("# this library has no cz_adam_step_device: nothing to time")
        return
    env = measure.make_env(64, max_steps=100)
    F, Cn = env.F, env.num_actions

    def alternated(table, n, unit="call"):
        """table: [(name, body(i), note)]; run r of every leg, then run r + 1"""
        runs = {name: [] for name, _, _ in table}
        for name, body, _ in table:                                # warm every leg
            measure.times(body, 2)()
        side.synchronize()
        for _ in range(args.reps):
            for name, body, _ in table:
                runs[name] += measure.torch_events(measure.times(body, K), K, 1)
        return {name: report.row(name, n, unit, runs[name], f"K={K} {note}".strip()) for name, _, note in table}

    def graph_of(body):
        body(0)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            body(0)
        return g

    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        torch.manual_seed(0)
        env.adam_reserve()
        for n_sets in args.sets:
            shapes = ((n_sets, 64, F), (n_sets, 64), (n_sets, Cn, 64), (n_sets, Cn), (n_sets, 64), (n_sets, 1))
            start = [torch.randn(s, device=dev) * k for s, k in zip(shapes, (0.05, 0.05, 0.1, 0.1, 0.1, 0.1))]
            params = [torch.nn.Parameter(p.clone()) for p in start]
            for p in params:
                p.grad = torch.randn_like(p) * 0.05
            m, v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
            state = torch.tensor([0, 1, 1, 0, 0, 0, 0, 0], dtype=torch.float64, device=dev)
            env.load_policy(*params[:4])
            env.load_value(*params[4:])
            grads = [p.grad for p in params]

            def device_step(max_norm):
                return lambda i: env.adam_step_device(params, grads, m, v, state, max_norm=max_norm, **ADAM)

            def torch_step(opt, max_norm):
                def body(i):
                    if max_norm:
                        torch.nn.utils.clip_grad_norm_(params, max_norm)
                    opt.step()
                    env.load_policy(*params[:4])
                    env.load_value(*params[4:])
                return body

            def fresh():
                return torch.optim.Adam(params, lr=ADAM["lr"], betas=ADAM["betas"], eps=ADAM["eps"], capturable=True)

            # ---- the optimiser alone
            report.say(f"# the optimiser alone, {n_sets} loaded set(s), {sum(p.numel() for p in params)} parameters; the rows' count column holds the sets")
            eager_plain, eager_clip = torch_step(fresh(), 0.0), torch_step(fresh(), 0.5)
            graphs = [graph_of(device_step(0.0)), graph_of(device_step(0.5)), graph_of(torch_step(fresh(), 0.0)), graph_of(torch_step(fresh(), 0.5))]
            med = alternated([("adam_step_device", device_step(0.0), ""),
                              ("adam_step_device, clipped", device_step(0.5), ""),
                              ("adam_step_device, from a graph", lambda i: graphs[0].replay(), ""),
                              ("adam_step_device, clipped, from a graph", lambda i: graphs[1].replay(), ""),
                              ("torch: Adam + loads", eager_plain, ""),
                              ("torch: clip + Adam + loads", eager_clip, ""),
                              ("torch: Adam + loads, from a graph", lambda i: graphs[2].replay(), ""),
                              ("torch: clip + Adam + loads, from a graph", lambda i: graphs[3].replay(), "")], n_sets)
            for mine, theirs in (("adam_step_device, from a graph", "torch: Adam + loads, from a graph"),
                                 ("adam_step_device, clipped, from a graph", "torch: clip + Adam + loads, from a graph"),
                                 ("adam_step_device", "torch: Adam + loads"), ("adam_step_device, clipped", "torch: clip + Adam + loads")):
                report.say(f"# {n_sets} set(s): {theirs} / {mine} = {med[theirs] / med[mine]:.2f}")
            del graphs
            side.synchronize()

            # ---- the whole update
            env.ppo_reserve(max(args.positions))
            for n in args.positions:
                x = torch.randn((n, A, F), device=dev) * 0.5
                act = torch.randint(0, Cn, (n, A), device=dev, dtype=torch.int32)
                lp = torch.log(torch.full((n, A), 1.0 / Cn, device=dev)) + torch.randn((n, A), device=dev) * 0.25
                ad, rt = torch.randn((n, A), device=dev), torch.randn((n, A), device=dev)
                idx = torch.randperm(n, device=dev).to(torch.int32)

                def grad(i):
                    env.ppo_grad_device(x, act, lp, ad, rt, grads, d_index=idx, sets=(0, 0), vsets=(0, 0), rows=n, **COEF)

                def both(second):
                    return lambda i: (grad(i), second(i))

                report.say(f"# the whole update, {n_sets} loaded set(s), {n} positions, shared trunk on set 0")
                bodies = [("update: device (torch Adam + loads)", both(torch_step(fresh(), 0.0))),
                          ("update: device + adam_step_device", both(device_step(0.0))),
                          ("update: device (torch clip + Adam + loads), clipped", both(torch_step(fresh(), 0.5))),
                          ("update: device + adam_step_device, clipped", both(device_step(0.5)))]
                graphs = [graph_of(body) for _, body in bodies]
                table = [(name, body, f"{n_sets} sets") for name, body in bodies]
                table += [(name + ", from a graph", (lambda g: lambda i: g.replay())(g), f"{n_sets} sets") for (name, _), g in zip(bodies, graphs)]
                table.insert(0, ("ppo_grad_device alone", grad, f"{n_sets} sets"))
                alternated(table, n)
                del graphs, x
                side.synchronize()
    env.set_stream(None)
    env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
