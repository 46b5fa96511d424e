#!/usr/bin/env python3
"""What PPO's update phase costs on the device (cz_ppo_grad_device; cooking_zoo_amd/ppo.py) next to the same loss in torch, at
config 2's shape (coop_test, 2 agents, scheme3, F = 278, 5 actions): minibatches of 4096, 16 384 and 65 536 positions of a synthetic
trajectory of as many rows; medians per call between device events on one stream:

  ppo_grad_device, shared trunk   one call, both agents' policy and critic on set 0
  ppo_grad_device, own critic     ... the critic on set 1: a second hidden pass forward and a second pass backward
  torch float32 grad              the same loss (log_softmax, min, clamp, mse) on stacked float32 parameters, forward + backward()
  ... from a graph                the same captured once into a torch.cuda.graph and replayed
  update: device                  ppo_grad_device + Adam.step + load_policy + load_value
  update: torch                   forward + backward() + Adam.step + load_policy + load_value
  ... from a graph                either update from a torch.cuda.graph (Adam capturable)
  k_ppo_outer tile T              ppo_grad_device on the shared trunk under CZ_PPO_TILE=T: T features per workgroup of k_ppo_outer

Rows that need an entry point the measured library lacks are left out (the parent of this change has no cz_ppo_grad_device).

    python3 tools/ppo_sizes.py --alternate PARENT            # -> profiles/r35/ppo_sizes.txt
"""
import os

import measure

ap = measure.parser(__doc__, reps=7, out=os.path.join(measure.REPO, "profiles", "r35", "ppo_sizes.txt"), timeout=900)
ap.add_argument("--positions", type=int, nargs="+", default=[4096, 16384, 65536])
ap.add_argument("--launches", type=int, default=2)
A = measure.A
COEF = dict(clip=0.2, c_value=0.5, c_entropy=0.01)


def legs(args, report):
    torch = measure.torch_first()
    K = args.launches
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    with_ppo = measure.has_entry("cz_ppo_grad_device")
    env = measure.make_env(64, max_steps=100)
    F, Cn = env.F, env.num_actions

    def timed(name, n, body, note="", k=K):
        measure.times(body, 2)()
        side.synchronize()
        return report.row(name, n, "call", measure.torch_events(measure.times(body, k), k, args.reps), f"K={k} {note}".strip())

    def graphed(name, n, body, note="", k=K):
        body(0)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            body(0)
        timed(name, n, lambda i: g.replay(), note, k)
        del g

    with torch.cuda.stream(side):
        env.set_stream(torch.cuda.current_stream())
        torch.manual_seed(0)
        shapes = ((2, 64, F), (2, 64), (2, Cn, 64), (2, Cn), (2, 64), (2, 1))
        start = [torch.randn(s, device=dev) * k for s, k in zip(shapes, (0.05, 0.05, 0.1, 0.1, 0.1, 0.1))]
        params = [torch.nn.Parameter(p.clone()) for p in start]
        for p in params:
            p.grad = torch.zeros_like(p)
        env.load_policy(*params[:4])
        env.load_value(*params[4:])
        if with_ppo:
            env.ppo_reserve(max(args.positions))
        for n in args.positions:                                   # (the row format's "envs" column holds the positions)
            x = torch.randn((n, A, F), device=dev) * 0.5
            act = torch.randint(0, Cn, (n, A), device=dev, dtype=torch.int32)
            lp = torch.log(torch.full((n, A), 1.0 / Cn, device=dev)) + torch.randn((n, A), device=dev) * 0.25
            ad, rt = torch.randn((n, A), device=dev), torch.randn((n, A), device=dev)
            idx = torch.randperm(n, device=dev).to(torch.int32)
            act64 = act.long()

            def device_grad(vsets):
                return lambda i: env.ppo_grad_device(x, act, lp, ad, rt, [p.grad for p in params], d_index=idx, sets=(0, 0), vsets=vsets, rows=n, **COEF)

            def torch_grad(vset):
                w1, b1, w2, b2, wv, bv = params

                def body(i):
                    rows = x[idx.long()]                           # the minibatch's gather, as a learner has it
                    h = torch.relu(rows @ w1[0].T + b1[0])
                    logq = torch.log_softmax(h @ w2[0].T + b2[0], dim=-1)
                    ratio = torch.exp(logq.gather(-1, act64[idx.long()][..., None])[..., 0] - lp[idx.long()])
                    Adv = ad[idx.long()]
                    surr = torch.min(ratio * Adv, torch.clamp(ratio, 1.0 - COEF["clip"], 1.0 + COEF["clip"]) * Adv)
                    entropy = -(torch.exp(logq) * logq).sum(-1)
                    hv = h if vset == 0 else torch.relu(rows @ w1[vset].T + b1[vset])
                    v = hv @ wv[vset] + bv[vset]
                    loss = -surr.mean() - COEF["c_entropy"] * entropy.mean() + COEF["c_value"] * 0.5 * torch.nn.functional.mse_loss(v, rt[idx.long()])
                    for p in params:
                        p.grad.zero_()
                    loss.backward()
                return body

            def update(grad, opt):
                return lambda i: (grad(i), opt.step(), env.load_policy(*params[:4]), env.load_value(*params[4:]))

            def fresh():
                with torch.no_grad():
                    for p, s in zip(params, start):
                        p.copy_(s)
                return torch.optim.Adam(params, lr=3e-4, capturable=True)

            for what, vset in (("shared trunk", 0), ("own critic", 1)):
                if with_ppo:
                    timed(f"ppo_grad_device, {what}", n, device_grad((vset, vset)))
                    graphed(f"ppo_grad_device, {what}, from a graph", n, device_grad((vset, vset)))
                timed(f"torch float32 grad, {what}", n, torch_grad(vset))
                graphed(f"torch float32 grad, {what}, from a graph", n, torch_grad(vset))
                if with_ppo:
                    timed(f"update: device, {what}", n, update(device_grad((vset, vset)), fresh()))
                    graphed(f"update: device, {what}, from a graph", n, update(device_grad((vset, vset)), fresh()))
                timed(f"update: torch, {what}", n, update(torch_grad(vset), fresh()))
                graphed(f"update: torch, {what}, from a graph", n, update(torch_grad(vset), fresh()))
            del x
        side.synchronize()
        # the k_ppo_outer instances: a small handle each (CZ_PPO_TILE is read when a handle is made)
        if with_ppo:
            for tile in (16, 32, 64):
                os.environ["CZ_PPO_TILE"] = str(tile)
                small = measure.make_env(64, max_steps=100)
                os.environ.pop("CZ_PPO_TILE")
                small.set_stream(torch.cuda.current_stream())
                small.load_policy(*params[:4])
                small.load_value(*params[4:])
                small.ppo_reserve(max(args.positions))
                for n in args.positions:
                    x = torch.randn((n, A, F), device=dev) * 0.5
                    act = torch.randint(0, Cn, (n, A), device=dev, dtype=torch.int32)
                    lp, ad, rt = (torch.randn((n, A), device=dev) for _ in range(3))
                    timed(f"k_ppo_outer tile {tile}: ppo_grad_device, shared trunk", n,
                          lambda i: small.ppo_grad_device(x, act, lp, ad, rt, [p.grad for p in params], sets=(0, 0), vsets=(0, 0), rows=n, **COEF))
                    del x
                side.synchronize()
                small.set_stream(None)
                small.close()
    env.set_stream(None)
    env.close()


if __name__ == "__main__":
    measure.main(ap, legs, __file__)
