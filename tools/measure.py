"""How this project times things: config 2's workload, four timers, one row format and its inverse, the choice of the library that
is measured, and the parent / change driver with its band summary.  The timing tools next to this file are their legs and nothing
else.  Importable without a GPU and without the built library: the package and torch are touched inside functions only."""
import argparse
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, RECIPES = 2, ["TomatoLettuceSalad", "CarrotBanana"]


# ---------------------------------------------------------------- which library is measured
def parser(doc, reps, out=None, timeout=400):
    """every timing tool's parser: the tool adds its own arguments to it"""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=REPO, help="the checkout whose package and built library are measured (default: this one)")
    ap.add_argument("--lib", default=os.environ.get("CZ_LIB"), help="a library loaded into that package instead of its own (CZ_LIB)")
    ap.add_argument("--label", default="change")
    ap.add_argument("--reps", type=int, default=reps, help="timed runs per row")
    ap.add_argument("--out", default=out, help="every line is also written here")
    ap.add_argument("--alternate", metavar="OTHER", help="the driver: OTHER (a built checkout or a .so) as parent and this selection "
                    "as change, alternated in fresh child processes; rows, summary and bands go to --out")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=timeout, help="seconds one child of --alternate may take")
    return ap


def select(args):
    """make `import cooking_zoo_amd` find --tree's package, and that package --lib's library"""
    if args.lib:
        os.environ["CZ_LIB"] = os.path.abspath(args.lib)
    else:
        os.environ.pop("CZ_LIB", None)
    sys.path.insert(0, os.path.abspath(args.tree))


def has_entry(name):
    from cooking_zoo_amd import _native
    return hasattr(C.CDLL(_native.LIB_PATH), name)          # (_native.lib() itself stands a raising stub in for a missing one)


def torch_first():
    """torch before the library loads: its bundled HIP runtime then serves both (_native._LateTorchGuard)"""
    import torch
    torch.cuda.init()
    return torch


def main(ap, legs, script):
    """a tool's entry: `legs(args, report)` in this process, or the driver over children of `script`"""
    args = ap.parse_args()
    if args.alternate:
        sys.exit(alternate(script, args.alternate, args.pairs, passthrough(sys.argv[1:]), args.timeout, args.out))
    select(args)
    report = Report(args.out, args.label)
    legs(args, report)
    report.write()


# ---------------------------------------------------------------- workload: config 2's shape
def make_env(n, max_steps=400, num_layouts=64, auto_reset=True, **kw):
    from cooking_zoo_amd.vec_env import CookingVecEnv
    env = CookingVecEnv(n, "coop_test", "example", A, max_steps, RECIPES, action_scheme="scheme3", num_layouts=num_layouts,
                        auto_reset=auto_reset, **kw)
    env.reset(return_obs=False)
    return env


def step_buffers(env, periods=1, seed=0, forms=("obs", "rew", "term", "trunc")):
    """`act`, a ring of `periods` seeded action slots, then of `rew`, `term`, `trunc`, `obs` (float64 rows), `obs32` and `codes`
    those named, allocated in the order given.  `seed` may be a Generator that several rings draw from in turn."""
    import numpy as np
    n = env.num_envs
    shapes = dict(rew=((n, A), np.float64), term=((n, A), np.uint8), trunc=((n, A), np.uint8), obs=((n, A, env.F), np.float64),
                  obs32=((n, A, env.F), np.float32), codes=((n, A, env.codes_pitch), np.uint8))
    b = dict(act=env.alloc((periods, n, A), np.int32))
    b["act"].from_host(np.random.default_rng(seed).integers(0, 5, size=(periods, n, A), dtype=np.int32))
    for form in forms:
        b[form] = env.alloc(*shapes[form])
    return b


def times(fn, k):
    """the body `fn(0) .. fn(k - 1)`"""
    def body():
        for i in range(k):
            fn(i)
    return body


# ---------------------------------------------------------------- the four timers: us per unit, one entry per timed run, unsorted
def handle_events(env, body, units, reps, before=None, warm=0):
    """the handle's own device events on its stream: cz_timer_start, body(), cz_timer_stop; `before()` runs ahead of each start,
    the first `warm` runs are dropped"""
    from cooking_zoo_amd import _native
    L, us, ms = _native.lib(), [], C.c_float()
    for _ in range(warm + reps):
        if before:
            before()
        _native.check(env._h, L.cz_timer_start(env._h))
        body()
        _native.check(env._h, L.cz_timer_stop(env._h, C.byref(ms)))
        us.append(ms.value * 1e3 / units)
    return us[warm:]


def torch_events(body, units, reps, warm=0):
    """torch events on the current stream around body()"""
    import torch
    us = []
    for _ in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        body()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / units)
    return us[warm:]


@contextlib.contextmanager
def graph_replay(env):
    """Yields `replay(body, calls, replays, reps)`: `calls` x body() captured once into a graph on a stream made for the env,
    `replays` launches of the graph between two HIP events per run, one warming run dropped.  On leaving, the env has its own
    stream back, and the events and the stream are destroyed, as every graph is after its runs."""
    from cooking_zoo_amd import _native
    rccl, path = C.create_string_buffer(512), C.create_string_buffer(512)
    _native.lib().cz_runtime_paths(rccl, path, 512)
    hip = C.CDLL(path.value.decode())

    def ck(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def replay(body, calls, replays, reps):
        graph, gexec, ms, us = C.c_void_p(), C.c_void_p(), C.c_float(), []
        ck(hip.hipStreamBeginCapture(stream, 0))
        for _ in range(calls):
            body()
        ck(hip.hipStreamEndCapture(stream, C.byref(graph)))
        ck(hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)))
        for _ in range(1 + reps):
            ck(hip.hipEventRecord(ev[0], stream))
            for _ in range(replays):
                ck(hip.hipGraphLaunch(gexec, stream))
            ck(hip.hipEventRecord(ev[1], stream))
            ck(hip.hipEventSynchronize(ev[1]))
            ck(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
            us.append(ms.value * 1e3 / (replays * calls))
        ck(hip.hipGraphExecDestroy(gexec))
        ck(hip.hipGraphDestroy(graph))
        return us[1:]

    stream, ev = C.c_void_p(), [C.c_void_p(), C.c_void_p()]
    ck(hip.hipStreamCreateWithFlags(C.byref(stream), 1))
    for e in ev:
        ck(hip.hipEventCreate(C.byref(e)))
    env.set_stream(stream)
    try:
        yield replay
    finally:
        env.set_stream(None)
        for e in ev:
            ck(hip.hipEventDestroy(e))
        ck(hip.hipStreamDestroy(stream))


def host_clock(env, body, units, reps, warm=0):
    """the host's clock around body() + env.sync().  A tuple of bodies is alternated run by run, each timed on its own (one's end
    is the next one's start), and one list per body comes back."""
    bodies = body if isinstance(body, tuple) else (body,)
    us = [[] for _ in bodies]
    env.sync()
    for _ in range(warm + reps):
        for out, one in zip(us, bodies):
            t0 = time.perf_counter()
            one()
            env.sync()
            out.append((time.perf_counter() - t0) * 1e6 / units)
    us = [u[warm:] for u in us]
    return us if isinstance(body, tuple) else us[0]


# ---------------------------------------------------------------- one line format and its inverse
def median(us):
    return sorted(us)[len(us) // 2]


def format_row(label, leg, n, unit, us, note=""):
    return (f"{label:7s} | {leg:58s} | {n:6d} envs | us per {unit:9s} | min {min(us):9.3f} | median {median(us):9.3f} | max {max(us):9.3f} | runs "
            + " ".join(f"{u:.3f}" for u in us) + (f" | {note}" if note else ""))


ROW = re.compile(r"^(.*?) *\| (.*?) *\| *(\d+) envs \| us per (.*?) *\| min +[\d.]+ \| median +[\d.]+ \| max +[\d.]+ \| runs ([\d. ]+?)(?: \| (.*))?$")


def parse_row(line):
    """(label, leg, n, unit, us, note) of a format_row line, None of any other"""
    m = ROW.match(line)
    return m and (m[1], m[2], int(m[3]), m[4], [float(u) for u in m[5].split()], m[6] or "")


class Report:
    """prints lines as they come, keeps them, writes them to `out` at the end"""

    def __init__(self, out, label=""):
        self.out, self.label, self.lines = out, label, []

    def say(self, line=""):
        print(line, flush=True)
        self.lines.append(line)

    def row(self, leg, n, unit, us, note=""):
        self.say(format_row(self.label, leg, n, unit, us, note))
        return median(us)

    def write(self):
        if self.out:
            os.makedirs(os.path.dirname(os.path.abspath(self.out)), exist_ok=True)
            with open(self.out, "w") as f:
                f.write("\n".join(self.lines) + "\n")


# ---------------------------------------------------------------- the A/B driver and its summary
def passthrough(argv):
    """a tool's own arguments: the command line without what the driver sets for each child"""
    own, skip = [], False
    for a in argv:
        if skip or a.split("=")[0] in ("--alternate", "--pairs", "--out", "--label", "--timeout"):
            skip = not skip and "=" not in a
            continue
        own.append(a)
    return own


def holds(parent_us, change_median):
    """profiles/r18/README.md: a row holds when the change's median lies inside the parent's min-max band of the same round,
    widened by the band's width on either side.  Returns (holds, band low, band high)."""
    lo, hi = min(parent_us), max(parent_us)
    lo, hi = lo - (hi - lo), hi + (hi - lo)
    return lo <= change_median <= hi, lo, hi


def summary(runs):
    """lines over `runs`, [(label, [parsed row, ...]), ...] in run order, consecutive runs being the pairs"""
    keys, medians = [], {}
    for label, rows in runs:
        for _, leg, n, _, us, _ in rows:
            if (leg, n) not in keys:
                keys.append((leg, n))
            medians.setdefault((leg, n, label), []).append(median(us))
    lines = ["# summary: every run's median in run order; spread = max - min between the runs of the same label"]
    for leg, n in keys:
        mean = {}
        for label in ("parent", "change"):
            m = medians.get((leg, n, label))
            if m:
                mean[label] = sum(m) / len(m)
                lines.append(f"{leg} | {n} envs | {label:7s} | " + " ".join(f"{x:.3f}" for x in m) + f" | spread {max(m) - min(m):.3f} | mean {mean[label]:.3f}")
        if len(mean) == 2:
            lines.append(f"{leg} | {n} envs | change - parent (means) | {mean['change'] - mean['parent']:+.3f} us")
    lines += ["# bands: us, min / median / max; band = parent min - width .. parent max + width, width = parent max - parent min",
              "| pair | row | parent | change | band | holds |", "|---|---|---|---|---|---|"]
    count = outside = 0
    for pair in range(len(runs) // 2):
        side = {label: {(r[1], r[2]): r[4] for r in rows} for label, rows in runs[2 * pair:2 * pair + 2]}
        for key, p in side.get("parent", {}).items():
            c = side.get("change", {}).get(key)
            if c:
                ok, lo, hi = holds(p, median(c))
                count, outside = count + 1, outside + (not ok)
                lines.append(f"| {pair + 1} | {key[0]}, {key[1]} envs | {min(p):.3f} / {median(p):.3f} / {max(p):.3f} | "
                             f"{min(c):.3f} / {median(c):.3f} / {max(c):.3f} | {lo:.3f} .. {hi:.3f} | {'yes' if ok else '**no**'} |")
    return lines + [f"{count} rows, {outside} outside"]


def alternate(script, other, pairs, passthrough_args, timeout_s, out):
    """Fresh children of `script`, one at a time: parent (`other`: a built checkout, or a .so for this tree's package), change,
    `pairs` times, then once more in the reverse order.  After a child that fails, dies of a signal or runs into `timeout_s`
    nothing more is started: a card that has faulted gets no further work.  Returns 0 only if every child ran to the end."""
    parent = ["--tree", other, "--lib="] if os.path.isdir(other) else ["--lib", other]
    order = [("parent", parent), ("change", [])]
    report, runs, bad = Report(out), [], None
    for i, (label, which) in enumerate(order * pairs + order[::-1]):
        report.say(f"# run {i}: {label}")
        cmd = [sys.executable, os.path.abspath(script)] + list(passthrough_args) + which + ["--label", label, "--out="]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s)
            stdout, stderr, rc = p.stdout, p.stderr, p.returncode
            bad = f"status {rc}" if rc > 0 else f"signal {-rc}" if rc < 0 else None
        except subprocess.TimeoutExpired as e:
            stdout, stderr = (s.decode(errors="replace") if isinstance(s, bytes) else s or "" for s in (e.stdout, e.stderr))
            bad = f"timeout after {timeout_s} s"
        for line in stdout.rstrip().split("\n"):
            report.say(line)
        runs.append((label, [r for r in map(parse_row, stdout.split("\n")) if r]))
        if bad:
            report.say(f"# run {i} ended with {bad}: nothing more is started\n{stderr[-2000:]}")
            break
    if not bad:
        for line in summary(runs):
            report.say(line)
    report.write()
    return 1 if bad else 0
