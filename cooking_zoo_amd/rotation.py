"""Layout rotation (CookingVecEnv.rotate_layouts): `Rotation` is the schedule - when the envs switch to the next part of the
pool and when the retired part may be refilled -, `DeviceRefill` and `ProcessRefill` are the two places a refill can come
from.  A source has `start()`, `refill(env, part, r)` -> done or not ready, `stop()` and `ready()`.  None of them keeps the
env, which owns the rotation and is handed in (so an env that is dropped still goes away at once, and stops its producer).
Nothing here touches the device library: the producer process imports this module in a fresh interpreter.
"""
from __future__ import annotations

import queue as _queue
import random as _random
import threading as _threading

import numpy as np

from cooking_zoo_amd import partner as _partner, soa
from cooking_zoo_amd.cooking_world.engine import load_level as _ll


def produce_layouts(q, stop, level_objects, meta, num_agents, dims_tuple, pool_slices, groups, seed, start=0):
    """Body of the layout-rotation process (CookingVecEnv.rotate_layouts): batch b refills part (start + b) % groups of every
    level's pool slice (`start` = the part the envs drew from when the rotation began: the first one to be retired); its
    layouts come from random.Random streams keyed by (seed, b, level), so a run can be replayed."""
    dims = soa.Dims(*dims_tuple)
    b = 0
    while not stop.is_set():
        g = (start + b) % groups
        batch = []
        for li, lv in enumerate(level_objects):
            base, count = pool_slices[li]
            sub = count // groups
            rng = _random.Random((int(seed) * 1000003 + b) * 101 + li)
            lays = [_ll.instantiate(lv, meta, num_agents, rng) for _ in range(sub)]
            first = base + g * sub
            recs = np.stack([l.init_record(dims, first + k) for k, l in enumerate(lays)])
            desc = np.stack([l.obs_descriptor(meta, dims) for l in lays])
            ranks = np.stack([_partner.rank_table(l) for l in lays])
            batch.append((first, lays, recs, desc, ranks))
        while not stop.is_set():
            try:
                q.put(batch, timeout=0.1)
                break
            except _queue.Full:
                pass
        b += 1


class Rotation:
    """The schedule: every `every` steps (at the next call boundary) the envs switch to the next of `groups` parts, and
    max_steps + 2 steps later - once the episodes that started on the retired part are over - `source` refills it."""

    def __init__(self, source, every, groups, start, steps):
        self.source, self.every, self.groups, self.start = source, int(every), int(groups), int(start)
        self.flip_due, self.refill_due, self.n_refills = int(steps) + self.every, None, 0

    def advanced(self, env):
        """the env's step count has moved: refill when due, then switch when due (at most one of each per call)"""
        if self.refill_due is not None and env._steps >= self.refill_due:
            # the part retired by the last switch
            if not self.source.refill(env, (self.start + self.n_refills) % self.groups, self.n_refills + 1):
                return                                              # not ready: next call, and the switch waits with it
            self.refill_due = None
            self.n_refills += 1
        if self.refill_due is None and env._steps >= self.flip_due:
            old = env._lay_active
            if old != (self.start + self.n_refills) % self.groups:      # the part the source's next refill is made for
                env.stop_rotation()
                raise RuntimeError("rotate_layouts: the active layout group was changed behind the rotation's back "
                                   "(set_layout_group while rotate_layouts runs); rotation stopped")
            env.set_layout_group(self.groups, (old + 1) % self.groups)
            self.refill_due = env._steps + env.max_steps + 2
            self.flip_due = env._steps + self.every


class DeviceRefill:
    """Refill number r is `generate_layouts` of the part with generation r under `seed`: launches on the env's own stream,
    nothing to start, stop or wait for."""

    def __init__(self, groups, seed):
        self.groups, self.seed = int(groups), int(seed)

    def start(self):
        pass

    def refill(self, env, part, r):
        for base, count in env.pool_slices:
            sub = count // self.groups
            env.generate_layouts(base + part * sub, sub, r, seed=self.seed, mirror=False)
        return True

    def stop(self):
        pass

    def ready(self):
        return 0


class ProcessRefill:
    """Refills come from a producer process (`produce_layouts`), in the order it makes them.  The instantiation is plain
    Python (engine/load_level.py, the reference's draw order) and takes milliseconds per batch: in a thread it would hold
    the interpreter lock against the thread that issues the steps, so it runs in a process of its own and hands finished
    arrays over `queue`.  A small thread takes the batches off that queue (unpickling costs a millisecond) into the local
    `ready` one, which is bounded: when it is full everything upstream sleeps."""

    def __init__(self, process, queue, stop_event, ready, blocking):
        self.process, self.queue, self.stop_event, self.ready_queue = process, queue, stop_event, ready
        self.blocking, self.dead_polls = bool(blocking), 0
        self.drain = _threading.Thread(target=self._drain, name="cz-layout-rotation-drain", daemon=True)

    @classmethod
    def spawn(cls, producer_args, prefetch, blocking):
        """the source over a producer process of its own (spawned: a fresh interpreter that never loads the HIP library);
        `producer_args`: what `produce_layouts` takes after the queue and the stop event"""
        import multiprocessing as _mp
        ctx = _mp.get_context("spawn")
        q, stop = ctx.Queue(maxsize=max(1, int(prefetch))), ctx.Event()
        process = ctx.Process(target=produce_layouts, name="cz-layout-rotation", daemon=True, args=(q, stop) + tuple(producer_args))
        return cls(process, q, stop, _queue.Queue(maxsize=max(1, int(prefetch))), blocking)

    def start(self):
        self.process.start()
        self.drain.start()

    def _drain(self):
        batch = None
        while not self.stop_event.is_set():
            try:
                if batch is None:
                    batch = self.queue.get(timeout=0.1)
                self.ready_queue.put(batch, timeout=0.1)
                batch = None
            except (_queue.Empty, _queue.Full):
                pass
            except (EOFError, OSError):
                return

    def _pending(self):
        """a batch still on its way from the producer's queue to the local one"""
        try:
            return not self.queue.empty()
        except (OSError, ValueError):
            return False

    def refill(self, env, part, r):
        batch = None
        while batch is None:
            try:
                # (blocking: waits for the producer if it is behind - in slices, so that a producer that died is noticed)
                batch = self.ready_queue.get(timeout=0.25) if self.blocking else self.ready_queue.get_nowait()
            except _queue.Empty:
                dead = not self.process.is_alive() and self.ready_queue.empty() and not self._pending()
                self.dead_polls = self.dead_polls + 1 if dead else 0      # (twice in a row: a batch may be in the drain thread's hands)
                if self.dead_polls >= 2:
                    code = self.process.exitcode
                    env.stop_rotation()
                    raise RuntimeError(f"rotate_layouts: the layout producer process died (exit code {code}); rotation stopped, "
                                       f"the envs keep drawing from part {env._lay_active} of {env._lay_groups}")
                if not self.blocking:
                    return False
        for first, lays, recs, desc, *ranks in batch:                  # (ranks: the producer's, else the env computes them)
            env._update_layout_arrays(first, lays, recs, desc, *ranks)
        return True

    def stop(self):
        self.stop_event.set()
        try:
            while True:                                   # (a producer blocked on a full queue sees the stop flag within 0.1 s)
                self.queue.get_nowait()
        except _queue.Empty:
            pass
        self.drain.join(timeout=5)
        self.process.join(timeout=10)
        if self.process.is_alive():
            self.process.terminate()

    def ready(self):
        return self.ready_queue.qsize()
