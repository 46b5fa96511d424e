"""Host logic of CookingVecEnv.rotate_layouts (cooking_zoo_amd/rotation.py) that needs no GPU: the switch / refill schedule
step by step and across larger jumps, a refill that is not ready holds the switch back, a producer process that died is
reported instead of waited for, the producer refills the part that was in use when the rotation began, a group switched
behind the rotation's back is an error (not an assert that -O removes), and the module loads no device library."""
import os
import queue
import subprocess
import sys

import pytest

from cooking_zoo_amd import rotation


class _Env:
    """What a rotation may call of a CookingVecEnv, and no more; records the `rotation_events` the real one would."""

    def __init__(self, max_steps, pool_slices, groups=1, active=0):
        self._steps, self.max_steps, self.pool_slices = 0, max_steps, list(pool_slices)
        self._lay_groups, self._lay_active = groups, active
        self._rot, self.events, self.stopped = None, [], 0

    def rotate(self, source, every, groups, start=0):
        """the tail of CookingVecEnv.rotate_layouts"""
        self._rot = rotation.Rotation(source, every, groups, start, self._steps)
        self.set_layout_group(groups, start)
        return self._rot

    def advance(self, k=1):
        """CookingVecEnv._advance"""
        self._steps += k
        if self._rot is not None:
            self._rot.advanced(self)

    def set_layout_group(self, groups, active):
        self._lay_groups, self._lay_active = groups, active
        self.events.append((self._steps, "group", groups, active))

    def generate_layouts(self, first, count, generation, seed=None, mirror=True):
        assert mirror is False
        self.events.append((self._steps, "generated", first, count, seed, generation))

    def _update_layout_arrays(self, first, layouts, recs, desc):
        self.events.append((self._steps, "layouts", first, layouts))

    def stop_rotation(self):
        self._rot, self.stopped = None, self.stopped + 1


class _Process:
    def __init__(self, alive, exitcode=None):
        self.alive, self.exitcode = alive, exitcode

    def is_alive(self):
        return self.alive


def _process_source(alive, blocking):
    """a ProcessRefill over a stand-in process and plain queues: nothing is started"""
    return rotation.ProcessRefill(_Process(alive, None if alive else -9), queue.Queue(), None, queue.Queue(), blocking)


def test_schedule_stepping_by_one():
    env = _Env(5, [(0, 6), (6, 12)])
    env.rotate(rotation.DeviceRefill(3, 9), every=10, groups=3, start=1)
    for _ in range(45):
        env.advance()
    assert env.events == [(0, "group", 3, 1),
                          (10, "group", 3, 2),
                          (17, "generated", 2, 2, 9, 1), (17, "generated", 10, 4, 9, 1),
                          (20, "group", 3, 0),
                          (27, "generated", 4, 2, 9, 2), (27, "generated", 14, 4, 9, 2),
                          (30, "group", 3, 1),
                          (37, "generated", 0, 2, 9, 3), (37, "generated", 6, 4, 9, 3),
                          (40, "group", 3, 2)]


def test_schedule_is_relative_to_call_boundaries():
    """at most one refill and one switch per call, the refill first"""
    env = _Env(5, [(0, 6)])
    env.rotate(rotation.DeviceRefill(2, 9), every=10, groups=2)
    for k in (25, 1, 10, 10, 3):
        env.advance(k)
    assert env.events == [(0, "group", 2, 0),
                          (25, "group", 2, 1),
                          (36, "generated", 0, 3, 9, 1), (36, "group", 2, 0),
                          (46, "generated", 3, 3, 9, 2), (46, "group", 2, 1)]


def test_device_source_starts_nothing():
    import threading
    before = threading.active_count()
    source = rotation.DeviceRefill(2, 0)
    source.start()
    assert threading.active_count() == before and source.ready() == 0
    source.stop()


def test_a_refill_that_is_not_ready_holds_the_switch_back():
    env = _Env(5, [(0, 6)])
    source = _process_source(alive=True, blocking=False)
    rot = env.rotate(source, every=10, groups=2)
    for _ in range(24):
        env.advance()
    assert env.events == [(0, "group", 2, 0), (10, "group", 2, 1)]      # refill due at 17, switch due at 20: both wait
    assert source.ready() == 0
    lays, recs, desc = [object()] * 3, object(), object()
    source.ready_queue.put([(0, lays, recs, desc)])
    assert source.ready() == 1
    env.advance()
    assert env.events[2:] == [(25, "layouts", 0, lays), (25, "group", 2, 0)]
    assert (rot.refill_due, rot.flip_due, rot.n_refills) == (32, 35, 1)
    assert not env.stopped


@pytest.mark.parametrize("blocking", [True, False])
def test_a_dead_producer_is_reported_not_waited_for(blocking):
    env = _Env(10, [(0, 8)], groups=2)
    rot = env.rotate(_process_source(alive=False, blocking=blocking), every=20, groups=2)
    rot.flip_due, rot.refill_due = 1000, 0
    calls = 0
    with pytest.raises(RuntimeError, match=r"producer process died \(exit code -9\).*part 0 of 2"):
        for _ in range(3):
            calls += 1
            env.advance()
    assert calls == (1 if blocking else 2)                   # (non-blocking: reported at the second call boundary)
    assert env.stopped == 1 and env._rot is None


def test_group_switched_behind_the_rotation_is_an_error():
    env = _Env(10, [(0, 8)], groups=2)
    env.rotate(_process_source(alive=False, blocking=True), every=20, groups=2)
    env._rot.flip_due = 0
    env.set_layout_group(2, 1)                               # somebody switched parts meanwhile
    with pytest.raises(RuntimeError, match="behind the rotation"):
        env.advance()
    assert env.stopped == 1 and env._rot is None


def test_producer_starts_with_the_part_in_use():
    """batch b of the producer refills part (start + b) % groups: with start = 1 the first batch is for part 1"""
    import threading
    from cooking_zoo_amd import soa
    from cooking_zoo_amd.cooking_world.engine import load_level as ll
    meta = ll.load_meta_file("example")
    lv = ll.load_level_file("coop_test")
    dims = soa.Dims(7, 7, 12, 2, 278)
    q, stop = queue.Queue(maxsize=1), threading.Event()
    th = threading.Thread(target=rotation.produce_layouts, args=(q, stop, [lv], meta, 2, dims.as_tuple(), [(0, 8)], 2, 5, 1), daemon=True)
    th.start()
    firsts = [q.get(timeout=30)[0][0] for _ in range(3)]
    stop.set()
    th.join(timeout=10)
    assert firsts == [4, 0, 4]                               # part 1 (slots 4..7), then part 0, then part 1 again


def test_process_source_runs_and_stops_over_a_stand_in_producer():
    """start / refill / stop over the real drain thread, with a thread in the producer process's place"""
    import threading

    class Producer(threading.Thread):
        exitcode = None

        def terminate(self):
            raise AssertionError("the producer did not see the stop flag")

    q, stop = queue.Queue(maxsize=1), threading.Event()

    def produce():
        b = 0
        while not stop.is_set():
            try:
                q.put([(b, [b], None, None)], timeout=0.05)
                b += 1
            except queue.Full:
                pass
    source = rotation.ProcessRefill(Producer(target=produce, daemon=True), q, stop, queue.Queue(maxsize=1), blocking=True)
    env = _Env(5, [(0, 6)])
    source.start()
    assert source.drain.name == "cz-layout-rotation-drain"
    assert source.refill(env, 0, 1) and source.refill(env, 1, 2)
    assert env.events == [(0, "layouts", 0, [0]), (0, "layouts", 1, [1])]          # in the order they were produced
    source.stop()
    assert not source.drain.is_alive() and not source.process.is_alive()


def test_importing_the_module_loads_no_device_library():
    """the producer process imports it in a fresh interpreter, which must stay off the GPU"""
    code = ("import sys; sys.path.insert(0, %r)\nimport cooking_zoo_amd.rotation\n"
            "n = sys.modules.get('cooking_zoo_amd._native')\n"
            "assert n is None or n._lib is None, 'the native library was loaded'\n"
            "assert 'cooking_zoo_amd.vec_env' not in sys.modules\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
