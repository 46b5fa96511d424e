"""GPU: the device-pointer step inside a stream capture of the CALLER (raw HIP through ctypes here, torch.cuda.graph in
test_gpu_zz_torch_interop.py): [policy kernel -> cz_step_device] captured once on the stream given to cz_set_stream, replayed many
times, must leave state and outputs bit for bit what the same launches leave when issued eagerly - also while a layout update is
staged (cz_update_layouts' copy is deferred, never issued from inside the capture).  Reference semantics of every captured step:
cooking_env.py:243-288."""
import ctypes as C
import functools

import numpy as np
import pytest

from cooking_zoo_amd import _native
from vec_common import CallerStream, bits, buffers, make_env

pytestmark = pytest.mark.gpu

make = functools.partial(make_env, max_steps=25)


def closed_loop_eager(env, b, steps, compact):
    L, h = _native.lib(), env._h
    for _ in range(steps):
        _native.check(h, L.cz_probe_policy(h, None if compact else b["obs"].ptr, b["codes"].ptr if compact else None, b["act"].ptr))
        if compact:
            env.step_device_compact(b["act"], b["codes"], b["rew"], b["term"], b["trunc"])
        else:
            env.step_device(b["act"], b["obs"], b["rew"], b["term"], b["trunc"])


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])                       # hipStreamCaptureModeGlobal / ThreadLocal / Relaxed
def test_step_captured_into_a_callers_graph_replays_bit_exact(compact, mode):
    n, K, R = 1024, 8, 200
    env, ref = make(n), make(n)
    be, br = buffers(env), buffers(ref)
    for e, b in ((env, be), (ref, br)):
        e.reset(return_obs=False)
        e.observe_device(b["obs"], b["codes"])                        # the first observation, on the device, in both forms
    cs = CallerStream(env)
    hip, stream, gexec = cs.hip, cs.stream, cs.gexec                   # (the timed replays at the end)
    # a staged layout update at capture time: the pool cut in two, the inactive half rewritten while a long rollout still runs -
    # cz_update_layouts cannot copy yet, and the captured steps must not try to (hipEventQuery / copies invalidate a capture)
    for e in (env, ref):
        e.set_layout_group(2, 0)
    env.rollout(1500, 7, 0); ref.rollout(1500, 7, 0)
    fresh = env.layouts[4:8][::-1]
    env.update_layouts(4, fresh); ref.update_layouts(4, fresh)
    with cs.capture(mode):
        closed_loop_eager(env, be, K, compact)                         # K x [policy, step]: captured, not executed
    t_before = env.get_state()[:, 0].copy()                            # (outside the capture: also flushes the staged update)
    cs.replay(R)
    cs.sync()
    ref.sync()
    assert np.array_equal(t_before, ref.get_state()[:, 0]), "capturing must not have stepped anything"
    closed_loop_eager(ref, br, K * R, compact)
    ref.sync()
    assert np.array_equal(env.get_state(), ref.get_state())
    for k in ("act", "rew", "term", "trunc") + (("codes",) if compact else ("obs",)):
        assert np.array_equal(be[k].to_host().view(np.uint8), br[k].to_host().view(np.uint8)), k
    assert env.stats() == ref.stats() and env.stats()["episodes"] > n
    # the replayed closed loop, timed: one graph launch = K x (policy + step)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip.lib.hipEventCreate(C.byref(ev0)); hip.lib.hipEventCreate(C.byref(ev1))
    hip.lib.hipEventRecord(ev0, stream)
    for _ in range(R):
        hip.lib.hipGraphLaunch(gexec, stream)
    hip.lib.hipEventRecord(ev1, stream)
    hip.ck(hip.lib.hipEventSynchronize(ev1), "hipEventSynchronize")
    ms = C.c_float()
    hip.lib.hipEventElapsedTime(C.byref(ms), ev0, ev1)
    print(f"\nreplayed closed loop in the caller's graph ({'codes' if compact else 'float64'}, {n} envs, capture mode {mode}): "
          f"{ms.value * 1e3 / (K * R):.2f} us per step")
    hip.lib.hipEventDestroy(ev0); hip.lib.hipEventDestroy(ev1)
    cs.close()
    env.close(); ref.close()


def test_ring_runs_and_rollouts_inside_a_capture():
    """cz_step_device_ring inside a caller's capture goes out as plain launches (no nested capture), cz_rollout_actions as its one
    fused launch; what must not be captured says so"""
    n, A, period = 512, 2, 8
    env, ref = make(n), make(n)
    be, br = buffers(env), buffers(ref)
    ring = np.random.default_rng(2).integers(0, 5, size=(period, n, A), dtype=np.int32)
    de, dr = env.alloc((period, n, A), np.int32), ref.alloc((period, n, A), np.int32)
    de.from_host(ring); dr.from_host(ring)
    env.reset(return_obs=False); ref.reset(return_obs=False)
    cs = CallerStream(env)
    _native.check(env._h, _native.lib().cz_update_layouts(env._h, 0, 0, None, None))   # (count 0: creates the copy stream, outside the capture)
    with cs.capture():
        env.step_device_ring(12, de, n * A, period, 3, be["obs"], be["rew"], be["term"], be["trunc"])
        env.rollout_actions(de, period, None, None, None, None)
        with pytest.raises(_native.NativeError, match="not inside a stream capture"):
            env.set_layout_group(2, 1)
        with pytest.raises(_native.NativeError, match="not inside a stream capture"):
            env.update_layouts(0, env.layouts[:2])
    for _ in range(5):
        cs.replay()
        ref.step_device_ring(12, dr, n * A, period, 3, br["obs"], br["rew"], br["term"], br["trunc"])
        ref.rollout_actions(dr, period, None, None, None, None)
    cs.sync()
    ref.sync()
    assert np.array_equal(env.get_state(), ref.get_state())
    assert np.array_equal(bits(be["obs"].to_host()), bits(br["obs"].to_host()))
    cs.close()
    env.close(); ref.close()


def test_rotating_pool_under_replays_of_a_callers_graph():
    """rotate_layouts + a captured step loop: capturing a launch is not a step - the env's step count (and with it the
    switch / refill schedule) does not move at capture time; the caller reports every replay with `advance(K)`, and the pool then
    rotates exactly as under eager launches of the same steps: same events at the same step numbers, same final records."""
    import warnings
    n, A, K, R = 256, 2, 10, 60
    env, ref = make(n, num_layouts=16, layout_seed=11), make(n, num_layouts=16, layout_seed=11)
    be, br = buffers(env), buffers(ref)
    ring = np.random.default_rng(5).integers(0, 5, size=(K, n, A), dtype=np.int32)
    de, dr = env.alloc((K, n, A), np.int32), ref.alloc((K, n, A), np.int32)
    de.from_host(ring); dr.from_host(ring)
    env.reset(return_obs=False); ref.reset(return_obs=False)
    cs = CallerStream(env)
    for e in (env, ref):
        e.rotate_layouts(50, groups=2, seed=3, prefetch=2)
    with cs.capture():
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            env.step_device_ring(K, de, n * A, K, 0, be["obs"], be["rew"], be["term"], be["trunc"])
            with pytest.raises(RuntimeError, match="inside a stream capture"):
                env.advance(K)
        assert any("advance(k)" in str(x.message) for x in w)
    assert env._steps == 0 and env.captured_steps == K and len(env.rotation_events) == 1      # (the initial cut of the pool into parts)
    for _ in range(R):
        cs.replay()
        env.advance(K)
        ref.step_device_ring(K, dr, n * A, K, 0, br["obs"], br["rew"], br["term"], br["trunc"])
    cs.sync()
    ref.sync()
    assert env._steps == ref._steps == K * R
    sig = lambda evs: [(e[0], e[1], e[2], e[3] if e[1] == "group" else [l.key() for l in e[3]]) for e in evs]
    assert sig(env.rotation_events) == sig(ref.rotation_events)
    assert sum(e[1] == "group" for e in env.rotation_events) >= 10 and sum(e[1] == "layouts" for e in env.rotation_events) >= 8
    assert np.array_equal(env.get_state(), ref.get_state())
    assert np.array_equal(bits(be["obs"].to_host()), bits(br["obs"].to_host()))
    env.stop_rotation(); ref.stop_rotation()
    cs.close()
    env.close(); ref.close()
