"""CPU: ShardedVecEnv.load_sprites / render_device / render cut the frame buffers and the env range at the shards' env ranges -
on the host plan alone (dry_run), with stand-ins for the shards that record what they were handed."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cooking_zoo_amd import render
from cooking_zoo_amd.sharded import ShardedVecEnv

CFG2 = ("coop_test", "example", 2, 100, ["TomatoLettuceSalad", "CarrotBanana"])
W, H = 7, 7


class HostBuffer:
    def __init__(self, shape, dtype):
        self.array = np.zeros(shape, dtype)

    def to_host(self):
        return self.array.copy()

    def from_host(self, arr):
        self.array[...] = arr

    def free(self):
        pass


class FakeShard:
    """what ShardedVecEnv asks of a shard here; the `device` answer of env e is its GLOBAL id in every byte of its frames"""

    def __init__(self, first, count):
        self.first, self.num_envs = first, count
        self.calls = []

    def alloc(self, shape, dtype):
        return HostBuffer(shape, dtype)

    def frame_shape(self, P=16):
        return (H * P, W * P, 3)

    def load_sprites(self, sprites=None, M=None):
        self.calls.append(("sprites", sprites, M))

    def render_device(self, d_rgb8=None, d_chw32=None, P=16, vis=0, env_begin=0, env_count=None):
        self.calls.append((d_rgb8, d_chw32, P, vis))
        ids = self.first + np.arange(self.num_envs)
        if d_rgb8 is not None:
            assert d_rgb8.array.shape == (self.num_envs, H * P, W * P, 3), "the shard was handed a buffer of another shard's size"
            d_rgb8.array[...] = ids[:, None, None, None]
        if d_chw32 is not None:
            assert d_chw32.array.shape == (self.num_envs, 3, H * P, W * P)
            d_chw32.array[...] = ids[:, None, None, None] + 0.5

    def render(self, env_begin=0, env_count=1, P=16, vis=0):
        self.calls.append(("host", env_begin, env_count, P, vis))
        assert 0 <= env_begin and env_begin + env_count <= self.num_envs
        ids = (self.first + env_begin + np.arange(env_count)).astype(np.uint8)
        return np.broadcast_to(ids[:, None, None, None], (env_count, H * P, W * P, 3)).copy()


def sharded(num_envs, k):
    env = ShardedVecEnv(num_envs, *CFG2, action_scheme="scheme3", device_ids=[0] * k, dry_run=True)
    env.dry_run = False
    env.shards = [FakeShard(first, count) for first, count in env.ranges]
    env._pools = [ThreadPoolExecutor(max_workers=1) for _ in range(k)] if k > 1 else [None]
    return env


@pytest.mark.parametrize("num_envs,k", [(50, 3), (64, 4), (7, 1), (13, 2)])
def test_frames_are_cut_at_the_shards_env_ranges(num_envs, k):
    env = sharded(num_envs, k)
    counts = [c for _f, c in env.ranges]
    assert sum(counts) == num_envs and (num_envs % k == 0 or len(set(counts)) > 1), "the shards are not the unequal ones meant"
    P = 4
    assert env.frame_shape(P) == (H * P, W * P, 3)
    sheet = render.builtin_sprites(4)
    env.load_sprites(sheet)
    assert all(sh.calls == [("sprites", sheet, None)] for sh in env.shards)
    ids = np.arange(num_envs)
    d_rgb, d_chw = env.alloc((H * P, W * P, 3), np.uint8), env.alloc((3, H * P, W * P), np.float32)
    assert [p.array.shape for p in d_rgb.parts] == [(c, H * P, W * P, 3) for c in counts]
    env.render_device(d_rgb, d_chw, P=P, vis=0b10)
    rgb, chw = d_rgb.to_host(), d_chw.to_host()
    assert rgb.shape == (num_envs, H * P, W * P, 3) and chw.shape == (num_envs, 3, H * P, W * P)
    assert (rgb == ids[:, None, None, None]).all() and (chw == ids[:, None, None, None] + 0.5).all(), "frames are not in global env order"
    for i, sh in enumerate(env.shards):
        assert sh.calls[-1] == (d_rgb.parts[i], d_chw.parts[i], P, 0b10)
    env.render_device(d_chw32=d_chw, P=P)                                  # one output: the other stays None on every shard
    assert all(sh.calls[-1] == (None, d_chw.parts[i], P, 0) for i, sh in enumerate(env.shards))
    for lo, n in ((0, num_envs), (0, 1), (num_envs - 1, 1), (counts[0] - 1 if k > 1 else 2, 3), (3, 0)):
        f = env.render(lo, n, P=P, vis=1)
        assert f.dtype == np.uint8 and f.shape == (n, H * P, W * P, 3)
        assert (f == ids[lo:lo + n, None, None, None]).all(), "the host form is not in global env order"
        assert all(sh.calls[-1][0] == "host" and sh.calls[-1][3:] == (P, 1) for sh in env.shards)
    with pytest.raises(ValueError, match="range"):
        env.render(num_envs - 1, 2)
    for pool in env._pools:
        if pool is not None:
            pool.shutdown()


def test_a_plan_alone_refuses_device_work():
    env = ShardedVecEnv(50, *CFG2, action_scheme="scheme3", device_ids=[0, 0, 0], dry_run=True)
    assert [c for _f, c in env.ranges] == [17, 17, 16]
    with pytest.raises(RuntimeError, match="plan only"):
        env.render_device(None, None)
    with pytest.raises(RuntimeError, match="plan only"):
        env.render()
    with pytest.raises(RuntimeError, match="plan only"):
        env.load_sprites()
