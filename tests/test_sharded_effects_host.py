"""CPU: ShardedVecEnv.action_effects_device / action_mask cut the [N, A, n_actions] buffers at the shards' env ranges - on the
host plan alone (dry_run), with stand-ins for the shards that record what they were handed."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cooking_zoo_amd import effects
from cooking_zoo_amd.sharded import ShardedVecEnv

CFG2 = ("coop_test", "example", 2, 100, ["TomatoLettuceSalad", "CarrotBanana"])


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
    """what ShardedVecEnv asks of a shard here; the `device` answer of env e is its GLOBAL id in every byte of its rows"""

    def __init__(self, first, count, A, n_act):
        self.first, self.num_envs, self.num_agents, self.num_actions = first, count, A, n_act
        self.calls = []

    def alloc(self, shape, dtype):
        return HostBuffer(shape, dtype)

    def _answer(self):
        ids = (self.first + np.arange(self.num_envs)).astype(np.uint8)
        return np.broadcast_to(ids[:, None, None], (self.num_envs, self.num_agents, self.num_actions))

    def action_effects_device(self, d_mask=None, d_effects=None, agents=None, ignore=0):
        self.calls.append((d_mask, d_effects, agents, ignore))
        for buf, add in ((d_mask, 0), (d_effects, 100)):
            if buf is not None:
                assert buf.array.shape == (self.num_envs, self.num_agents, self.num_actions), "the shard was handed a buffer of another shard's size"
                buf.array[...] = self._answer() + add

    def action_mask(self, agents=None, ignore=0):
        self.calls.append(("host", agents, ignore))
        return (self._answer() + 0).astype(np.uint8), (self._answer() + 100).astype(np.uint8)


def sharded(num_envs, k):
    env = ShardedVecEnv(num_envs, *CFG2, action_scheme="scheme3", device_ids=[0] * k, dry_run=True)
    env.dry_run = False
    env.shards = [FakeShard(first, count, env.num_agents, effects.num_actions(3)) for first, count in env.ranges]
    env._pools = [ThreadPoolExecutor(max_workers=1) for _ in range(k)] if k > 1 else [None]
    return env


@pytest.mark.parametrize("num_envs,k", [(50, 3), (64, 4), (7, 1), (13, 2)])
def test_buffers_are_cut_at_the_shards_env_ranges(num_envs, k):
    env = sharded(num_envs, k)
    counts = [c for _f, c in env.ranges]
    assert sum(counts) == num_envs and (num_envs % k == 0 or len(set(counts)) > 1), "the shards are not the unequal ones meant"
    assert env.num_actions == 5
    ids = np.arange(num_envs, dtype=np.uint8)
    d_m, d_e = env.alloc((2, 5), np.uint8), env.alloc((2, 5), np.uint8)
    assert [p.array.shape for p in d_m.parts] == [(c, 2, 5) for c in counts]
    env.action_effects_device(d_m, d_e, agents=0b10, ignore=effects.TURNED)
    m, e = d_m.to_host(), d_e.to_host()
    assert m.shape == e.shape == (num_envs, 2, 5)
    assert (m == ids[:, None, None]).all() and (e == ids[:, None, None] + 100).all(), "rows are not in global env order"
    for i, sh in enumerate(env.shards):
        assert sh.calls == [(d_m.parts[i], d_e.parts[i], 0b10, effects.TURNED)]
    env.action_effects_device(d_effects=d_e)                              # one output: the other stays None on every shard
    assert all(sh.calls[-1] == (None, d_e.parts[i], None, 0) for i, sh in enumerate(env.shards))
    m, e = env.action_mask(agents=1, ignore=effects.MOVED | effects.TURNED)
    assert m.dtype == np.uint8 and m.shape == e.shape == (num_envs, 2, 5)
    assert (m == ids[:, None, None]).all() and (e == ids[:, None, None] + 100).all(), "the host form is not concatenated in global env order"
    assert all(sh.calls[-1] == ("host", 1, effects.MOVED | effects.TURNED) for sh in env.shards)
    for pool in env._pools:
        if pool is not None:
            pool.shutdown()


def test_a_plan_alone_refuses_device_work():
    env = ShardedVecEnv(50, *CFG2, action_scheme="scheme3", device_ids=[0, 0, 0], dry_run=True)
    assert [c for _f, c in env.ranges] == [17, 17, 16]
    with pytest.raises(RuntimeError, match="plan only"):
        env.action_effects_device(None, None)
    with pytest.raises(RuntimeError, match="plan only"):
        env.action_mask()
