"""Shared by the episode-record tests (cz_episodes_collect): the numpy model that says what every collect must report, made from
the oracle's per-step rewards and records alone, and the guarded device buffers a collect writes into."""
import numpy as np

from cooking_zoo_amd import _native, soa

EP = np.dtype(_native.EPISODE_DTYPE)
GUARD = 16                              # elements behind every output array that no collect may touch
SENT_MASK, SENT64, SENT_LEN, SENT_FLAGS, SENT_BYTE, SENT_COUNT = 0xAA, 0x7FF8BEEF0BADF00D, -77, 0xDEADBEEF, 0xCD, -5


class EpisodeModel:
    """What the device keeps, from the oracle's run: for every env and agent the oracle's reward is added with np.float64 adds, in step
    order, on the steps that are neither a reset pass nor frozen (`ret += myrew` under `o.stepped`); at a step whose record gains the
    done bit the env's episode is emitted - returns, t, episode word, end flags, root marks - and the sum restarts from 0.0."""

    def __init__(self, n, agents, wide, env_id_base=0):
        self.n, self.A, self.wide, self.base = n, agents, wide, env_id_base
        self.ret = np.zeros((n, 4), dtype=np.float64)
        self.pending = {}               # env -> [entry, episodes finished since the last collect]
        self.emitted = []               # every entry ever emitted (the tests' vacuity conditions read it)

    def step(self, before, after, rew):
        stepped = (before[:, soa.W_STATUS] & soa.STATUS_DONE) == 0
        ended = stepped & ((after[:, soa.W_STATUS] & soa.STATUS_DONE) != 0)
        self.ret[stepped, :self.A] += rew[stepped]
        for e in np.nonzero(ended)[0]:
            st = int(after[e, soa.W_STATUS])
            marks = int(after[e, soa.W_MARKS]) | ((int(after[e, soa.W_MARKS_HI]) << 32) if self.wide else 0)
            roots = sum(((marks >> ((16 if self.wide else 8) * a)) & 1) << a for a in range(self.A))
            flags = (1 if st & soa.STATUS_TERM else 0) | (2 if st & soa.STATUS_TRUNC else 0) | (roots << 4)
            entry = np.zeros((), dtype=EP)
            entry["env"], entry["episode"], entry["length"], entry["flags"] = self.base + e, after[e, soa.W_EPISODE], after[e, soa.W_T], flags
            entry["ret"] = self.ret[e]
            self.pending[int(e)] = [entry, self.pending.get(int(e), [None, 0])[1] + 1]
            self.emitted.append(entry.copy())
            self.ret[e] = 0.0

    def abort(self, e):
        """the env was restarted in mid-episode (reset_device with a mask): no record, the next return starts from 0.0"""
        self.ret[e] = 0.0

    def clear(self):
        """reset_stats: what is pending is forgotten"""
        self.pending = {}

    def collect(self):
        """-> the entries a collect must report now, in env order; they count as seen afterwards"""
        out = np.zeros(len(self.pending), dtype=EP)
        for k, e in enumerate(sorted(self.pending)):
            out[k] = self.pending[e][0]
            out[k]["finished"] = self.pending[e][1]
        self.pending = {}
        return out


def same_entries(got, want):
    """bit for bit: the structured arrays as bytes (returns compare as their uint64 patterns)"""
    return got.shape == want.shape and got.tobytes() == want.tobytes()


class Collector:
    """Guarded device buffers for every output of collect_episodes, pre-filled with sentinels before every call; `collect` makes the
    call and checks everything it wrote - and everything it must not have written - against the model's entries."""

    def __init__(self, env, capacity=None):
        n, A = env.num_envs, env.num_agents
        self.env, self.n, self.A = env, n, A
        self.cap = n if capacity is None else capacity
        self.mask, self.ret = env.alloc((n + GUARD,), np.uint8), env.alloc((n * A + GUARD,), np.uint64)
        self.length, self.flags = env.alloc((n + GUARD,), np.int32), env.alloc((n + GUARD,), np.uint32)
        self.list, self.count = env.alloc(((self.cap + GUARD) * EP.itemsize,), np.uint8), env.alloc((1 + GUARD,), np.int32)

    def fill(self):
        self.mask.from_host(np.full(self.mask.shape, SENT_MASK, np.uint8)); self.ret.from_host(np.full(self.ret.shape, SENT64, np.uint64))
        self.length.from_host(np.full(self.length.shape, SENT_LEN, np.int32)); self.flags.from_host(np.full(self.flags.shape, SENT_FLAGS, np.uint32))
        self.list.from_host(np.full(self.list.shape, SENT_BYTE, np.uint8)); self.count.from_host(np.full(self.count.shape, SENT_COUNT, np.int32))

    def read(self):
        return dict(mask=self.mask.to_host(), ret=self.ret.to_host(), length=self.length.to_host(), flags=self.flags.to_host(),
                    list=self.list.to_host(), count=self.count.to_host())

    def collect(self, want, ctx, capacity=None, dense=True, packed=True, count=True):
        cap = self.cap if capacity is None else capacity
        assert cap <= self.cap
        self.fill()
        self.env.collect_episodes(self.mask if dense else None, self.ret if dense else None, self.length if dense else None,
                                  self.flags if dense else None, self.list if packed else None, cap, self.count if count else None)
        got = self.read()
        self.verify(got, want, ctx, cap, dense, packed, count)
        return got

    def verify(self, got, want, ctx, cap, dense=True, packed=True, count=True):
        n, A = self.n, self.A
        local = (want["env"] - self.env.env_id_base).astype(np.int64)
        mask, ret = np.full(n + GUARD, SENT_MASK, np.uint8), np.full(n * A + GUARD, SENT64, np.uint64)
        length, flags = np.full(n + GUARD, SENT_LEN, np.int32), np.full(n + GUARD, SENT_FLAGS, np.uint32)
        if dense:
            mask[:n] = 0
            mask[local] = 1
            length[local], flags[local] = want["length"].astype(np.int32), want["flags"]
            rows = ret[:n * A].reshape(n, A)
            rows[local] = want["ret"][:, :A].view(np.uint64)
        assert np.array_equal(got["mask"], mask), f"{ctx}: mask (want envs {local.tolist()}, got {np.nonzero(got['mask'][:n] == 1)[0].tolist()})"
        assert np.array_equal(got["ret"], ret), f"{ctx}: dense returns"
        assert np.array_equal(got["length"], length), f"{ctx}: dense lengths"
        assert np.array_equal(got["flags"], flags), f"{ctx}: dense flags"
        lst = np.full((self.cap + GUARD) * EP.itemsize, SENT_BYTE, np.uint8)
        if packed:
            k = min(len(want), cap)
            lst[:k * EP.itemsize] = np.frombuffer(want[:k].tobytes(), dtype=np.uint8)
        if not np.array_equal(got["list"], lst):
            k = min(len(want), cap)
            g = got["list"][:k * EP.itemsize].view(EP)
            bad = [i for i in range(k) if g[i].tobytes() != want[i].tobytes()]
            raise AssertionError(f"{ctx}: packed list, {len(bad)} of {k} entries differ" +
                                 (f", the first: got {g[bad[0]]}, want {want[bad[0]]}" if bad else " none; bytes behind them were touched"))
        cnt = np.full(1 + GUARD, SENT_COUNT, np.int32)
        if count:
            cnt[0] = len(want)
        assert np.array_equal(got["count"], cnt), f"{ctx}: count {got['count'][0]}, want {len(want)}"
