"""Helpers shared by the tests that drive a `CookingVecEnv` (gpu_common.py is the raw C-ABI `Handle` layer): bit views, env
construction, the diagnostics of a handle, sentinel-filled device buffers with their checkers, the oracle's restatement of a
device reset, and the stream capture of a caller.  One definition of each; a test module imports what it needs from here and
never from another test module.  (pytest rewrites asserts in test modules only: every assert here carries its own message.)"""
import contextlib
import ctypes as C
import os

import numpy as np

from cooking_zoo_amd import _native, soa

TWO = ["TomatoLettuceSalad", "CarrotBanana"]
DENSE_RECIPES = ["TomatoSalad", "no_recipe", "TomatoLettuceSalad", "CarrotBanana"]
CROWDED4 = ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"]
HUGE3 = ["TomatoLettuceSalad", "MashedCarrotBanana", "TomatoSalad"]
COOP = dict(level="coop_test", meta="example", agents=2, recipes=TWO, scheme="scheme3", max_steps=12, num_layouts=3)
SENTINEL = 0x7FC0BEEF               # float32 rows: a quiet NaN no table entry equals
SENT64 = 0x7FF8BEEF0BADF00D         # float64 rows: a quiet NaN no table entry equals
SENT8 = 199                         # no entry of the quotient table in use and not the padding value: no code equals it
GUARD = 1024                        # float32 words behind the last row
MIN_INEXACT = 0.05                  # `Sensitivity`: the share of expected elements that must be inexact in float32

# (scheme, level, agents, recipes, meta): every level family and kernel instance, both schemes, 1-4 agents - the observation tests
OBS_CASES = [
    ("scheme3", "coop_test", 2, ["TomatoLettuceSalad", "CarrotBanana"], "example"),
    ("scheme3", "coop_test", 2, ["TomatoLettuceSalad", "CarrotBanana"], "example_odd"),          # F = 283: not a multiple of 4
    ("scheme1", "switch_test", 2, ["MashedCarrotBanana", "TomatoSalad"], "example"),
    ("scheme3", "coexistence_test", 1, ["TomatoLettuceOnionSalad"], "example"),
    ("scheme3", "crowded_6x5", 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], "crowded_6x5"),
    ("scheme1", "crowded_6x5", 3, ["TomatoSalad", "TomatoLettuceSalad", "MashedCarrotBanana"], "crowded_6x5"),
    ("scheme3", "large_16x16", 4, ["TomatoLettuceSalad", "CarrotBanana", "AppleWatermelon", "CucumberOnion"], "large_16x16"),
    ("scheme1", "dense_16x16", 2, ["TomatoLettuceOnionSalad", "MashedCarrotBanana"], "dense_16x16"),
    ("scheme3", "edge_8x8", 3, ["TomatoSalad", "MashedCarrotBanana", "TomatoLettuceSalad"], "edge"),
    ("scheme3", "limit_32x8", 3, ["TomatoSalad", "MashedCarrotBanana", "TomatoLettuceSalad"], "limits"),
    ("scheme3", "limit_8x31", 2, ["TomatoSalad", "CarrotBanana"], "limits"),
    ("scheme3", "huge_20x20", 3, ["TomatoLettuceSalad", "MashedCarrotBanana", "TomatoSalad"], "huge_20x20"),
    ("scheme1", "huge_32x32", 4, ["TomatoLettuceSalad", "CarrotBanana", "AppleWatermelon", "CucumberOnion"], "huge_32x32"),
]
# (level, meta, agents, recipes, scheme, instance): every kernel instance and agent count - the reset and restore tests
INSTANCE_CASES = [
    ("crowded_6x5", "crowded_6x5", 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], "scheme1", 0),
    ("dense_8x8", "dense_8x8", 1, DENSE_RECIPES[:1], "scheme3", 0),
    ("dense_8x8", "dense_8x8", 2, DENSE_RECIPES[:2], "scheme3", 0),
    ("dense_8x8", "dense_8x8", 3, DENSE_RECIPES[:3], "scheme3", 0),
    ("dense_8x8", "dense_8x8", 4, DENSE_RECIPES[:4], "scheme3", 0),
    ("dense_16x16", "dense_16x16", 2, ["TomatoLettuceOnionSalad", "MashedCarrotBanana"], "scheme1", 1),
    ("huge_20x20", "huge_20x20", 3, ["TomatoLettuceSalad", "MashedCarrotBanana", "TomatoSalad"], "scheme1", 2),
]


def bits(a):
    """float64 values as uint64: what `bit for bit` compares"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def want32(obs64):
    """what the float32 rows must hold, as uint32"""
    return np.ascontiguousarray(obs64, dtype=np.float64).astype(np.float32).view(np.uint32)


def strip(recs):
    """records without the eight running-return words (device-side statistics only)"""
    r = recs.copy()
    r[:, soa.RET_WORD0:soa.RET_WORD0 + 8] = 0
    return r


def junk(shape, dtype):
    """0xFF in every byte: NaN for float64, 255 for flags"""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xFF, np.uint8).view(dtype).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------------
# envs, tables, oracle, policy
# ---------------------------------------------------------------------------------------------------------------------------

def make_env(n, level="coop_test", meta="example", agents=2, recipes=TWO, scheme="scheme3", max_steps=30, **kw):
    """a CookingVecEnv with 8 layouts and auto-reset unless `kw` says otherwise; a module with other defaults binds them once"""
    from cooking_zoo_amd.vec_env import CookingVecEnv
    args = dict(action_scheme=scheme, num_layouts=8, auto_reset=True)
    args.update(kw)
    return CookingVecEnv(n, level, meta, agents, max_steps, recipes, **args)


def tables_of(n, level, meta, agents, recipes, scheme, max_steps, num_layouts, **kw):
    from cooking_zoo_amd.vec_env import BatchTables
    return BatchTables(n, level, meta, agents, max_steps, recipes, action_scheme=scheme, num_layouts=num_layouts, **kw)


def env_of(tables, auto_reset=True):
    """a CookingVecEnv over prepared tables"""
    from cooking_zoo_amd.vec_env import CookingVecEnv
    return CookingVecEnv(tables.num_envs, tables=tables, auto_reset=auto_reset)


def oracle_for(env, **kw):
    from oracle_binding import VecOracle
    return VecOracle.from_vec_env(env, **kw)


def policy(env, seed):
    from fuzz_policy import BumperActions
    return BumperActions(env.dims, env.scheme_class.CODE, np.random.default_rng(seed))


@contextlib.contextmanager
def lean(enabled):
    """CZ_LEAN is read by cz_create: the handles made inside take (or never take) a lean kernel"""
    old = os.environ.get("CZ_LEAN")
    os.environ["CZ_LEAN"] = "1" if enabled else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CZ_LEAN"]
        else:
            os.environ["CZ_LEAN"] = old


# ---------------------------------------------------------------------------------------------------------------------------
# what a handle says about itself
# ---------------------------------------------------------------------------------------------------------------------------

def _diag(env, name):
    f = getattr(_native.lib(), name)
    f.restype, f.argtypes = C.c_int32, [C.c_void_p]
    return int(f(env._h))


def instance(env):
    return _diag(env, "cz_diag_instance")


def last_lean(env):
    return _diag(env, "cz_diag_last_step_lean")


def last_mode(env):
    return _diag(env, "cz_diag_last_step_mode")


# ---------------------------------------------------------------------------------------------------------------------------
# one-step outputs
# ---------------------------------------------------------------------------------------------------------------------------

def widen(recs, dn, dd):
    """records of dims dn laid out for dims dd (more slots): shared words copied, every further slot and padding word zero"""
    out = np.zeros((recs.shape[0], dd.RW), dtype=np.uint32)
    out[:, :dn.dyn0_word0] = recs[:, :dn.dyn0_word0]
    out[:, dd.dyn0_word0:dd.dyn0_word0 + dn.D] = recs[:, dn.dyn0_word0:dn.dyn0_word0 + dn.D]
    out[:, dd.dyn1_word0:dd.dyn1_word0 + dn.D] = recs[:, dn.dyn1_word0:dn.dyn1_word0 + dn.D]
    return out


class Outs:
    """one-step device outputs (None for those in `skip`: the launch gets a null pointer); step() fills them with junk first"""

    def __init__(self, env, skip=()):
        n, A, F = env.num_envs, env.num_agents, env.F
        spec = dict(obs=((n, A, F), np.float64), rew=((n, A), np.float64), term=((n, A), np.uint8), trunc=((n, A), np.uint8))
        self.act = env.alloc((n, A), np.int32)
        self.buf = {k: None if k in skip else env.alloc(s, t) for k, (s, t) in spec.items()}
        self.junk = {k: junk(s, t) for k, (s, t) in spec.items()}

    def fill(self):
        for k, b in self.buf.items():
            if b is not None:
                b.from_host(self.junk[k])

    def get(self):
        return tuple(None if self.buf[k] is None else self.buf[k].to_host() for k in ("obs", "rew", "term", "trunc"))

    def step(self, env, acts):
        self.fill()
        self.act.from_host(acts)
        b = self.buf
        env.step_device(self.act, b["obs"], b["rew"], b["term"], b["trunc"])
        return self.get()


def check_step(ctx, got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        if k < 2:
            bad = np.argwhere(bits(g) != bits(w))
            assert not len(bad), f"{ctx}: {('observation', 'reward')[k]} differs at {bad[:6].tolist()}"
        else:
            assert np.array_equal(g, w), f"{ctx}: {('terminations', 'truncations')[k - 2]}"


PADDED = [(None, 0), (64, 0), (65, 1), (128, 1), (129, 2), (255, 2)]       # (max_dyn, instance); None: the level's own D = 12


def one_world_trajectory(scheme, n, T):
    """the coop_test world at its natural D = 12 under the state-aware policy, auto-resets included (max_steps 40): the dims, the
    reset observation and records, the actions [T][n][A], per step (observation, rewards, terminations, truncations, records),
    and the fewest episodes an env has finished"""
    base = make_env(n, scheme=scheme, max_steps=40)
    dn = base.dims
    assert dn.D == 12, f"coop_test has D = {dn.D}, not 12"
    orc = oracle_for(base)
    obs0 = orc.reset()
    rec0 = strip(orc.records)
    pol = policy(base, 31 if scheme == "scheme3" else 37)
    acts, want = [], []
    for t in range(T):
        acts.append(pol.act(orc.records))
        want.append(tuple(x.copy() for x in orc.step(acts[-1])) + (strip(orc.records),))
        pol.observe_result(orc.records)
    base.close()
    return dn, obs0, rec0, np.stack(acts), want, int(orc.records[:, soa.W_EPISODE].min())


def run_compact(env, acts, want, dn):
    """the trajectory through cz_step_device_compact on an env of `dn`'s world with at least as many slots"""
    n, A, F, Fp = env.num_envs, env.num_agents, env.F, env.codes_pitch
    table = env.obs_table()
    o = Outs(env, skip=("obs",))
    d_codes = env.alloc((n, A, Fp), np.uint8)
    for t, a in enumerate(acts):
        ctx = f"D={env.dims.D} cz_step_device_compact step {t}"
        o.fill()
        d_codes.from_host(np.full((n, A, Fp), 7, np.uint8))             # (a real code: 255 would read as 0.0, the padding value)
        o.act.from_host(a)
        b = o.buf
        env.step_device_compact(o.act, d_codes, b["rew"], b["term"], b["trunc"])
        codes = d_codes.to_host()
        assert (codes[:, :, F:] == 255).all(), f"{ctx}: padding bytes"
        check_step(ctx, (table[codes[:, :, :F]],) + o.get()[1:], want[t])
        assert np.array_equal(strip(env.get_state()), widen(want[t][4], dn, env.dims)), f"{ctx}: records"
    return env.stats()


def buffers(env):
    """whole-batch device buffers of a closed loop: actions, the step's four outputs and the codes"""
    n, A = env.num_envs, env.num_agents
    return dict(act=env.alloc((n, A), np.int32), obs=env.alloc((n, A, env.F), np.float64), rew=env.alloc((n, A), np.float64),
                term=env.alloc((n, A), np.uint8), trunc=env.alloc((n, A), np.uint8), codes=env.alloc((n, A, env.codes_pitch), np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------
# sentinel-filled observation buffers
# ---------------------------------------------------------------------------------------------------------------------------

class GuardedRows:
    """float32 rows [n][A][F] with GUARD sentinel words behind the last one"""

    def __init__(self, env, n=None):
        self.n = env.num_envs if n is None else n
        self.shape = (self.n, env.num_agents, env.F)
        self.words = int(np.prod(self.shape))
        self.buf = env.alloc((self.words + GUARD,), np.uint32)
        self.ptr = self.buf.ptr
        self.fill()

    def fill(self):
        self.buf.from_host(np.full(self.words + GUARD, SENTINEL, dtype=np.uint32))

    def rows(self):
        """the rows as uint32 [n][A][F]; asserts the guard is untouched"""
        got = self.buf.to_host()
        bad = np.nonzero(got[self.words:] != SENTINEL)[0]
        assert not len(bad), f"a store went past the last row: guard words {bad[:6].tolist()} were written"
        return got[:self.words].reshape(self.shape)


class Sensitivity:
    """share of the expected elements whose float64 value is not a float32: what makes the comparison sensitive to the rounding"""

    def __init__(self):
        self.inexact = self.total = 0

    def add(self, want64):
        w = np.asarray(want64, dtype=np.float64)
        self.inexact += int((w.astype(np.float32).astype(np.float64) != w).sum())
        self.total += w.size

    def check(self, ctx):
        share = self.inexact / max(self.total, 1)
        assert share >= MIN_INEXACT, f"{ctx}: only {self.inexact} of {self.total} expected elements are inexact in float32"


class Bufs:
    """whole-batch device buffers of one handle: the step's and the three observation forms, each with its sentinel"""

    def __init__(self, env):
        n, A, F = env.num_envs, env.num_agents, env.F
        self.env, self.shape = env, (n, A, F)
        self.act, self.rew = env.alloc((n, A), np.int32), env.alloc((n, A), np.float64)
        self.term, self.trunc = env.alloc((n, A), np.uint8), env.alloc((n, A), np.uint8)
        self.obs, self.codes, self.rows32 = env.alloc((n, A, F), np.uint64), env.alloc((n, A, env.codes_pitch), np.uint8), GuardedRows(env)
        self.mask, self.ids = env.alloc((n,), np.uint8), env.alloc((n,), np.int32)
        self.fill()

    def fill(self):
        self.obs.from_host(np.full(self.shape, SENT64, dtype=np.uint64))
        self.codes.from_host(np.full(self.codes.shape, SENT8, dtype=np.uint8))
        self.rows32.fill()

    def read(self):
        return self.obs.to_host(), self.codes.to_host(), self.rows32.rows()


ALL_FORMS = ("obs", "obs32", "codes")
FORM_SUBSETS = [tuple(f for k, f in enumerate(ALL_FORMS) if m >> k & 1) for m in range(1, 8)]      # the seven non-empty ones


def check_rows(ctx, env, before, got, rows, forms=ALL_FORMS):
    """the three buffers after a reset call: a buffer the call named holds what it held before with rows e of the restarted envs
    replaced by the oracle's reset observation, a buffer it did not name is untouched"""
    F, table = env.F, env.obs_table()
    obs, codes, r32 = (x.copy() for x in before)
    for e, o in rows.items():
        if "obs" in forms:
            obs[e] = o.view(np.uint64)
        if "obs32" in forms:
            r32[e] = want32(o)
    assert np.array_equal(got[0], obs), f"{ctx}: float64 rows"
    assert np.array_equal(got[2], r32), f"{ctx}: float32 rows"
    for e in range(codes.shape[0]):
        if e in rows and "codes" in forms:
            assert np.array_equal(table[got[1][e][:, :F]].view(np.uint64), rows[e].view(np.uint64)), f"{ctx}: codes of env {e}"
            assert (got[1][e][:, F:] == 255).all(), f"{ctx}: padding of env {e}"
        else:
            assert np.array_equal(got[1][e], codes[e]), f"{ctx}: codes of env {e} were touched"


def oracle_reset(orc, e, layout_id=-1, groups=1, active=0):
    """a device reset of env e on the oracle: bump the episode word, draw (or take) the layout, czo_reset_env -> the fresh
    world's float64 rows"""
    lib = orc.oracle.lib
    lib.czo_next_layout_group.restype = C.c_uint32
    rec = orc.records[e]
    rec[soa.W_EPISODE] += 1
    if layout_id < 0:
        layout_id = lib.czo_next_layout_group(C.c_int64(orc.env_id_base + e), C.c_uint32(int(rec[soa.W_EPISODE])), C.c_uint32(int(rec[soa.W_POOL])),
                                              C.c_uint32(orc.n_layouts), C.c_uint32(groups), C.c_uint32(active))
    obs = np.empty((orc.dims.A, orc.dims.F))
    err = lib.czo_reset_env(C.byref(orc.oracle.ctx), C.c_int64(e), C.c_uint32(int(layout_id)), rec.ctypes.data_as(C.c_void_p),
                            obs.ctypes.data_as(C.c_void_p))
    assert err == 0, f"czo_reset_env of env {e} onto layout {int(layout_id)} failed with {err}"
    return obs


# ---------------------------------------------------------------------------------------------------------------------------
# a stream capture of the caller
# ---------------------------------------------------------------------------------------------------------------------------

class Hip:
    """the few HIP calls a caller's graph needs, from the runtime the step library itself uses"""

    def __init__(self):
        rccl, hip = C.create_string_buffer(512), C.create_string_buffer(512)
        _native.lib().cz_runtime_paths(rccl, hip, 512)
        self.lib = C.CDLL(hip.value.decode())
        for name in ("hipStreamCreateWithFlags", "hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphInstantiate", "hipGraphLaunch",
                     "hipStreamSynchronize", "hipGraphExecDestroy", "hipGraphDestroy", "hipStreamDestroy", "hipEventCreate", "hipEventRecord",
                     "hipEventSynchronize", "hipEventElapsedTime", "hipEventDestroy"):
            getattr(self.lib, name).restype = C.c_int

    def ck(self, rc, what):
        assert rc == 0, f"{what} failed with HIP error {rc}"


class CallerStream:
    """A non-blocking stream of the caller, handed to the env with set_stream, and one graph captured on it:

        cs = CallerStream(env)
        with cs.capture():           # hipStreamBeginCapture ... hipStreamEndCapture + hipGraphInstantiate
            env.step_device(...)     # captured, not executed
        cs.replay(R); cs.sync()
        cs.close()                   # the graph, set_stream(None), the stream

    `hip`, `stream` and `gexec` are there for what a test does with them itself (timing a replay)."""

    def __init__(self, env):
        self.hip, self.env = Hip(), env
        self.stream, self.graph, self.gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.hip.ck(self.hip.lib.hipStreamCreateWithFlags(C.byref(self.stream), 1), "hipStreamCreateWithFlags")
        env.set_stream(self.stream)

    @contextlib.contextmanager
    def capture(self, mode=0):
        """mode: hipStreamCaptureModeGlobal / ThreadLocal / Relaxed"""
        hip = self.hip
        hip.ck(hip.lib.hipStreamBeginCapture(self.stream, mode), "hipStreamBeginCapture")
        yield self
        hip.ck(hip.lib.hipStreamEndCapture(self.stream, C.byref(self.graph)), "hipStreamEndCapture (a call inside the capture invalidated it)")
        hip.ck(hip.lib.hipGraphInstantiate(C.byref(self.gexec), self.graph, None, None, C.c_size_t(0)), "hipGraphInstantiate")

    def replay(self, R=1):
        for _ in range(R):
            self.hip.ck(self.hip.lib.hipGraphLaunch(self.gexec, self.stream), "hipGraphLaunch")

    def sync(self):
        self.hip.ck(self.hip.lib.hipStreamSynchronize(self.stream), "hipStreamSynchronize")

    def close(self):
        self.hip.lib.hipGraphExecDestroy(self.gexec)
        self.hip.lib.hipGraphDestroy(self.graph)
        self.env.set_stream(None)
        self.hip.lib.hipStreamDestroy(self.stream)
