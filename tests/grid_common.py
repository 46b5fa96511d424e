"""Helpers of the grid observation tests (host and GPU): the levels, oracle trajectories under the state-aware policy with their
checkpoint records, channel coverage, and the second, independent route to the grid - the object view of
`symbolic.materialize` walked by the definition of cooking_zoo_amd/grid.py.  Nothing here touches the device library."""
import functools

import numpy as np

from cooking_zoo_amd import grid, soa
from cooking_zoo_amd.cooking_world import symbolic
from cooking_zoo_amd.cooking_world.constants import ActionObjectState, BlenderFoodStates, ChopFoodStates
from vec_common import DENSE_RECIPES, GUARD, SENTINEL, oracle_for, tables_of

FOUR = ["TomatoLettuceSalad", "CarrotBanana", "AppleWatermelon", "CucumberOnion"]
# name -> level, meta, agents, recipes, scheme, kernel instance, steps; every kernel instance, both non-square orientations, 1-4 agents
CASES = {
    "coop_test": ("coop_test", "example", 2, ["TomatoLettuceSalad", "CarrotBanana"], "scheme3", 0, 240),       # 49 cells: lanes without a cell
    "crowded_6x5": ("crowded_6x5", "crowded_6x5", 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], "scheme3", 0, 240),
    "dense_8x8": ("dense_8x8", "dense_8x8", 1, DENSE_RECIPES[:1], "scheme3", 0, 120),                          # a full wave of cells
    "switch_test": ("switch_test", "example", 2, ["MashedCarrotBanana", "TomatoSalad"], "scheme1", 0, 240),
    "limit_32x8": ("limit_32x8", "limits", 3, ["TomatoSalad", "MashedCarrotBanana", "TomatoLettuceSalad"], "scheme3", 1, 120),
    "limit_8x31": ("limit_8x31", "limits", 2, ["TomatoSalad", "CarrotBanana"], "scheme3", 1, 120),
    "dense_16x16": ("dense_16x16", "dense_16x16", 2, ["TomatoLettuceOnionSalad", "MashedCarrotBanana"], "scheme1", 1, 240),
    "large_16x16": ("large_16x16", "large_16x16", 4, FOUR, "scheme3", 1, 240),                                # every food class gets chopped here
    "huge_20x20": ("huge_20x20", "huge_20x20", 3, ["TomatoLettuceSalad", "MashedCarrotBanana", "TomatoSalad"], "scheme3", 2, 90),
    "huge_32x32": ("huge_32x32", "huge_32x32", 4, FOUR, "scheme1", 2, 90),
}
SPAWN = dict(agent_despawn_rate=0.1, agent_respawn_rate=0.3, grace_period=3, spawn_seed=4)


def case_tables(name, n, spawn=False, **kw):
    level, meta, agents, recipes, scheme, _inst, steps = CASES[name]
    args = dict(num_layouts=4, max_steps=steps + 1)
    args.update(SPAWN if spawn else {})
    args.update(kw)
    return tables_of(n, level, meta, agents, recipes, scheme, **args)


@functools.lru_cache(maxsize=None)
def checkpoints(name, n=6, spawn=False, points=4, seed=5):
    """the oracle's records uint32 [points][n][RW] at evenly spaced steps of one trajectory of the case under the state-aware
    policy (the last point is the last step), and the tables; computed once per argument set and shared - do not write to it"""
    from fuzz_policy import BumperActions
    tables = case_tables(name, n, spawn)
    orc = oracle_for(tables)
    orc.reset()
    pol = BumperActions(tables.dims, tables.scheme_class.CODE, np.random.default_rng(seed))
    steps = CASES[name][6]
    at = {steps * (k + 1) // points for k in range(points)}
    out = []
    for t in range(1, steps + 1):
        orc.step(pol.act(orc.records), want_obs=False)
        pol.observe_result(orc.records)
        if t in at:
            out.append(orc.records.copy())
    recs = np.stack(out)
    recs.setflags(write=False)
    return tables, recs


class Coverage:
    """which of the 48 channels have been seen set and seen clear"""

    def __init__(self):
        self.ones, self.zeros = np.zeros(2, np.uint32), np.zeros(2, np.uint32)

    def add(self, bits):
        b = np.asarray(bits, dtype=np.uint32).reshape(-1, 2)
        self.ones |= np.bitwise_or.reduce(b)
        self.zeros |= np.bitwise_or.reduce(~b)

    def never(self, which):
        """names of the channels never seen set (which = 1) or never seen clear (0)"""
        seen = self.ones if which else self.zeros
        return [n for c, n in enumerate(grid.channels(True)) if not (int(seen[c >> 5]) >> (c & 31)) & 1]


def view_bits(dims, layout, record):
    """the extended `bits` form uint32 [W][H][2] of one record by the second route: `symbolic.materialize`'s objects, each
    contributing the reference's numeric_state_representation of its class at its location, and for channels 32.. its attributes"""
    view = symbolic.materialize(dims, layout, record)
    g = np.zeros((dims.W, dims.H, 2), dtype=np.uint32)
    held = {id(a.holding) for a in view["Agent"] if a.holding is not None}
    in_plate = {id(c) for p in view.get("Plate", []) for c in p.content}

    def put(o, word, bit):
        g[o.location[0], o.location[1], word] |= np.uint32(1 << bit)

    for name, objs in view.items():
        for o in objs:
            if name == "Agent":
                vec = (1,) + tuple(int(o.orientation == k) for k in (1, 2, 3, 4))                   # world_objects.py:802-804
            elif name == "Bread":
                vec = (1, 0, 0)                                                                     # world_objects.py:747-748
            elif hasattr(o, "chop_state"):
                vec = (1, int(o.chop_state == ChopFoodStates.CHOPPED))                              # e.g. world_objects.py:444-445
            else:
                vec = (1,)
            assert len(vec) == symbolic.STATE_LENGTH[name], name
            for j, v in enumerate(vec):
                if v:
                    put(o, 0, grid.CLASS_OFFSET[name] + j)
            if name in soa.DYNAMIC_CLASSES:
                mashed = getattr(o, "blend_state", None) == BlenderFoodStates.MASHED
                if mashed and name in ("Carrot", "Banana"):
                    put(o, 1, grid.X_CARROT_MASHED if name == "Carrot" else grid.X_BANANA_MASHED)
                if name != "Plate" and not mashed and o.chop_state != ChopFoodStates.CHOPPED:
                    put(o, 1, grid.X_FRESH)
                for cond, bit in ((o.free, grid.X_FREE), (id(o) in held, grid.X_HELD), (id(o) in in_plate, grid.X_IN_PLATE)):
                    if cond:
                        put(o, 1, bit)
            ready = getattr(o, "status", None) == ActionObjectState.READY
            for cond, bit in ((name == "Cutboard" and ready, grid.X_CUT_READY), (name == "Blender" and ready, grid.X_BL_READY),
                              (name == "Blender" and getattr(o, "toggle", False), grid.X_BL_TOGGLE),
                              (name == "Switch" and getattr(o, "switch_active", False), grid.X_SW_ACTIVE),
                              (name == "Block" and o.walkable, grid.X_BLOCK_WALK)):
                if cond:
                    put(o, 1, bit)
    for a, ag in enumerate(view["Agent"]):
        put(ag, 1, grid.X_AGENT0 + a)
        if int(record[soa.W_STATUS]) >> (8 + a) & 1:
            put(ag, 1, grid.X_DESPAWNED)
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# sentinel-filled device buffers of the four outputs
# ---------------------------------------------------------------------------------------------------------------------------

FORMS = ("bits", "grid8", "grid32", "agent_xy")
FORM_SUBSETS = [tuple(f for k, f in enumerate(FORMS) if m >> k & 1) for m in range(1, 16)]         # the 15 non-empty ones
GUARD_WORDS = GUARD
# sentinels no form can produce: 0xDEADBEEF has bit 12 set (Bread's second channel, a literal zero of the reference) and bits behind
# channel 47; 0xAB is neither 0 / 1 nor a coordinate; the float32 one is vec_common.SENTINEL, a quiet NaN
SENT_BITS, SENT_BYTE, SENT_F32 = 0xDEADBEEF, 0xAB, SENTINEL


class GridBufs:
    """the four outputs laid out for n envs, each with GUARD_WORDS 32-bit words behind it, all filled with their sentinels"""

    def __init__(self, env, n, extended):
        W, H, A = env.dims.W, env.dims.H, env.num_agents
        C = 48 if extended else 32
        self.n, self.extended = n, extended
        self.shape = dict(bits=(n, W, H, (C + 31) // 32), grid8=(n, W, H, C), grid32=(n, W, H, C), agent_xy=(n, A, 2))
        self.dtype = dict(bits=np.uint32, grid8=np.uint8, grid32=np.uint32, agent_xy=np.uint32)
        self.sent = dict(bits=SENT_BITS, grid8=SENT_BYTE, grid32=SENT_F32, agent_xy=SENT_BYTE * 0x01010101)
        self.size = {f: int(np.prod(s)) for f, s in self.shape.items()}
        self.guard = {f: GUARD_WORDS * 4 // np.dtype(self.dtype[f]).itemsize for f in FORMS}
        self.buf = {f: env.alloc((self.size[f] + self.guard[f],), self.dtype[f]) for f in FORMS}
        self.fill()

    def fill(self):
        for f in FORMS:
            self.buf[f].from_host(np.full(self.size[f] + self.guard[f], self.sent[f], dtype=self.dtype[f]))

    def args(self, forms):
        """the keyword arguments of observe_grid_device that name `forms`"""
        return {("d_" + f): self.buf[f] for f in forms}

    def check(self, ctx, forms, dims, records):
        """a named buffer holds the host model of `records` in every element and its guard is untouched; a buffer the call did not
        name keeps its sentinel everywhere"""
        bits = grid.host_bits(dims, records, self.extended)
        want = dict(bits=bits, grid8=grid.expand(bits, np.uint8), grid32=grid.expand(bits, np.float32).view(np.uint32),
                    agent_xy=grid.agent_xy(dims, records).view(np.uint32))
        for f in FORMS:
            got = self.buf[f].to_host()
            body, guard = got[:self.size[f]].reshape(self.shape[f]), got[self.size[f]:]
            if f not in forms:
                assert (got == self.sent[f]).all(), f"{ctx}: {f} was not named and was written"
                continue
            assert (guard == self.sent[f]).all(), f"{ctx}: {f}: a store went behind the last cell (guard words {np.nonzero(guard != self.sent[f])[0][:6].tolist()})"
            bad = np.argwhere(body != want[f])
            assert not len(bad), (f"{ctx}: {f} differs from the host model at {bad[:6].tolist()}: got {body[tuple(bad[0])]:#x}, "
                                  f"want {want[f][tuple(bad[0])]:#x}")
