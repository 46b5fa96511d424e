"""CPU: the definition of the action effects (cooking_zoo_amd/effects.py) - the host model over the oracle against the bytes the
unmodified reference gave (tests/golden/effects_ref.json.gz), on hand-built records, `mask_of`, and the C header / binding."""
import re

import numpy as np
import pytest

import effects_common as ec
from cooking_zoo_amd import _native, effects, nav, soa
from golden_io import GoldenSet
from host_common import HEADER
from oracle_binding import Oracle

M, T, H, O, C = effects.MOVED, effects.TURNED, effects.HAND, effects.OBJECTS, effects.CELLS
CODE_OF = {(dx, dy): c for c, dx, dy in nav.DELTAS}                    # walk code of a direction


def oracle_of(gs, ep):
    off, cells = ep.static_table()
    return Oracle(ep.dims, gs.meta, gs.recipe_table, [(ep.states[0], off, cells)], scheme=gs.scheme, max_steps=1 << 30,
                  num_recipes=len(gs.cfg["recipes"]))


class World:
    """a golden set's first world with its oracle: records to edit by hand and the model's answer for them"""

    def __init__(self, name, state=0):
        self.gs = GoldenSet(name)
        self.ep = self.gs.episodes[0]
        self.dims, self.n_act = self.ep.dims, effects.num_actions(self.gs.scheme)
        self.step = ec.world_step_of(oracle_of(self.gs, self.ep))
        self.base = np.array(self.ep.states[state], dtype=np.uint32)

    def effects(self, rec):
        return effects.host_effects(self.step, rec[None], self.dims, self.n_act)[0]

    def cell(self, rec, x, y):
        return int(soa.record_cells(self.dims, rec)[y * self.dims.W + x])

    def objects_at(self, rec, x, y):
        d0 = rec[self.dims.dyn0_word0:self.dims.dyn0_word0 + self.dims.D]
        return [s for s in range(self.dims.D) if (int(d0[s]) >> 24) & soa.DYN_ALIVE and (int(d0[s]) & 0xFFFF) == (x | y << 8)]

    def wall_spot(self, rec, taken=()):
        """(x, y, code): a Floor cell next to an empty Counter in direction `code`, not one of `taken`"""
        for y in range(self.dims.H):
            for x in range(self.dims.W):
                for c, dx, dy in nav.DELTAS:
                    if ((x, y) not in taken and self.cell(rec, x, y) & soa.CELL_TYPE_MASK == soa.FLOOR and 0 <= x + dx < self.dims.W
                            and 0 <= y + dy < self.dims.H and self.cell(rec, x + dx, y + dy) & soa.CELL_TYPE_MASK == soa.COUNTER
                            and not self.objects_at(rec, x + dx, y + dy)):
                        return x, y, c
        raise AssertionError("no Floor cell next to an empty Counter")

    def place(self, rec, a, x, y, o, held=-1):
        rec[soa.AGENT_WORD0 + a] = soa.pack_agent(x, y, o, held)


def test_model_reproduces_every_byte_of_the_reference():
    doc = ec.golden()
    census, n = ec.Census(), 0
    for ep in doc["episodes"]:
        dims, recs = soa.Dims(*ep["dims"]), ec.golden_records(ep)
        want, raises = ec.golden_effects(ep)
        got = effects.host_effects(ec.world_step_of(ec.golden_oracle(ep)), recs, dims, want.shape[2])
        assert (want[raises] == 0).all(), f"{ep['set']}: an entry marked `raises` is not stored as 0"
        assert (got[raises] == 0).all(), f"{ep['set']}: where the reference raises the model's effect is not 0"
        bad = np.argwhere((got != want) & ~raises)
        assert not len(bad), (f"{ep['set']}: the model differs from the reference at (state, agent, code) {bad[:6].tolist()}: "
                              f"got {effects.names(got[tuple(bad[0])])}, stored {effects.names(want[tuple(bad[0])])}")
        assert (want[:, :, 0] == 0).all()
        census.add(ep["scheme"], want)
        n += len(recs)
    assert 24 <= n <= 64, f"the file holds {n} states, not a few dozen"
    assert {ep["level"] for ep in doc["episodes"]} >= {"coop_test", "switch_test", "crowded_6x5", "dense_8x8"}
    assert {(ep["level"], ep["scheme"]) for ep in doc["episodes"]} >= {("switch_test", 1), ("switch_test", 3), ("crowded_6x5", 1), ("crowded_6x5", 3)}
    census.check("effects_ref.json.gz", (1, 3))                      # the tool's own condition, from the file itself


def test_walking_into_walls_and_onto_floor():
    w = World("cfg2_coop_2agents")
    up, down, left = CODE_OF[(0, -1)], CODE_OF[(0, 1)], CODE_OF[(-1, 0)]
    rec = w.base.copy()
    assert w.cell(rec, 1, 0) & soa.CELL_TYPE_MASK == soa.COUNTER and not w.objects_at(rec, 1, 0), "the wall is not an empty Counter"
    assert w.cell(rec, 1, 2) & soa.CELL_TYPE_MASK == soa.FLOOR
    w.place(rec, 1, 5, 5, 1)                                         # (the other agent: out of the way)
    w.place(rec, 0, 1, 1, up)
    assert w.effects(rec)[0, up] == 0, "walking into a wall the agent already faces does something"
    w.place(rec, 0, 1, 1, left)
    assert w.effects(rec)[0, up] == T, "the same wall faced from another orientation is not TURNED alone"
    w.place(rec, 0, 1, 1, down)
    assert w.effects(rec)[0, down] == M, "a free floor cell ahead is not MOVED alone"
    # ... carrying an object: the Tomato goes into agent 0's hands
    d0 = w.dims.dyn0_word0
    slot = next(s for s in range(w.dims.D) if (int(rec[d0 + s]) >> 16) & 0xFF == soa.TOMATO and (int(rec[d0 + s]) >> 24) & soa.DYN_ALIVE)
    rec[d0 + slot] = soa.pack_dyn0(1, 1, soa.TOMATO, soa.DYN_ALIVE | soa.DYN_FREE)
    rec[w.dims.dyn1_word0 + slot] = 0
    w.place(rec, 0, 1, 1, down, held=slot)
    eff = w.effects(rec)
    assert eff[0, down] == M | O, f"walking with an object in hand gives {effects.names(eff[0, down])}"
    assert eff[0, up] == T | H | O, "bumping the empty Counter with an object in hand (scheme3) does not turn and put it down"
    assert (eff[:, 0] == 0).all()


def test_execute_on_a_ready_cutboard_with_empty_content_is_a_noop():
    """where the reference raises TypeError (cooking_world.py:162) the build has a no-op: effect 0"""
    gs = GoldenSet("refcrash_cutboard_scheme1")
    crash = gs.cfg["episodes"][0]["refcrash"]
    assert "Cutboard status=READY content=[]" in crash["detail"]
    w = World("refcrash_cutboard_scheme1", state=crash["step"])
    a = crash["action"].index(7)
    ax, ay, o, _h = soa.unpack_agent(w.base[soa.AGENT_WORD0 + a])
    dx, dy = next((dx, dy) for c, dx, dy in nav.DELTAS if c == o)
    front = w.cell(w.base, ax + dx, ay + dy)
    assert front & soa.CELL_TYPE_MASK == soa.CUTBOARD and front & soa.CELL_READY and not w.objects_at(w.base, ax + dx, ay + dy)
    eff = w.effects(w.base)
    assert eff[a, 7] == 0, f"EXECUTE on the READY Cutboard with empty content gives {effects.names(eff[a, 7])}"


def test_scheme1_interaction_aimed_off_grid_is_a_noop():
    """where the reference raises IndexError the build has a no-op: effect 0 for codes 5, 6 and 7"""
    w = World("scheme1_switch_2agents")
    rec = w.base.copy()
    cells = soa.record_cells(w.dims, rec)
    assert w.cell(rec, 1, 3) & soa.CELL_TYPE_MASK == soa.FLOOR
    cells[3 * w.dims.W + 0] = soa.FLOOR                              # a Floor cell on the rim: (0, 3), entered from (1, 3)
    for s in w.objects_at(rec, 0, 3):
        rec[w.dims.dyn0_word0 + s] = 0
    w.place(rec, 0, 0, 3, CODE_OF[(-1, 0)])
    eff = w.effects(rec)
    assert (eff[0, 5:8] == 0).all(), f"interactions aimed off-grid give {[effects.names(b) for b in eff[0, 5:8]]}"
    assert eff[0, CODE_OF[(-1, 0)]] == 0, "walking off the grid does something"
    assert eff[0, CODE_OF[(1, 0)]] == M | T


def test_a_running_blender_is_part_of_s0():
    """S0, not S: what progresses by itself is in both sides of the comparison"""
    w = World("cfg2_coop_2agents")
    rec = w.base.copy()
    cells = soa.record_cells(w.dims, rec)
    bx, by = next((c % w.dims.W, c // w.dims.W) for c in range(w.dims.C) if cells[c] & soa.CELL_TYPE_MASK == soa.BLENDER)
    d0 = w.dims.dyn0_word0
    slot = next(s for s in range(w.dims.D) if (int(rec[d0 + s]) >> 16) & 0xFF == soa.BANANA and (int(rec[d0 + s]) >> 24) & soa.DYN_ALIVE)
    assert not w.objects_at(rec, bx, by)
    rec[d0 + slot] = soa.pack_dyn0(bx, by, soa.BANANA, soa.DYN_ALIVE | soa.DYN_FREE)
    cells[by * w.dims.W + bx] |= soa.CELL_TOGGLE
    x0, y0, c0 = w.wall_spot(rec)
    x1, y1, c1 = w.wall_spot(rec, taken=[(x0, y0)])
    w.place(rec, 0, x0, y0, c0)
    w.place(rec, 1, x1, y1, c1)
    s0 = w.step(rec[None], np.zeros((1, 2), np.int32))[0]
    assert effects.diff(w.dims, rec[None], s0[None], 0)[0] == O | C, "the Blender does not run by itself in this record"
    eff = w.effects(rec)
    assert (eff[:, 0] == 0).all() and eff[0, c0] == 0 and eff[1, c1] == 0, "the running Blender shows in the effects of actions that do nothing"
    assert not ((eff[:, 1:] & (O | C)) == (O | C)).all(), "every action shows the Blender's own progress: the comparison is with S, not S0"


def test_done_and_gone_give_noop_only_rows():
    w = World("cfg2_coop_2agents")
    live = w.effects(w.base)
    assert live[0].any() and live[1].any()
    done = w.base.copy()
    done[soa.W_STATUS] |= soa.STATUS_DONE
    gone = w.base.copy()
    gone[soa.W_STATUS] |= 1 << (effects.SPAWN_GONE0 + 1)
    eff = effects.host_effects(w.step, np.stack([done, gone, w.base]), w.dims, w.n_act)
    assert not eff[0].any(), "a finished env has effects"
    assert not eff[1, 1].any() and eff[1, 0].any(), "a despawned agent has effects, or its present neighbour has none"
    assert np.array_equal(eff[2], live)
    mask = effects.mask_of(eff)
    assert mask[0].tolist() == [[1, 0, 0, 0, 0]] * 2 and mask[1, 1].tolist() == [1, 0, 0, 0, 0]


@pytest.mark.parametrize("ignore", ec.IGNORES)
def test_mask_of(ignore):
    eff = np.arange(32, dtype=np.uint8).reshape(2, 2, 8)
    eff[..., 0] = [[0, 7], [0, 31]]                                   # (code 0 is 1 whatever its byte)
    mask = effects.mask_of(eff, ignore)
    assert mask.dtype == np.uint8 and mask.shape == eff.shape
    for idx in np.ndindex(eff.shape):
        want = 1 if idx[-1] == 0 or int(eff[idx]) & ~ignore & 31 else 0
        assert mask[idx] == want, (idx, int(eff[idx]), ignore)
    if ignore == effects.ALL:
        assert mask[..., 1:].sum() == 0
    with pytest.raises(ValueError):
        effects.mask_of(eff, 32)


def test_num_actions_and_bit_names():
    assert effects.num_actions(3) == 5 and effects.num_actions(1) == 8
    with pytest.raises(ValueError):
        effects.num_actions(2)
    assert (M, T, H, O, C) == (1, 2, 4, 8, 16) and effects.ALL == 31
    assert effects.names(M | O) == "MOVED|OBJECTS" and effects.names(0) == "0"


def test_header_binding_and_abi_number():
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+CZ_ABI_VERSION\s+10\b", hdr), "the ABI number moved: the two entry points are additions"
    assert _native.header_abi_version() == 10
    flat = re.sub(r"\s+", " ", hdr)
    assert "int32_t cz_num_actions(cz_handle h);" in flat
    assert ("int cz_action_effects_device(cz_handle h, int64_t env_begin, int64_t env_count, uint32_t agents, uint32_t ignore, "
            "uint8_t *d_mask, uint8_t *d_effects);") in flat
    for name, value in (("MOVED", M), ("TURNED", T), ("HAND", H), ("OBJECTS", O), ("CELLS", C)):
        assert re.search(rf"#define\s+CZ_EFFECT_{name}\s+{value}\b", hdr), f"CZ_EFFECT_{name}"
    for cite in ("cooking_world.py:104-108", "action_scheme3.py:4-43", "action_scheme1.py:4-40", "cooking_zoo_amd/effects.py"):
        assert cite in hdr, f"the header does not cite {cite}"
    import ctypes as Ct
    sigs = {n: (r, a) for n, r, a in _native.SYMBOLS}
    VP, I64, U32 = Ct.c_void_p, Ct.c_int64, Ct.c_uint32
    assert sigs["cz_num_actions"] == (Ct.c_int32, [VP])
    assert sigs["cz_action_effects_device"] == (Ct.c_int, [VP, I64, I64, U32, U32, VP, VP])
    assert {"cz_num_actions", "cz_action_effects_device"} <= _native.ADDED_SYMBOLS
    lib = _native.lib()
    assert lib.cz_num_actions(None) == -1                              # (no device needed: a null handle has no scheme)
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for cls in (CookingVecEnv, ShardedVecEnv):
        for name in ("action_effects_device", "action_mask", "num_actions"):
            assert hasattr(cls, name), f"{cls.__name__}.{name}"
    assert "masked_fill" in CookingVecEnv.action_effects_device.__doc__
