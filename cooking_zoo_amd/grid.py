"""The grid observation: the reference's `(width, height, graph_representation_length)` state tensor, defined on records.

The reference declares `obs_spaces=["full"]` as a dict of a `(W, H, 32)` tensor, `agent_location` and `goal_vector`
(`cooking_env.py:118-123, 274-278`), allocates the tensor (`cooking_env.py:149-150`) and never writes it; every class of
`world_objects.py` carries the per-object vector it was meant to hold (`numeric_state_representation()`, `state_length()`).
This module is the definition of that tensor for the batched env, on the host, from records alone (it never loads the device
library); `k_observe_grid` (csrc/cz_query.h, `CookingVecEnv.observe_grid_device`) computes the same words on the device.

Reference channels (32): the classes in `GAME_CLASSES` order (alphabetical), `state_length()` consecutive channels each; the
content at `[x, y, off(cls) : off(cls) + len]` is `numeric_state_representation()` of an object of that class whose location is
`(x, y)`, the element-wise maximum where several share the cell (food inside a plate, a held object on its holder's cell).
Objects that are not alive contribute nothing, every agent of the record is drawn (a despawned one keeps its location, as in
the feature vector), and a cell's static object sets its class's channel.  All 32 are 0 or 1 (Bread's second and third are the
reference's literal zeros), so one cell is one 32-bit word.

Extended channels (16, opt-in, 32..47): what the reference vectors leave out - see EXT_CHANNELS.

Memory layout: cell (x, y) at index `x * H + y`, the reference's own (W, H, C) shape per env; `t.permute(0, 3, 1, 2)` of an
(N, W, H, C) torch tensor is a channels_last (N, C, W, H) view.  Three forms: `bits` uint32 [N][W][H][C / 32] (channel c is bit
c & 31 of word c >> 5), `grid8` uint8 [N][W][H][C], `grid32` float32 [N][W][H][C] (exactly 0.0 or 1.0).  A slot or an agent
whose coordinates lie outside the grid (no valid record has one) is not drawn.
"""
from __future__ import annotations

import numpy as np

from cooking_zoo_amd import soa
from cooking_zoo_amd.cooking_world.symbolic import STATE_LENGTH

# GAME_CLASSES order (inspect.getmembers: alphabetical) and each class's first channel
REF_CLASSES = sorted(STATE_LENGTH)
CLASS_OFFSET = {}
_off = 0
for _name in REF_CLASSES:
    CLASS_OFFSET[_name] = _off
    _off += STATE_LENGTH[_name]
N_REF = _off
assert N_REF == 32

_SUFFIX = {"Agent": ["", ".o1", ".o2", ".o3", ".o4"], "Bread": ["", ".zero1", ".zero2"]}
REF_CHANNELS = []
for _name in REF_CLASSES:
    REF_CHANNELS += [_name + s for s in _SUFFIX.get(_name, ["", ".chopped"][:STATE_LENGTH[_name]])]
EXT_CHANNELS = ["Carrot.mashed", "Banana.mashed", "food.fresh", "object.free", "object.held", "object.in_plate", "Cutboard.ready",
                "Blender.ready", "Blender.toggle", "Switch.active", "Block.walkable", "agent.despawned", "agent0", "agent1", "agent2",
                "agent3"]
N_EXT = len(EXT_CHANNELS)
(X_CARROT_MASHED, X_BANANA_MASHED, X_FRESH, X_FREE, X_HELD, X_IN_PLATE, X_CUT_READY, X_BL_READY, X_BL_TOGGLE, X_SW_ACTIVE,
 X_BLOCK_WALK, X_DESPAWNED, X_AGENT0) = range(13)                      # bit numbers inside the second word
SPAWN_GONE0 = 8                                                        # status word: bit 8 + a = agent a is despawned

STATIC_CHANNEL = [CLASS_OFFSET[n] for n in soa.STATIC_CLASSES]         # by cell type
DYN_CHANNEL = [CLASS_OFFSET[n] for n in soa.DYNAMIC_CLASSES]           # by dynamic class
DYN_HAS_CHOPPED = [n not in ("Plate", "Bread") for n in soa.DYNAMIC_CLASSES]


def channels(extended=False):
    """the channel names, 32 or 48"""
    return REF_CHANNELS + EXT_CHANNELS if extended else list(REF_CHANNELS)


def n_channels(extended=False):
    return N_REF + N_EXT if extended else N_REF


def host_bits(dims, records, extended=False):
    """records uint32 [n][RW] (or one record) -> the `bits` form uint32 [n][W][H][C / 32]"""
    recs = np.asarray(records, dtype=np.uint32)
    single = recs.ndim == 1
    recs = recs.reshape(-1, recs.shape[-1])
    W, H = dims.W, dims.H
    out = np.zeros((recs.shape[0], W, H, 2), dtype=np.uint32)
    for i, rec in enumerate(recs):
        g = out[i]
        cells = soa.record_cells(dims, rec)
        for c in range(dims.C):
            b, x, y = int(cells[c]), c % W, c // W
            ty = b & soa.CELL_TYPE_MASK
            if ty >= len(STATIC_CHANNEL):
                continue
            g[x, y, 0] |= 1 << STATIC_CHANNEL[ty]
            ext = 0
            if ty == soa.CUTBOARD and b & soa.CELL_READY:
                ext |= 1 << X_CUT_READY
            if ty == soa.BLENDER:
                ext |= (1 << X_BL_READY if b & soa.CELL_READY else 0) | (1 << X_BL_TOGGLE if b & soa.CELL_TOGGLE else 0)
            if ty == soa.SWITCH and b & soa.CELL_ACTIVE:
                ext |= 1 << X_SW_ACTIVE
            if ty == soa.BLOCK and b & soa.CELL_WALK:
                ext |= 1 << X_BLOCK_WALK
            g[x, y, 1] |= ext
        agents = [soa.unpack_agent(rec[soa.AGENT_WORD0 + a]) for a in range(dims.A)]
        held = {h for _x, _y, _o, h in agents if h >= 0}
        for s in range(dims.D):
            x, y, cls, flags = soa.unpack_dyn0(rec[dims.dyn0_word0 + s])
            if not flags & soa.DYN_ALIVE or cls >= len(DYN_CHANNEL) or x >= W or y >= H:
                continue
            ch = DYN_CHANNEL[cls]
            w0 = 1 << ch
            if DYN_HAS_CHOPPED[cls] and flags & soa.DYN_CHOPPED:
                w0 |= 1 << (ch + 1)
            ext = 0
            if flags & soa.DYN_MASHED and cls == soa.CARROT:
                ext |= 1 << X_CARROT_MASHED
            if flags & soa.DYN_MASHED and cls == soa.BANANA:
                ext |= 1 << X_BANANA_MASHED
            if cls != soa.PLATE and not flags & (soa.DYN_CHOPPED | soa.DYN_MASHED):
                ext |= 1 << X_FRESH
            if flags & soa.DYN_FREE:
                ext |= 1 << X_FREE
            if s in held:
                ext |= 1 << X_HELD
            if soa.unpack_dyn1(rec[dims.dyn1_word0 + s])[0] >= 0:
                ext |= 1 << X_IN_PLATE
            g[x, y, 0] |= w0
            g[x, y, 1] |= ext
        status = int(rec[soa.W_STATUS])
        for a, (x, y, orient, _h) in enumerate(agents):
            if x >= W or y >= H:
                continue
            g[x, y, 0] |= (1 << CLASS_OFFSET["Agent"]) | ((1 << (CLASS_OFFSET["Agent"] + orient)) if 1 <= orient <= 4 else 0)
            g[x, y, 1] |= (1 << (X_AGENT0 + a)) | ((1 << X_DESPAWNED) if status >> (SPAWN_GONE0 + a) & 1 else 0)
    out = np.ascontiguousarray(out if extended else out[..., :1])
    return out[0] if single else out


def expand(bits, dtype=np.uint8):
    """the `bits` form [..., C / 32] -> [..., C] of `dtype` (uint8: grid8, float32: grid32), values 0 and 1"""
    b = np.asarray(bits, dtype=np.uint32)
    planes = (b[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return np.ascontiguousarray(planes.reshape(b.shape[:-1] + (32 * b.shape[-1],))[..., :32 if b.shape[-1] == 1 else N_REF + N_EXT].astype(dtype))


def agent_xy(dims, records):
    """the `agent_location` entry: int32 [n][A][2]"""
    recs = np.asarray(records, dtype=np.uint32)
    recs = recs.reshape(-1, recs.shape[-1])
    w = recs[:, soa.AGENT_WORD0:soa.AGENT_WORD0 + dims.A]
    return np.stack([w & 0xFF, (w >> 8) & 0xFF], axis=-1).astype(np.int32)
