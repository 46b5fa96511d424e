"""Action effects and action masks: which of an agent's actions would do anything at all.

In CookingZoo most actions are no-ops most of the time; PettingZoo's remedy is an `action_mask` beside the observation.  The
reference offers none.  This module is the definition of the one `CookingVecEnv.action_effects_device` computes on the device
(`cz_action_effects_device`, `k_action_effects`), and its host model.

Definition.  For an env whose done bit is clear, an agent `a` that is present, and an action code `c` of the env's scheme:

- Codes are `0 .. n_actions - 1`.  `n_actions` is 5 for `scheme3` and 8 for `scheme1` (action_scheme3.py:4-43, action_scheme1.py:4-40).
- `S0` is the record after `world_step` with every present agent playing 0.
- `Sc` is the record after `world_step` with agent `a` playing `c` and every other present agent playing 0.
- `world_step` means `perform_agent_actions` + `progress_world` + the linked interactions + the free-flag normalisation
  (`cooking_world.py:104-108`).
- `world_step` here does **not** include `handle_agent_spawn` (cooking_world.py:109-112), `t`, recipe marks, rewards or flags.
- A despawned agent takes no part, as in the step kernels (action -1).
- `S0` is not `S`: a running Blender progresses by itself.

`effects[a][c]` is a byte of five bits.  Each bit is a difference between `Sc` and `S0`, in the words a step would write:

    bit 0  MOVED    agent a's (x, y) differs
    bit 1  TURNED   agent a's orientation differs
    bit 2  HAND     agent a's held-slot field differs (picked up, put down, swapped)
    bit 3  OBJECTS  any dyn0 / dyn1 word differs (an object moved, changed state, was created, deleted, plated, delivered)
    bit 4  CELLS    any cell byte differs (appliance READY / TOGGLE, Switch, Block)

Other agents' words cannot differ while they play 0, so there is no bit for them.

- `effects[a][0] = 0`.
- `mask[a][c] = 1` if `c == 0` or `(effects[a][c] & ~ignore) != 0`, else 0.
- `ignore` is a caller's bit set.  For example, `TURNED` makes "only turns on the spot" count as a no-op, which `scheme3` users
  will want.

Special cases: a despawned agent gets `mask = [1, 0, ...]` and effects 0.  A finished env (done bit set) gets the same for every
agent: the next step resets or freezes it whatever is played.  Where the reference raises and the build has a defined no-op, the
effect is 0 like any no-op: `EXECUTE` on a READY Cutboard with empty content, and a `scheme1` interaction aimed off-grid (DESIGN.md
section 2).

The one caveat: the mask speaks about one agent acting alone.  With several agents acting at once, the collision filter and the
serial interaction order can change what happens; that is what every per-agent action mask means.
"""
import numpy as np

from cooking_zoo_amd import soa

MOVED, TURNED, HAND, OBJECTS, CELLS = 1, 2, 4, 8, 16
ALL = MOVED | TURNED | HAND | OBJECTS | CELLS
BIT_NAMES = {MOVED: "MOVED", TURNED: "TURNED", HAND: "HAND", OBJECTS: "OBJECTS", CELLS: "CELLS"}
SPAWN_GONE0 = 8                                                        # status word: bit 8 + a = agent a is despawned


def num_actions(scheme_code):
    """codes per agent of an action scheme (its number: 3 or 1)"""
    if int(scheme_code) == 3:
        return 5
    if int(scheme_code) == 1:
        return 8
    raise ValueError(f"action scheme {scheme_code}: only scheme1 and scheme3 exist here")


def names(byte):
    """'MOVED|OBJECTS' for an effect byte ('0' for none)"""
    return "|".join(n for b, n in BIT_NAMES.items() if int(byte) & b) or "0"


def mask_of(effects, ignore=0):
    """uint8 mask of an effects array [..., n_actions]: 1 for code 0 and for every code with an effect outside `ignore`"""
    if int(ignore) & ~ALL:
        raise ValueError(f"ignore has bits outside the five effects: {int(ignore):#x}")
    eff = np.asarray(effects, dtype=np.uint8)
    mask = ((eff & np.uint8(ALL & ~int(ignore))) != 0).astype(np.uint8)
    mask[..., 0] = 1
    return mask


def diff(dims, s0, sc, a):
    """the effect bytes uint8 [n] of agent `a` between records s0 and sc (uint32 [n, RW] each)"""
    x = s0[:, soa.AGENT_WORD0 + a] ^ sc[:, soa.AGENT_WORD0 + a]
    dyn = slice(dims.dyn0_word0, dims.dyn1_word0 + dims.D)
    cells = slice(dims.cells_word0, dims.cells_word0 + dims.CW)

    def cell_bytes(r):
        return np.ascontiguousarray(r[:, cells]).view(np.uint8)[:, :dims.C]

    out = np.where(x & 0xFFFF, MOVED, 0) | np.where(x & 0xFF0000, TURNED, 0) | np.where(x >> 24, HAND, 0)
    out = out | np.where((s0[:, dyn] != sc[:, dyn]).any(axis=1), OBJECTS, 0)
    out = out | np.where((cell_bytes(s0) != cell_bytes(sc)).any(axis=1), CELLS, 0)
    return out.astype(np.uint8)


def host_effects(world_step, records, dims, n_actions):
    """The definition written out: effects uint8 [n, A, n_actions] of `records` (uint32 [n, RW]).

    `world_step(records, actions)` takes records uint32 [m, RW] and actions int32 [m, A] (-1: the agent is not in the list
    world_step acts on) and returns the records after one world_step; header words are not looked at.  It is asked S0 once and once
    per (agent, code); finished envs are never handed to it."""
    recs = np.ascontiguousarray(records, dtype=np.uint32)
    n, A = recs.shape[0], dims.A
    effects = np.zeros((n, A, n_actions), dtype=np.uint8)
    live = np.nonzero((recs[:, soa.W_STATUS] & soa.STATUS_DONE) == 0)[0]
    if not len(live):
        return effects
    base = recs[live]
    gone = ((base[:, soa.W_STATUS, None] >> (SPAWN_GONE0 + np.arange(A))) & 1) != 0
    idle = np.where(gone, -1, 0).astype(np.int32)
    s0 = np.asarray(world_step(base.copy(), idle.copy()), dtype=np.uint32)
    for a in range(A):
        for c in range(1, n_actions):
            acts = idle.copy()
            acts[~gone[:, a], a] = c
            sc = np.asarray(world_step(base.copy(), acts), dtype=np.uint32)
            e = diff(dims, s0, sc, a)
            e[gone[:, a]] = 0
            effects[live, a, c] = e
    return effects
