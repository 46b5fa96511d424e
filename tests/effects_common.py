"""Helpers of the action-effect tests (host and GPU): the fixture computed from the unmodified reference, the oracle's step as the
`world_step` callable of `effects.host_effects`, the census of codes and bits, and sentinel-filled device buffers of the two outputs.
Nothing here touches the device library."""
import functools
import gzip
import json
import os

import numpy as np

from cooking_zoo_amd import effects, soa
from vec_common import GUARD

HERE = os.path.dirname(os.path.abspath(__file__))
IGNORES = (0, effects.TURNED, effects.MOVED | effects.TURNED, effects.ALL)
BITS = (effects.MOVED, effects.TURNED, effects.HAND, effects.OBJECTS, effects.CELLS)


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/effects_ref.json.gz (tools/gen_effects_golden.py); do not write to it"""
    with gzip.open(os.path.join(HERE, "golden", "effects_ref.json.gz")) as f:
        return json.load(f)


def golden_records(ep):
    return np.array([s["record"] for s in ep["states"]], dtype=np.uint32)


def golden_effects(ep):
    """(effects uint8 [states, A, n_actions], raises bool of the same shape) as stored: digit strings, two digits per code"""
    A, n_act = ep["dims"][3], effects.num_actions(ep["scheme"])
    eff = np.zeros((len(ep["states"]), A, n_act), dtype=np.uint8)
    raises = np.zeros(eff.shape, dtype=bool)
    for i, s in enumerate(ep["states"]):
        for a, row in enumerate(s["effects"]):
            assert len(row) == 2 * n_act, f"a stored row has {len(row)} digits, not two per code"
            eff[i, a] = [int(row[2 * c:2 * c + 2]) for c in range(n_act)]
        for a, c, _kind in s.get("raises", []):
            raises[i, a, c] = True
    return eff, raises


def static_table_of(dims, record):
    """(offsets, cells) of an oracle layout from a record's cell types, cells in index order (observations are not compared here)"""
    cells = soa.record_cells(dims, np.asarray(record, dtype=np.uint32)) & soa.CELL_TYPE_MASK
    off, out = [0], []
    for t in range(len(soa.STATIC_CLASSES)):
        out += [int(c) for c in np.nonzero(cells == t)[0]]
        off.append(len(out))
    return np.asarray(off, dtype=np.int32), np.asarray(out, dtype=np.int16)


def golden_oracle(ep):
    """an Oracle for a stored episode: its world, scheme and recipes; no spawn block"""
    from golden_io import RECIPE_NAMES, recipe_table
    from cooking_zoo_amd.cooking_world.engine.load_level import load_meta_file
    from oracle_binding import Oracle
    dims = soa.Dims(*ep["dims"])
    rec0 = np.array(ep["states"][0]["record"], dtype=np.uint32)
    off, cells = static_table_of(dims, rec0)
    assert all(r in RECIPE_NAMES for r in ep["recipes"])
    return Oracle(dims, load_meta_file(ep["meta_file"]), recipe_table(), [(rec0, off, cells)], scheme=ep["scheme"], max_steps=1 << 30,
                  num_recipes=len(ep["recipes"]))


def world_step_of(oracle):
    """`Oracle.step_batch` as the `world_step` callable of effects.host_effects: an oracle without a spawn block (so no
    handle_agent_spawn), -1 passed through for agents that are not in the list; header words are not compared, so max_steps and the
    marks the oracle's step also updates are irrelevant.  The records handed in are never finished ones."""
    assert not oracle.ctx.spawn, "world_step_of: the oracle has a spawn block - its step would run handle_agent_spawn"

    def world_step(records, actions):
        recs = np.ascontiguousarray(records, dtype=np.uint32).copy()
        assert not (recs[:, soa.W_STATUS] & soa.STATUS_DONE).any(), "a finished env was handed to world_step"
        err = oracle.step_batch(recs, np.ascontiguousarray(actions, dtype=np.int32), want_obs=False)[0]
        assert err == 0, f"the oracle's step failed with {err}"
        return recs
    return world_step


def world_step_for(env):
    """... for the world of a CookingVecEnv / BatchTables"""
    from oracle_binding import VecOracle
    return world_step_of(VecOracle._from_vec_env(env, 1, 0, 0).oracle)        # (_from_vec_env: the twin without the spawn block)


def model(env, records):
    """effects uint8 [n, A, n_actions] of `records` by the host model over the oracle"""
    return effects.host_effects(world_step_for(env), records, env.dims, effects.num_actions(env.scheme_class.CODE))


class Census:
    """per scheme: how often every code was seen without / with an effect, and every bit clear / set (codes >= 1, live rows only)"""

    def __init__(self):
        self.codes, self.bits = {}, {}

    def add(self, scheme, eff, live=None):
        eff = np.asarray(eff).reshape(-1, eff.shape[-1])
        if live is not None:
            eff = eff[np.asarray(live).reshape(-1)]
        n_act = eff.shape[-1]
        codes = self.codes.setdefault(scheme, np.zeros((n_act, 2), dtype=np.int64))
        bits = self.bits.setdefault(scheme, np.zeros((len(BITS), 2), dtype=np.int64))
        for c in range(1, n_act):
            codes[c, 0] += int((eff[:, c] == 0).sum())
            codes[c, 1] += int((eff[:, c] != 0).sum())
        for k, b in enumerate(BITS):
            bits[k, 1] += int(((eff[:, 1:] & b) != 0).sum())
            bits[k, 0] += int(((eff[:, 1:] & b) == 0).sum())

    def check(self, ctx, schemes):
        for scheme in schemes:
            assert scheme in self.codes, f"{ctx}: no case of scheme {scheme}"
            codes, bits = self.codes[scheme], self.bits[scheme]
            for c in range(1, len(codes)):
                assert codes[c, 0] > 0 and codes[c, 1] > 0, f"{ctx}: scheme {scheme} code {c} was seen {codes[c, 0]} times without and {codes[c, 1]} times with an effect"
            for k, b in enumerate(BITS):
                assert bits[k, 0] > 0 and bits[k, 1] > 0, f"{ctx}: scheme {scheme} bit {effects.BIT_NAMES[b]} was clear {bits[k, 0]} times and set {bits[k, 1]} times"


def live_rows(records, A):
    """bool [n, A]: the env is not finished and the agent is present"""
    recs = np.asarray(records)
    done = (recs[:, soa.W_STATUS] & soa.STATUS_DONE) != 0
    gone = ((recs[:, soa.W_STATUS, None] >> (effects.SPAWN_GONE0 + np.arange(A))) & 1) != 0
    return ~done[:, None] & ~gone


# ---------------------------------------------------------------------------------------------------------------------------
# sentinel-filled device buffers of the two outputs
# ---------------------------------------------------------------------------------------------------------------------------

OUTPUTS = ("mask", "effects")
OUTPUT_SUBSETS = [("mask",), ("effects",), ("mask", "effects")]
SENT = dict(mask=0xA7, effects=0xE3)                                   # neither 0 / 1 nor a byte of the five bits


class EffectBufs:
    """the two outputs laid out for n envs, each with GUARD bytes behind the last row, all filled with their sentinels"""

    def __init__(self, env, n):
        self.n, self.A, self.n_act = n, env.num_agents, env.num_actions
        self.shape = (n, self.A, self.n_act)
        self.size = int(np.prod(self.shape))
        self.buf = {f: env.alloc((self.size + GUARD,), np.uint8) for f in OUTPUTS}
        self.fill()

    def fill(self):
        for f in OUTPUTS:
            self.buf[f].from_host(np.full(self.size + GUARD, SENT[f], dtype=np.uint8))

    def args(self, outputs):
        return {("d_" + f): self.buf[f] for f in outputs}

    def read(self, f):
        got = self.buf[f].to_host()
        return got[:self.size].reshape(self.shape), got[self.size:]

    def check(self, ctx, outputs, want_effects, agents=None, ignore=0, rows=None):
        """a named buffer holds the model's answer in rows `rows` (a slice of the env axis; None: all) of the chosen agents and its
        sentinel everywhere else, guard included; a buffer the call did not name keeps its sentinel everywhere"""
        chosen = (1 << self.A) - 1 if agents is None else agents
        asked = np.zeros(self.shape[:2], dtype=bool)
        asked[slice(None) if rows is None else rows] = [bool(chosen >> a & 1) for a in range(self.A)]
        want = dict(effects=np.asarray(want_effects, dtype=np.uint8), mask=effects.mask_of(want_effects, ignore))
        for f in OUTPUTS:
            body, guard = self.read(f)
            if f not in outputs:
                assert (body == SENT[f]).all() and (guard == SENT[f]).all(), f"{ctx}: {f} was not named and was written"
                continue
            assert (guard == SENT[f]).all(), f"{ctx}: {f}: a store went behind the last row"
            assert (body[~asked] == SENT[f]).all(), f"{ctx}: {f}: a row outside the range or of an agent that was not asked for was written"
            bad = np.argwhere(body[asked] != want[f][asked])
            assert not len(bad), (f"{ctx}: {f} differs from the host model at (asked row, code) {bad[:6].tolist()}: got "
                                  f"{body[asked][tuple(bad[0])]}, want {want[f][asked][tuple(bad[0])]}")
