"""Helpers of the render tests (host and GPU): the golden file of the reference's recorded draw ops, the census of what a
record and its ops show, the whole-canvas painter (the second route to a frame), a random-byte sprite sheet and sentinel-filled
device buffers.  Nothing here touches the device library."""
import functools
import gzip
import json
import os

import numpy as np

from cooking_zoo_amd import render, soa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_ref.json.gz")
TILE_SIZES = (80, 16, 7)
CENSUS_ITEMS = ["orientation1", "orientation2", "orientation3", "orientation4", "held_object", "plate_2_foods_on_counter",
                "plate_with_food_in_hands", "blender_on", "blender_off", "switch_on", "switch_off", "block_solid", "block_walkable",
                "four_agents", "non_square"]
OPTIONAL_ITEMS = ["food_stack_without_plate"]          # only if a seeded episode produces one (the golden's "census" says)


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


def golden_states():
    """(episode, dims, state) of every stored step"""
    for ep in golden()["episodes"]:
        dims = soa.Dims(*ep["dims"])
        for st in ep["states"]:
            yield ep, dims, st


def vis_mask(ep):
    return sum(1 << a for a, v in enumerate(ep["vis"]) if v == "robot")


def census(dims, record):
    """the CENSUS_ITEMS / OPTIONAL_ITEMS one record shows"""
    rec = np.asarray(record, dtype=np.uint32)
    out = set()
    agents = [soa.unpack_agent(rec[soa.AGENT_WORD0 + a]) for a in range(dims.A)]
    held = {h for _x, _y, _o, h in agents if h >= 0}
    for _x, _y, o, _h in agents:
        out.add(f"orientation{o}")
    if held:
        out.add("held_object")
    if dims.A == 4:
        out.add("four_agents")
    if dims.W != dims.H:
        out.add("non_square")
    for b in soa.record_cells(dims, rec):
        ty = int(b) & soa.CELL_TYPE_MASK
        if ty == soa.BLENDER:
            out.add("blender_on" if b & soa.CELL_TOGGLE else "blender_off")
        if ty == soa.SWITCH:
            out.add("switch_on" if b & soa.CELL_ACTIVE else "switch_off")
        if ty == soa.BLOCK:
            out.add("block_walkable" if b & soa.CELL_WALK else "block_solid")
    slots = [soa.unpack_dyn0(rec[dims.dyn0_word0 + s]) for s in range(dims.D)]
    inside = {}
    for s in range(dims.D):
        cont = soa.unpack_dyn1(rec[dims.dyn1_word0 + s])[0]
        if slots[s][3] & soa.DYN_ALIVE and cont >= 0:
            inside[cont] = inside.get(cont, 0) + 1
    for plate, n in inside.items():
        if plate in held:
            out.add("plate_with_food_in_hands")
        elif n >= 2:
            out.add("plate_2_foods_on_counter")
    groups = {}
    for x, y, cls, flags in slots:
        if flags & soa.DYN_ALIVE:
            groups.setdefault((x, y), []).append(cls)
    if any(len(g) >= 2 and soa.PLATE not in g for g in groups.values()):
        out.add("food_stack_without_plate")
    return out


def decode_ops(doc, ops):
    """the stored ops -> ("fill", rgb) | ("rect", rgb, x, y, w, h) | ("blit", name, (w, h), (raw x, raw y), (int x, int y))"""
    out = []
    for op in ops:
        if op[0] == "f":
            out.append(("fill", tuple(op[1:4])))
        elif op[0] == "r":
            out.append(("rect", tuple(op[1:4]), op[4], op[5], op[6], op[7]))
        else:
            out.append(("blit", doc["names"][op[1]], (op[2], op[3]), (op[4], op[5]), (op[6], op[7])))
    return out


def ops_by_cell(dims, P, ops):
    """the rect and blit ops as per-cell lists of (sprite, x0, y0, size) in draw order, and the fill / rect ops: the form of
    render.display_list"""
    cells = [[] for _ in range(dims.W * dims.H)]
    plain = []
    for op in ops:
        if op[0] == "fill":
            plain.append(op)
            continue
        if op[0] == "rect":
            plain.append(op)
            _k, _rgb, x, y, w, h = op
            assert w == h == P
            entry = (render.RECT, x, y, w)
        else:
            _k, name, (w, h), _raw, (x, y) = op
            assert w == h
            entry = (render.sprite_index(name), x, y, w)
        cells[(entry[2] // P) * dims.W + entry[1] // P].append(entry)
    return cells, plain


def paint_ops(dims, P, ops, sprites):
    """the plain whole-canvas painter: the ops in their recorded order onto one canvas uint8 [H * P][W * P][3]"""
    canvas = np.zeros((dims.H * P, dims.W * P, 3), dtype=np.uint8)
    M = sprites.shape[1]
    for op in ops:
        if op[0] == "fill":
            canvas[:, :] = op[1]
        elif op[0] == "rect":
            _k, rgb, x, y, w, h = op
            canvas[y:y + h, x:x + w] = rgb
        else:
            _k, name, (w, h), _raw, (x, y) = op
            if w == 0 or h == 0:
                continue
            src = sprites[render.sprite_index(name)].astype(np.int64)
            rows = np.array([py * M // h for py in range(h)]), np.array([px * M // w for px in range(w)])
            src = src[np.ix_(*rows)]                                                   # [h][w][4]
            dst = canvas[y:y + h, x:x + w].astype(np.int64)
            a = src[..., 3:]
            # round-half-up of the exact quotient, as an integer division (the blend identity test ties the two together)
            canvas[y:y + h, x:x + w] = ((2 * (src[..., :3] * a + dst * (255 - a)) + 255) // 510).astype(np.uint8)
    return canvas


def random_sheet(M, seed=0):
    """every byte random: every sampled byte matters (alpha 0 and 255 are forced into a few places)"""
    s = np.random.default_rng(1000 * M + seed).integers(0, 256, size=(render.N_SPRITES, M, M, 4), dtype=np.uint8)
    s[:, 0, 0, 3] = 0
    s[:, -1, -1, 3] = 255
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# sentinel-filled device buffers of the two outputs
# ---------------------------------------------------------------------------------------------------------------------------

FORMS = ("rgb8", "chw32")
FORM_SUBSETS = [("rgb8",), ("chw32",), ("rgb8", "chw32")]
GUARD_BYTES = 256
SENT_BYTE, SENT_F32 = 0xAB, 0x7FC00BAD          # the float32 one is a quiet NaN no pixel can be


class RenderBufs:
    """both outputs laid out for n frames, each with a guard behind it, all filled with their sentinels"""

    def __init__(self, env, n, P):
        h, w, _ = env.frame_shape(P)
        self.n, self.P = n, P
        self.shape = dict(rgb8=(n, h, w, 3), chw32=(n, 3, h, w))
        self.dtype = dict(rgb8=np.uint8, chw32=np.uint32)
        self.sent = dict(rgb8=SENT_BYTE, chw32=SENT_F32)
        self.size = {f: int(np.prod(s)) for f, s in self.shape.items()}
        self.guard = {f: GUARD_BYTES // np.dtype(self.dtype[f]).itemsize for f in FORMS}
        self.buf = {f: env.alloc((self.size[f] + self.guard[f],), self.dtype[f]) for f in FORMS}
        self.fill()

    def fill(self):
        for f in FORMS:
            self.buf[f].from_host(np.full(self.size[f] + self.guard[f], self.sent[f], dtype=self.dtype[f]))

    def args(self, forms):
        return {("d_" + f): self.buf[f] for f in forms}

    def check(self, ctx, forms, want_frames):
        """a named buffer holds `want_frames` (uint8 [n][h][w][3]) in every element and its guard is untouched; a buffer the
        call did not name keeps its sentinel everywhere"""
        want = dict(rgb8=want_frames, chw32=render.to_chw32(want_frames).view(np.uint32)) if forms else {}
        for f in FORMS:
            got = self.buf[f].to_host()
            body, guard = got[:self.size[f]].reshape(self.shape[f]), got[self.size[f]:]
            if f not in forms:
                assert (got == self.sent[f]).all(), f"{ctx}: {f} was not named and was written"
                continue
            assert (guard == self.sent[f]).all(), f"{ctx}: {f}: a store went behind the last frame"
            bad = np.argwhere(body != want[f])
            assert not len(bad), (f"{ctx}: {f} differs from the host model at {bad[:6].tolist()} ({len(bad)} elements): got "
                                  f"{body[tuple(bad[0])]:#x}, want {want[f][tuple(bad[0])]:#x}")
