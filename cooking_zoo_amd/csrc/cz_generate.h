// cz_generate.h -- level instantiation on the device (cz_generate_layouts): one wavefront draws one slot of the layout pool.
//
// Stands in for the reference building a new level at reset (cooking_env.py:191-195; engine/parsing.py:5-18 the base grid,
// :21-76 static objects, :79-115 dynamic objects, :118-151 agents) and for cooking_zoo_amd/cooking_world/layout.py
// (init_record, obs_descriptor), which turn the drawn level into the pool's two tables.  The level arrives as a "level program"
// (cooking_zoo_amd/cooking_world/engine/level_program.py describes the words); the n-th draw of slot s, generation g, in the
// reference's call order, is spawn_uniform(seed, s, g, GEN_TAG, n) - the host model is load_level.instantiate fed by
// level_program.KeyedDraws, and tests/golden/layouts_keyed_ref.json is the unmodified reference parser under that stream.
//
// The draws of one object are a rejection loop: each attempt's verdict depends on the grid as the previous OBJECT left it, not on
// the previous attempt.  So the wave evaluates 64 consecutive attempts at once - lane k takes the draws of attempt t0 + k, tests
// its candidate cell against the grid in LDS - and the first lane whose attempt ends the loop (ballot + count trailing zeros)
// decides; the draw counter advances by what the reference would have consumed up to there.  Everything between objects is
// wave-uniform.  Nothing is written to global memory before every reason to fail has been ruled out: a failed draw leaves the
// slot's record and descriptor as they were and adds one to the failure counter.
#pragma once
#include "cz_device.h"

namespace cz {

constexpr uint32_t GEN_MAGIC = 0x504C5A43u, GEN_TAG = 0x100u;      // level_program.MAGIC / LAYOUT_TAG
enum : uint32_t { GH_MAGIC = 0, GH_WORDS, GH_W, GH_H, GH_A, GH_F, GH_NSTATIC, GH_NDYN, GH_NAGENT, GH_NEXCL, GH_NMETA, GH_OFF_ENTRIES,
                  GH_OFF_EXCL, GH_OFF_META, GH_RESERVED, GH_D, GEN_HEADER_WORDS };
enum : uint32_t { GE_CLASS = 0, GE_COUNT, GE_CAP, GE_FLAGS, GE_OPT_LO, GE_OPT_HI, GE_NX, GE_NY, GEN_ENTRY_WORDS };
constexpr uint32_t GEN_CODE_DYN0 = 16, GEN_CODE_AGENT = 32, GEN_MAX_CANDIDATES = 1024;
constexpr uint32_t GEN_TRIES_OBJECT = 10000, GEN_TRIES_AGENT = 1000;        // parsing.py:73,112 / :149 (`time_out > N` raises)
// working bits of a grid byte beside the static type (bits 0..2): a dynamic object lies here, an agent stands here, the cell is in
// DYNAMIC_EXCLUDED_POSITIONS
enum : uint32_t { GEN_AGENT = 0x20, GEN_EXCLUDED = 0x40, GEN_OCCUPIED = 0x80 };

struct GenParams {
    uint32_t *lay_init;                 // [L][RW]
    uint32_t *lay_desc;                 // [L][F]
    uint16_t *lay_rank;                 // [L][W * H] the position of a cell's static object in world_objects[class]
    const uint32_t *programs;           // every level's program, one after the other
    const uint32_t *prog_off;           // [n_levels] word offset of a level's program
    const uint8_t *level_of_slot;       // [L]
    uint32_t *failures;
    uint64_t seed;
    uint32_t generation;
    int32_t first;
    int32_t RW, F, W, H, D, A, dyn0_off;
    uint32_t img_obj0, img_cell0, img_ag0, img_zero;      // halfword bases of the LDS image of the handle's kernel instance
};

__device__ __forceinline__ uint32_t gen_dw(uint32_t hw, uint32_t code = 0u) { return ((hw * 2u) & 0xFFFFu) | ((code * 4u) << 16); }

__global__ __launch_bounds__(64) void k_generate_layouts(const GenParams G) {
    __shared__ uint32_t grid32[256];                 // the working grid, one byte per cell
    __shared__ uint16_t st_cell[1024];               // static placements in creation order: cell, class
    __shared__ uint8_t st_cls[1024];
    __shared__ uint32_t dyn[256];                    // dynamic placements in creation order: x | y << 8 | class << 16 | rank in class << 24
    __shared__ uint32_t rec[(CELL_WORD0 + 256 + 2 * 255 + 15) / 16 * 16];     // the init record being built: the longest there is (32 x 32 cells, 255 slots)
    __shared__ uint32_t loaded[64];                  // objects accepted so far, by class code (world.loaded_object_counter)
    __shared__ uint32_t dyn_order[16], dyn_base[16], dyn_cap[16], agents[MAX_AGENTS];
    uint8_t *const grid = reinterpret_cast<uint8_t *>(grid32);
    const uint32_t lane = threadIdx.x;
    const uint32_t slot = (uint32_t)G.first + blockIdx.x;
    const uint32_t *__restrict__ P = G.programs + G.prog_off[G.level_of_slot[slot]];
    const uint32_t W = (uint32_t)G.W, H = (uint32_t)G.H, C = W * H, CW = (C + 3u) / 4u;

    // ---- parse_level_layout (parsing.py:5-18): the base grid, then the excluded cells as a flag
    for (uint32_t i = lane; i < CW; i += 64u) grid32[i] = P[GEN_HEADER_WORDS + i];
    loaded[lane] = 0u;
    if (lane < 16u) { dyn_order[lane] = 0u; dyn_base[lane] = 0u; dyn_cap[lane] = 0u; }
    __syncthreads();
    for (uint32_t i = lane; i < P[GH_NEXCL]; i += 64u) {
        const uint32_t w = P[P[GH_OFF_EXCL] + i], x = w & 0xFFFFu, y = w >> 16;
        if (x < W && y < H) grid[y * W + x] |= (uint8_t)GEN_EXCLUDED;
    }
    __syncthreads();

    // ---- the keyed stream: the first two mixing rounds of spawn_uniform are the same for every draw of the slot
    uint64_t kbase = spawn_mix(G.seed + 0x9E3779B97F4A7C15ull * (uint64_t)slot);
    kbase = spawn_mix(kbase ^ ((uint64_t)G.generation * 0xD1B54A32D192ED03ull)) ^ ((uint64_t)GEN_TAG << 32);
    auto uniform = [&](uint32_t n) { return (double)(spawn_mix(kbase ^ (uint64_t)n) >> 11) * (1.0 / 9007199254740992.0); };

    uint32_t n_draws = 0, n_static = 0, n_dyn = 0, n_dyn_classes = 0, n_agents = 0, n_switch = 0, agent_idx = 0;
    bool failed = false, agents_done = false;
    uint32_t pos = P[GH_OFF_ENTRIES];
    const uint32_t n_entries_sd = P[GH_NSTATIC] + P[GH_NDYN], n_entries = n_entries_sd + P[GH_NAGENT];
    for (uint32_t ei = 0; ei < n_entries && !failed && !agents_done; ++ei) {
        const uint32_t kind = ei < P[GH_NSTATIC] ? 0u : ei < n_entries_sd ? 1u : 2u;          // static, dynamic, agent
        const uint32_t cls = P[pos + GE_CLASS], count = P[pos + GE_COUNT], cap = P[pos + GE_CAP];
        const bool has_opt = (P[pos + GE_FLAGS] & 1u) && kind != 2u;                           // (parse_agents reads no OPTIONAL)
        const double optional = __hiloint2double((int)P[pos + GE_OPT_HI], (int)P[pos + GE_OPT_LO]);
        const uint32_t nx = P[pos + GE_NX], ny = P[pos + GE_NY];
        const uint32_t *xs = P + pos + GEN_ENTRY_WORDS, *ys = xs + nx;
        pos += GEN_ENTRY_WORDS + nx + ny;
        const uint32_t per = has_opt ? 3u : 2u;
        const uint32_t attempts = (kind == 2u ? GEN_TRIES_AGENT : GEN_TRIES_OBJECT) + 1u;
        for (uint32_t k = 0; k < count && !failed; ++k) {
            if (kind == 2u && ++agent_idx > (uint32_t)G.A) { agents_done = true; break; }      // parsing.py:124-126
            bool placed = false, stopped = false;
            uint32_t px = 0, py = 0;
            for (uint32_t t0 = 0; t0 < attempts; t0 += 64u) {
                const uint32_t t = t0 + lane, d = n_draws + t * per;
                // `optional <= random.random()` leaves the loop without an object (parsing.py:29-31, :87-89)
                const bool stop = has_opt && optional <= uniform(d);
                const uint32_t dx = d + (has_opt ? 1u : 0u);
                const uint32_t ix = min((uint32_t)(uniform(dx) * (double)nx), nx - 1u);
                const uint32_t iy = min((uint32_t)(uniform(dx + 1u) * (double)ny), ny - 1u);
                const uint32_t x = xs[ix], y = ys[iy];
                const bool inside = x < W && y < H;            // (a candidate on the far edge passes the reference's `>` test and finds no cell)
                const uint32_t g = inside ? grid[y * W + x] : 0xFFu;
                const bool fits = kind == 0u   ? (g & CELL_TYPE) <= COUNTER                      // a Counter or a Floor (parsing.py:37-76)
                                  : kind == 1u ? g == COUNTER                                     // a plain Counter, nothing on it, not excluded (:95-103)
                                               : (g & (CELL_TYPE | GEN_AGENT)) == FLOOR;          // a Floor no agent stands on (:134-140)
                const uint64_t m = ballot(t < attempts && (stop || (inside && fits)));
                if (m) {
                    const int l = __builtin_ctzll(m);
                    stopped = rdl((uint32_t)stop, l) != 0u;
                    px = rdl(x, l); py = rdl(y, l);
                    n_draws += (t0 + (uint32_t)l) * per + (stopped ? 1u : per);
                    placed = !stopped;
                    break;
                }
            }
            if (!placed && !stopped) { failed = true; break; }                                 // "Can't find valid position ..."
            if (!placed) continue;
            // take_meta: "Too many X objects loaded" (parsing.py:44, :99, :137)
            const uint32_t have = loaded[cls];
            if (cap <= have) { failed = true; break; }
            const uint32_t c = py * W + px;
            __syncthreads();
            loaded[cls] = have + 1u;
            if (kind == 0u) {
                grid[c] = (uint8_t)((grid[c] & ~CELL_TYPE) | cls);
                st_cell[n_static] = (uint16_t)c; st_cls[n_static] = (uint8_t)cls;
                ++n_static;
                n_switch += cls == SWITCH ? 1u : 0u;
            } else if (kind == 1u) {
                if (n_dyn >= 255u) { failed = true; break; }                                   // more objects than any record has slots
                const uint32_t dc = cls - GEN_CODE_DYN0, rank = dyn_cap[dc];
                if (rank == 0u) dyn_order[n_dyn_classes++] = dc;                               // world_objects key order: first creation
                dyn_cap[dc] = rank + 1u;
                dyn[n_dyn++] = px | (py << 8) | (dc << 16) | (rank << 24);
                grid[c] |= (uint8_t)GEN_OCCUPIED;
            } else {
                agents[n_agents++] = px | (py << 8);
                grid[c] |= (uint8_t)GEN_AGENT;
            }
            __syncthreads();
        }
    }
    // a second Switch (every LinkedObject shares one group: the reference crashes on the first press)
    failed = failed || n_switch > 1u;
    // slot table (layout.py): class-major in key order, Bread with head-room for its clones; must fit the record
    uint32_t slots = 0;
    if (!failed) {
        __syncthreads();
        for (uint32_t i = 0; i < n_dyn_classes; ++i) {
            const uint32_t dc = dyn_order[i], n = dyn_cap[dc];          // (dyn_cap held the count so far)
            __syncthreads();
            dyn_base[dc] = slots;
            dyn_cap[dc] = dc == BREAD ? 2u * n : n;
            slots += dc == BREAD ? 2u * n : n;
        }
        __syncthreads();
        failed = slots > (uint32_t)G.D;
    }
    // Counters left must fit the meta file's Counter features (obs_descriptor refuses; the reference would emit an over-long vector)
    uint32_t n_counter = 0;
    for (uint32_t c0 = 0; c0 < C; c0 += 64u) n_counter += (uint32_t)__popcll(ballot(c0 + lane < C && (grid[c0 + lane] & CELL_TYPE) == COUNTER));
    const uint32_t n_meta = P[GH_NMETA], off_meta = P[GH_OFF_META];
    for (uint32_t i = 0; i < n_meta; ++i)
        if (P[off_meta + 2u * i] == COUNTER && n_counter > P[off_meta + 2u * i + 1u]) failed = true;
    if (failed) {
        if (lane == 0u) atomicAdd(G.failures, 1u);
        return;
    }

    // ---- Layout.init_record: header, agents (orientation 1, empty hands), cells 4 per word, dyn0 in slot order
    const uint32_t RW = (uint32_t)G.RW, dyn0 = (uint32_t)G.dyn0_off;
    for (uint32_t i = lane; i < RW; i += 64u) {
        uint32_t v = 0u;
        if (i == W_LAYOUT) v = slot;
        else if (i == W_RECIPES) v = 0xFFFFFFFFu;
        else if (i >= (uint32_t)AGENT_WORD0 && i < (uint32_t)AGENT_WORD0 + n_agents && i < (uint32_t)AGENT_WORD0 + (uint32_t)G.A)
            v = agents[i - AGENT_WORD0] | (1u << 16);
        else if (i >= (uint32_t)CELL_WORD0 && i < (uint32_t)CELL_WORD0 + CW) v = grid32[i - CELL_WORD0] & 0x07070707u;
        rec[i] = v;
    }
    __syncthreads();
    for (uint32_t i = lane; i < n_dyn; i += 64u) {
        const uint32_t w = dyn[i], dc = (w >> 16) & 0xFFu, rank = w >> 24;
        rec[dyn0 + dyn_base[dc] + rank] = (w & 0xFFFFFFu) | D_ALIVE | D_FREE;
        if (dc == BREAD) rec[dyn0 + dyn_base[dc] + (dyn_cap[dc] >> 1) + rank] = BREAD << 16;      // clone head-room, not alive
    }
    __syncthreads();
    uint32_t *const out_rec = G.lay_init + (size_t)slot * RW;
    for (uint32_t i = lane; i < RW; i += 64u) out_rec[i] = rec[i];

    // ---- the rank table (the scripted partner's list order): Floor and Counter are what is left of the base grid, row-major; the
    // other classes in placement order - one store per static
    {
        uint16_t *const rk = G.lay_rank + (size_t)slot * C;
        for (uint32_t code = FLOOR; code <= BLENDER; ++code) {
            const bool base = code <= COUNTER;
            const uint32_t total = base ? C : n_static;
            uint32_t seen = 0;
            for (uint32_t j0 = 0; j0 < total; j0 += 64u) {
                const uint32_t j = j0 + lane;
                const bool mine = j < total && (base ? (grid[j] & CELL_TYPE) == code : st_cls[j] == code);
                const uint64_t m = ballot(mine);
                if (mine) rk[base ? j : st_cell[j]] = (uint16_t)(seen + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
                seen += (uint32_t)__popcll(m);
            }
        }
    }

    // ---- Layout.obs_descriptor: meta-file class order, list order inside a class, zero padding up to the meta count
    uint32_t *const out = G.lay_desc + (size_t)slot * (uint32_t)G.F;
    const uint32_t F = (uint32_t)G.F, zero = gen_dw(G.img_zero);
    auto put = [&](uint32_t at, uint32_t v) { if (at < F) out[at] = v; };
    uint32_t o = 0;
    for (uint32_t mi = 0; mi < n_meta; ++mi) {
        const uint32_t code = P[off_meta + 2u * mi], num = P[off_meta + 2u * mi + 1u];
        uint32_t flen = 0, emitted = 0;
        if (code < GEN_CODE_DYN0) {
            // world_objects[class] list order: Counters are what is left of the base grid, row-major; other classes in placement order
            flen = code == FLOOR ? 0u : (code == SWITCH || code == BLOCK) ? 4u : 3u;
            const uint32_t total = code == COUNTER ? C : n_static;
            for (uint32_t j0 = 0; flen && j0 < total; j0 += 64u) {
                const uint32_t j = j0 + lane;
                const bool mine = j < total && (code == COUNTER ? (grid[j] & CELL_TYPE) == COUNTER : st_cls[j] == code);
                const uint64_t m = ballot(mine);
                const uint32_t r = emitted + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (mine && r < num) {
                    const uint32_t cell = code == COUNTER ? j : st_cell[j], hw = G.img_cell0 + 4u * cell;
                    uint32_t at = o + r * flen;
                    put(at++, gen_dw(hw, 1u)); put(at++, gen_dw(hw + 1u, 2u));
                    if (flen == 4u) put(at++, gen_dw(hw + 2u));                 // switch_active / int(walkable)
                    put(at, gen_dw(hw + 3u));
                }
                emitted += (uint32_t)__popcll(m);
            }
        } else if (code < GEN_CODE_AGENT) {
            const uint32_t dc = code - GEN_CODE_DYN0;
            const bool blender_food = dc == CARROT || dc == BANANA;
            flen = dc == PLATE ? 3u : blender_food ? 6u : 5u;
            emitted = min(dyn_cap[dc], num);
            for (uint32_t k = lane; k < emitted; k += 64u) {
                const uint32_t hw = G.img_obj0 + 6u * (dyn_base[dc] + k);
                uint32_t at = o + k * flen;
                put(at++, gen_dw(hw, 1u)); put(at++, gen_dw(hw + 1u, 2u));
                if (dc != PLATE) {
                    put(at++, gen_dw(hw + 2u));                                  // int(not done())
                    put(at++, gen_dw(hw + 3u));                                  // chopped
                    if (blender_food) put(at++, gen_dw(hw + 4u));                // mashed
                }
                put(at, gen_dw(hw + 5u));
            }
        } else {
            flen = 7u;
            emitted = min((uint32_t)G.A, num);
            if (lane < emitted) {
                const uint32_t hw = G.img_ag0 + 8u * lane;
                uint32_t at = o + lane * flen;
                put(at++, gen_dw(hw, 4u + 2u * lane)); put(at++, gen_dw(hw + 1u, 5u + 2u * lane));
                for (uint32_t q = 0; q < 4u; ++q) put(at++, gen_dw(hw + 2u + q));
                put(at, gen_dw(hw + 6u));
            }
        }
        emitted = min(emitted, num);
        for (uint32_t at = o + emitted * flen + lane; at < o + num * flen; at += 64u) put(at, zero);
        o += num * flen;
    }
}

// cz_set_layout_group inside a stream capture of the caller: the one control word that changes, written by a launch
__global__ void k_set_layout_active(uint32_t *ctl, uint32_t active) {
    if (threadIdx.x == 0 && blockIdx.x == 0) ctl[LC_ACTIVE] = active;
}

}  // namespace cz
