// cz_query.h -- the read-only kernels, their argument blocks and constants: k_observe_grid, k_render, k_navigate, k_partner,
// k_action_effects and k_infos.  Each is a pure function of the records (no kernel here writes one); of the step path they use load_env, the
// constant block's coordinate table and, k_action_effects alone, the world step.
#pragma once
#include "cz_kernels.h"

namespace cz {

// The grid observation (cz_observe_grid_device): the (W, H, 32) state tensor the reference declares for obs_spaces=["full"]
// (cooking_env.py:118-123, 149-150, 274-278) and never fills, from the per-object vectors of world_objects.py
// (numeric_state_representation); cooking_zoo_amd/grid.py is the definition and the host model.  All channels are 0 / 1: one cell is
// one word of reference channels plus, `extended`, one word of which 16 bits are used.  A pure function of the record, in the shape
// of k_observe_f32: one wavefront per env and workgroup.
//   1. every lane ORs its alive slots' bits into the words of the slot's cell (LDS atomics, `acc`, record order c = y * W + x),
//      lanes a < NA the agents' bits; a slot or agent outside the grid (no valid record has one) is not drawn;
//   2. every lane takes its own cells, adds the static bit of the cell type and the mutable cell bits and puts the words at the
//      cell's place in the output order (`fin`, o = x * H + y; x and y from the constant block's coordinate table: no division);
//   3. the forms that were asked for (a uniform test each) go out in output order: `bits` one word or pair per lane, `grid8` two or
//      three 16-byte stores per lane, `grid32` with four lanes per cell - neighbouring lanes write neighbouring 16 bytes, 64 bytes per
//      cell and store.  Every channel of every cell is written, nothing behind the last cell; plain stores.
// Channels of a dynamic class / a cell type: 5 bits each, by class id (cooking_zoo_amd/grid.py DYN_CHANNEL, STATIC_CHANNEL)
constexpr uint64_t GRID_DYN_CHANNEL = 26ull | 24ull << 5 | 28ull << 10 | 22ull << 15 | 14ull << 20 | 17ull << 25 | 7ull << 30 | 5ull << 35 | 30ull << 40 | 11ull << 45;
constexpr uint64_t GRID_STATIC_CHANNEL = 21ull | 16ull << 5 | 20ull << 10 | 27ull << 15 | 10ull << 20 | 19ull << 25 | 9ull << 30;
constexpr uint32_t GRID_N_DYN = 10u, GRID_N_STATIC = 7u, GRID_CHOPPED_CLASSES = 0x1FEu;   // Onion .. Watermelon: a `chopped` channel behind the class's
enum : uint32_t { GX_CARROT_MASHED = 0, GX_BANANA_MASHED, GX_FRESH, GX_FREE, GX_HELD, GX_IN_PLATE, GX_CUT_READY, GX_BL_READY, GX_BL_TOGGLE,
                  GX_SW_ACTIVE, GX_BLOCK_WALK, GX_DESPAWNED, GX_AGENT0 };                  // bits of the second word (channel 32 + bit)
// four channel bits -> four bytes 0 / 1 (bit i of the nibble lands at bit 8 i: i + 7 i)
__device__ __forceinline__ uint32_t grid_bytes(uint32_t nibble) { return (nibble * 0x00204081u) & 0x01010101u; }
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_observe_grid(const Params P, int64_t env_begin, int32_t extended, uint32_t *bits_out, uint8_t *grid8_out,
                                                     float *grid32_out, int32_t *agent_xy_out) {
    constexpr int CELLS = 64 * CPL;
    __shared__ uint32_t acc[2][CELLS], fin[2][CELLS];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint32_t W = (uint32_t)P.W, H = (uint32_t)P.H, C = W * H;
    Ctx cx{P.W, P.H, P.D, P.W * P.H, (int)lane};
    const CoordWords<CPL> cw = load_coord_words<CPL>(P, (int)lane);
    Env<OPL, CPL, NA> e;
    load_env(P, e, cx, P.state + (size_t)(env_begin + i) * P.RW);
#pragma unroll
    for (int k = 0; k < CPL; ++k) acc[0][lane + 64u * k] = acc[1][lane + 64u * k] = 0u;
    __syncthreads();                                                  // (one wave: the LDS fence)
    uint32_t held[NA];                                                // slot + 1 in every agent's hands, 0: empty
#pragma unroll
    for (int a = 0; a < NA; ++a) held[a] = rdl(e.agw, a) >> 24;
#pragma unroll
    for (int k = 0; k < OPL; ++k) {
        const uint32_t d0 = e.d0[k], d1 = e.d1[k], s1 = lane + 64u * k + 1u;
        const uint32_t x = d0 & 0xFFu, y = (d0 >> 8) & 0xFFu, cls = (d0 >> 16) & 0xFFu;
        if ((d0 & D_ALIVE) && cls < GRID_N_DYN && x < W && y < H) {   // (lanes past D hold zeros)
            const uint32_t ch = (uint32_t)(GRID_DYN_CHANNEL >> (5u * cls)) & 31u;
            const bool chopped = (d0 & D_CHOPPED) && ((GRID_CHOPPED_CLASSES >> cls) & 1u), mashed = (d0 & D_MASHED) != 0u;
            bool in_hand = false;
#pragma unroll
            for (int a = 0; a < NA; ++a) in_hand = in_hand || held[a] == s1;
            const uint32_t w0 = (1u << ch) | (chopped ? 2u << ch : 0u);
            const uint32_t w1 = (uint32_t)(mashed && cls == CARROT) << GX_CARROT_MASHED | (uint32_t)(mashed && cls == BANANA) << GX_BANANA_MASHED |
                                (uint32_t)(cls != PLATE && !(d0 & D_DONE)) << GX_FRESH | (uint32_t)((d0 & D_FREE) != 0u) << GX_FREE |
                                (uint32_t)in_hand << GX_HELD | (uint32_t)((d1 & 0xFFu) != 0u) << GX_IN_PLATE;
            const uint32_t c = y * W + x;
            atomicOr(&acc[0][c], w0);
            atomicOr(&acc[1][c], w1);
        }
    }
    if (lane < (uint32_t)NA) {
        const uint32_t x = e.agw & 0xFFu, y = (e.agw >> 8) & 0xFFu, orient = (e.agw >> 16) & 0xFFu;
        if (x < W && y < H) {
            const uint32_t c = y * W + x;
            atomicOr(&acc[0][c], 1u | (orient - 1u < 4u ? 1u << orient : 0u));           // Agent: channels 0..4
            atomicOr(&acc[1][c], (1u << (GX_AGENT0 + lane)) | (((e.status >> (SPAWN_GONE0 + lane)) & 1u) << GX_DESPAWNED));
        }
        if (agent_xy_out) {
            int32_t *xy = agent_xy_out + ((size_t)i * NA + lane) * 2;
            xy[0] = (int32_t)x;
            xy[1] = (int32_t)y;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const uint32_t c = lane + 64u * k;
        if (c < C) {
            const uint32_t x = ((cw.w[k] & 0xFFFFu) >> 3) - (W - 1u), y = (cw.w[k] >> 19) - ((uint32_t)LUT_Y0 + H - 1u);
            const uint32_t cv = e.cell[k], ty = cv & CELL_TYPE;
            const uint32_t st = ty < GRID_N_STATIC ? 1u << ((uint32_t)(GRID_STATIC_CHANNEL >> (5u * ty)) & 31u) : 0u;
            const bool ready = (cv & CELL_READY) != 0u;
            const uint32_t w1 = (uint32_t)(ty == CUTBOARD && ready) << GX_CUT_READY | (uint32_t)(ty == BLENDER && ready) << GX_BL_READY |
                                (uint32_t)(ty == BLENDER && (cv & CELL_TOGGLE)) << GX_BL_TOGGLE | (uint32_t)(ty == SWITCH && (cv & CELL_ACTIVE)) << GX_SW_ACTIVE |
                                (uint32_t)(ty == BLOCK && (cv & CELL_WALK)) << GX_BLOCK_WALK;
            const uint32_t o = x * H + y;                             // (x < W, y < H: o < C)
            fin[0][o] = acc[0][c] | st;
            fin[1][o] = acc[1][c] | w1;
        }
    }
    __syncthreads();
    const uint32_t CH = extended ? 48u : 32u;
    if (bits_out) {
        uint32_t *out = bits_out + (size_t)i * C * (extended ? 2u : 1u);
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const uint32_t o = lane + 64u * k;
            if (o < C) {
                if (extended) stg<uint2_t>(out, o * 8u, uint2_t{fin[0][o], fin[1][o]});
                else stg<uint32_t>(out, o * 4u, fin[0][o]);
            }
        }
    }
    if (grid8_out) {
        uint8_t *out = grid8_out + (size_t)i * C * CH;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const uint32_t o = lane + 64u * k;
            if (o < C) {
                const uint32_t w0 = fin[0][o], w1 = fin[1][o];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if (q == 2 && !extended) break;
                    const uint32_t h = q == 0 ? w0 : q == 1 ? w0 >> 16 : w1;
                    stg<uint4_t>(out, o * CH + 16u * q, uint4_t{grid_bytes(h & 0xFu), grid_bytes((h >> 4) & 0xFu), grid_bytes((h >> 8) & 0xFu),
                                                                 grid_bytes((h >> 12) & 0xFu)});
                }
            }
        }
    }
    if (grid32_out) {
        float *out = grid32_out + (size_t)i * C * CH;
        const uint32_t sub = lane & 3u;
#pragma nounroll
        for (uint32_t o = lane >> 2; o < C; o += 16u) {
            const uint32_t w0 = fin[0][o], w1 = fin[1][o];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (q == 2 && !extended) break;
                const uint32_t chunk = 4u * q + sub;                  // 16 bytes = four channels from 4 * chunk
                const uint32_t n = ((q < 2 ? w0 : w1) >> ((4u * chunk) & 31u)) & 0xFu;
                const uint32_t one = 0x3F800000u;
                stg<uint4_t>(out, (o * CH + 4u * chunk) * 4u, uint4_t{(n & 1u) ? one : 0u, (n & 2u) ? one : 0u, (n & 4u) ? one : 0u, (n & 8u) ? one : 0u});
            }
        }
    }
}

// Frames (cz_render_device): the reference's GraphicPipeline.render (environment/game/graphic_pipeline.py) as a display list per
// cell composited per pixel; cooking_zoo_amd/render.py is the definition (display list, sampling, blend, deviations) and the host
// model.  A pure function of the record plus the sprite sheet; records are only read.  One workgroup of four wavefronts per
// (env, row of cells, band of RENDER_BAND pixel rows):
//   A. the first wave runs load_env and puts the slot words, the row's cell bytes, the agent words and the status word into LDS;
//      thread x < W owns cell (x, row): it counts the cell's draws (static 2, agents 2 each, the alive slots of the cell in slot
//      order), the W counts are summed into list starts, and the thread writes its cell's commands - sprite | x0 << 8 | y0 << 16
//      | size << 24 relative to the tile, and the multiplier that replaces the division by the size - at its start.  The list
//      holds every command of every record: a row has at most 2 W static, 2 NA agent and D slot commands (RENDER_CMDS), so
//      nothing is clipped whatever the record holds;
//   B. all threads share the band's (up to RENDER_BAND) x (W P) pixels.  A pixel finds its cell (a multiply and a shift: the API passes the
//      multipliers), starts from Color.FLOOR and walks the cell's commands in order, since every draw stays inside its tile.
//      Where the row pitch W * P * 3 is a multiple of 4 a thread owns 4 neighbouring pixels: three dword stores of rgb8, one
//      16-byte store per plane of chw32; otherwise one pixel: three byte stores, three float stores.  Every output byte is
//      written exactly once, nothing behind the last frame; plain stores.  chw32 goes through the 256-entry table v * (1 / 255).
constexpr int RENDER_BAND = 16;       // pixel rows per workgroup: a tile above 16 pixels is drawn by several workgroups (each repeats A)
constexpr int RENDER_THREADS = 256, RENDER_SPRITES = 40, RENDER_RECT = 255, RENDER_MAX_W = 32, RENDER_ROW_SHIFT = 31;
constexpr int RENDER_P_MIN = 4, RENDER_P_MAX = 128, RENDER_M_MAX = 128, RENDER_DIV_SHIFT = 21;
constexpr uint32_t RENDER_FLOOR_RGB = 245u | 230u << 8 | 210u << 16, RENDER_DELIVERY_RGB = 96u | 96u << 8 | 96u << 16;
// sprite numbers (cooking_zoo_amd/render.py SPRITES), 5 bits per dynamic class: fresh, chopped (mashed is the chopped one, for a
// Carrot the one behind it); 4 bits per cell type: plain, and with TOGGLE, ACTIVE or WALK set
constexpr uint64_t RENDER_DYN_FRESH = 9ull | 10ull << 5 | 12ull << 10 | 14ull << 15 | 16ull << 20 | 19ull << 25 | 20ull << 30 | 22ull << 35 | 24ull << 40 | 26ull << 45;
constexpr uint64_t RENDER_DYN_CHOPPED = 9ull | 11ull << 5 | 13ull << 10 | 15ull << 15 | 17ull << 20 | 19ull << 25 | 21ull << 30 | 23ull << 35 | 25ull << 40 | 27ull << 45;
constexpr uint32_t RENDER_CELL_PLAIN = 0u | 1u << 4 | 2u << 8 | 4u << 12 | 5u << 16 | 6u << 20 | 8u << 24, RENDER_CELL_SET = 0u | 1u << 4 | 2u << 8 | 3u << 12 | 0u << 16 | 6u << 20 | 7u << 24;
constexpr uint32_t RENDER_SPR_COUNTER = 1u, RENDER_SPR_HUMAN0 = 28u, RENDER_SPR_ROBOT0 = 32u, RENDER_SPR_ARROW0 = 36u;
struct RenderArgs {
    int64_t env_begin;
    const uint32_t *sheet;          // [RENDER_SPRITES][M][M] RGBA, one word per texel (r in the low byte)
    const float *ftab;              // [256]: v * (1 / 255)
    uint8_t *rgb8;                  // [count][H P][W P][3] or null
    float *chw32;                   // [count][3][H P][W P] or null
    uint32_t P, M, vis;
    uint32_t holding, container, holding_container, arrow, holding_off, container_off, holding_container_off;   // render.geometry(P)
    uint32_t mul_p;                 // floor(2^20 / P) + 1: px / P = px * mul_p >> 20 for px < 4096
    uint32_t mul_row;               // floor(2^31 / units per pixel row) + 1: u / units = u * mul_row >> 31 (64-bit product), u < 2^19
};
// floor(n / s) = n * render_mul(s) >> RENDER_DIV_SHIFT for n < s * RENDER_M_MAX, 1 <= s <= 128
__host__ __device__ inline uint32_t render_mul(uint32_t s) { return s ? (1u << RENDER_DIV_SHIFT) / s + 1u : 0u; }
__device__ __forceinline__ uint32_t render_tiles(uint32_t n) {        // floor(sqrt(n - 1)) + 1: the smallest t with t * t >= n
    uint32_t t = 1u;
    while (t * t < n) ++t;
    return t;
}
// one channel: round-half-up of (src a + dst (255 - a)) / 255
__device__ __forceinline__ uint32_t render_blend(uint32_t dst, uint32_t src, uint32_t a) {
    const uint32_t t = src * a + dst * (255u - a) + 128u;
    return (t + (t >> 8)) >> 8;
}
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(RENDER_THREADS) void k_render(const Params P, const RenderArgs G) {
    constexpr int SLOTS = 64 * OPL, MAX_W = RENDER_MAX_W, RENDER_CMDS = 2 * MAX_W + 2 * NA + SLOTS;
    static_assert(MAX_W <= 64, "one thread of the first wave per cell of a row");
    __shared__ uint32_t d0s[SLOTS], rowcell[MAX_W], ag[MAX_AGENTS], status_s, cnt[MAX_W], start[MAX_W];
    __shared__ uint32_t cmd[RENDER_CMDS], cmdmul[RENDER_CMDS];
    __shared__ float ftab[256];
    const uint32_t tid = threadIdx.x, W = (uint32_t)P.W, H = (uint32_t)P.H, D = (uint32_t)P.D;
    const uint32_t i = blockIdx.x / H, row = blockIdx.x - i * H;      // (uniform: one scalar division per workgroup)
    const uint32_t TP = G.P, M = G.M;
    ftab[tid] = G.ftab[tid];
    if (tid < 64u) {
        Ctx cx{P.W, P.H, P.D, P.W * P.H, (int)tid};
        Env<OPL, CPL, NA> e;
        load_env(P, e, cx, P.state + (size_t)(G.env_begin + i) * P.RW);
#pragma unroll
        for (int k = 0; k < OPL; ++k) d0s[tid + 64u * k] = e.d0[k];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const uint32_t c = tid + 64u * k - row * W;               // (wraps for the cells in front of the row)
            if (c < W) rowcell[c] = e.cell[k];
        }
        if (tid < (uint32_t)NA) ag[tid] = e.agw;
        if (tid == 0u) status_s = e.status;
    }
    __syncthreads();
    // ---- A: the cell's draws, counted and then written
    uint32_t n_dyn = 0u, n_plate = 0u, plate_at = 0u, n_total = 0u;
    bool agent_here = false;
    const uint32_t here = tid | row << 8;                             // x | y << 8 of this thread's cell
    if (tid < W) {
        const uint32_t ty = rowcell[tid] & CELL_TYPE;
        n_total = ty < 7u ? 2u : 0u;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const uint32_t w = ag[a], orient = (w >> 16) & 0xFFu;
            if ((w & 0xFFFFu) == here) {
                agent_here = true;
                if (!((status_s >> (SPAWN_GONE0 + a)) & 1u)) n_total += 1u + (uint32_t)(orient - 1u < 4u);
            }
        }
        for (uint32_t s = 0u; s < D; ++s) {
            const uint32_t d0 = d0s[s], cls = (d0 >> 16) & 0xFFu;
            if ((d0 & D_ALIVE) && cls < 10u && (d0 & 0xFFFFu) == here) {
                if (cls == PLATE && n_plate++ == 0u) plate_at = n_dyn;
                ++n_dyn;
            }
        }
        n_total += n_dyn;
        cnt[tid] = n_total;
    }
    __syncthreads();
    if (tid < W) {
        uint32_t at = 0u;
        for (uint32_t x = 0u; x < tid; ++x) at += cnt[x];
        start[tid] = at;
        const uint32_t cv = rowcell[tid], ty = cv & CELL_TYPE;
        const uint32_t mul_tile = render_mul(TP);
        if (ty < 7u) {
            cmd[at] = (ty == DELIVERSQUARE ? (uint32_t)RENDER_RECT : RENDER_SPR_COUNTER) | TP << 24;
            cmdmul[at++] = mul_tile;
            cmd[at] = ((((cv & (CELL_TOGGLE | CELL_ACTIVE | CELL_WALK)) ? RENDER_CELL_SET : RENDER_CELL_PLAIN) >> (4u * ty)) & 0xFu) | TP << 24;
            cmdmul[at++] = mul_tile;
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const uint32_t w = ag[a], orient = (w >> 16) & 0xFFu;
            if ((w & 0xFFFFu) == here && !((status_s >> (SPAWN_GONE0 + a)) & 1u)) {
                cmd[at] = ((((G.vis >> a) & 1u) ? RENDER_SPR_ROBOT0 : RENDER_SPR_HUMAN0) + (uint32_t)a) | TP << 24;
                cmdmul[at++] = mul_tile;
                if (orient - 1u < 4u) {                               // draw_agents: left, right, down, up
                    const uint32_t q = G.arrow, far = 3u * TP / 4u;
                    const uint32_t ax = orient == 1u ? 0u : orient == 2u ? far : q, ay = orient == 3u ? far : orient == 4u ? 0u : q;
                    cmd[at] = (RENDER_SPR_ARROW0 + orient - 1u) | ax << 8 | ay << 16 | q << 24;
                    cmdmul[at++] = render_mul(q);
                }
            }
        }
        if (n_dyn) {
            const uint32_t base = agent_here ? G.holding : TP, boff = agent_here ? G.holding_off : 0u;
            const uint32_t inner = agent_here ? G.holding_container : G.container, ioff = agent_here ? G.holding_container_off : G.container_off;
            const bool plated = n_plate == 1u;
            const uint32_t n_stack = plated ? n_dyn - 1u : n_dyn, sbase = plated ? inner : base, soff = plated ? ioff : boff;
            const uint32_t tiles = render_tiles(n_stack ? n_stack : 1u), size = sbase / tiles, mul_stack = render_mul(size), mul_base = render_mul(base);
            uint32_t k = 0u, idx = 0u, col = 0u, rowi = 0u;           // k: place in the group; idx = rowi * tiles + col: place in the stack
            for (uint32_t s = 0u; s < D; ++s) {
                const uint32_t d0 = d0s[s], cls = (d0 >> 16) & 0xFFu;
                if ((d0 & D_ALIVE) && cls < 10u && (d0 & 0xFFFFu) == here) {
                    const uint32_t spr = (d0 & D_CHOPPED) ? (uint32_t)(RENDER_DYN_CHOPPED >> (5u * cls)) & 31u
                                         : (d0 & D_MASHED) ? ((uint32_t)(RENDER_DYN_CHOPPED >> (5u * cls)) & 31u) + (uint32_t)(cls == CARROT)
                                                           : (uint32_t)(RENDER_DYN_FRESH >> (5u * cls)) & 31u;
                    if (plated && k == plate_at) {
                        cmd[at] = spr | boff << 8 | boff << 16 | base << 24;
                        cmdmul[at++] = mul_base;
                    } else {
                        cmd[at] = spr | (soff + size * col) << 8 | (soff + size * rowi) << 16 | size << 24;
                        cmdmul[at++] = mul_stack;
                        ++idx;
                        if (++col == tiles) { col = 0u; ++rowi; }
                    }
                    ++k;
                }
            }
        }
    }
    __syncthreads();
    // ---- B: the pixels of the row
    const uint32_t WP = W * TP, HP = H * TP;
    const bool wide = (WP & 3u) == 0u;
    const uint32_t per_row = wide ? WP >> 2 : WP, units = per_row * TP, NPIX = wide ? 4u : 1u;
    uint8_t *rgb = G.rgb8 ? G.rgb8 + ((size_t)i * HP + (size_t)row * TP) * WP * 3u : nullptr;
    float *pl = G.chw32 ? G.chw32 + (size_t)i * 3u * HP * WP + (size_t)row * TP * WP : nullptr;
    const size_t plane = (size_t)HP * WP;
    // blockIdx.y: which RENDER_BAND pixel rows of the row of cells this workgroup draws
    const uint32_t u_end = min(units, (blockIdx.y + 1u) * (uint32_t)RENDER_BAND * per_row);
    for (uint32_t u = blockIdx.y * (uint32_t)RENDER_BAND * per_row + tid; u < u_end; u += (uint32_t)RENDER_THREADS) {
        const uint32_t py = (uint32_t)(((uint64_t)u * G.mul_row) >> RENDER_ROW_SHIFT), px0 = (u - py * per_row) * NPIX;
        uint32_t r[4], g[4], b[4];
#pragma unroll
        for (uint32_t j = 0u; j < 4u; ++j) {
            if (j >= NPIX) break;
            const uint32_t px = px0 + j, cxl = (px * G.mul_p) >> 20, lx = px - cxl * TP;
            uint32_t cr = RENDER_FLOOR_RGB & 0xFFu, cg = (RENDER_FLOOR_RGB >> 8) & 0xFFu, cb = RENDER_FLOOR_RGB >> 16;
            const uint32_t c0 = start[cxl], c1 = c0 + cnt[cxl];
            for (uint32_t c = c0; c < c1; ++c) {
                const uint32_t w = cmd[c], size = w >> 24, dx = lx - ((w >> 8) & 0xFFu), dy = py - ((w >> 16) & 0xFFu);
                if (dx < size && dy < size) {                         // (unsigned: also false in front of the draw)
                    if ((w & 0xFFu) == (uint32_t)RENDER_RECT) {
                        cr = RENDER_DELIVERY_RGB & 0xFFu; cg = (RENDER_DELIVERY_RGB >> 8) & 0xFFu; cb = RENDER_DELIVERY_RGB >> 16;
                    } else {
                        const uint32_t m = cmdmul[c], sx = (dx * M * m) >> RENDER_DIV_SHIFT, sy = (dy * M * m) >> RENDER_DIV_SHIFT;
                        const uint32_t t = G.sheet[((w & 0xFFu) * M + sy) * M + sx], a = t >> 24;
                        cr = render_blend(cr, t & 0xFFu, a);
                        cg = render_blend(cg, (t >> 8) & 0xFFu, a);
                        cb = render_blend(cb, (t >> 16) & 0xFFu, a);
                    }
                }
            }
            r[j] = cr; g[j] = cg; b[j] = cb;
        }
        const uint32_t o = py * WP + px0;                             // pixel index inside the row of cells
        if (wide) {
            if (rgb) {
                stg<uint32_t>(rgb, o * 3u, r[0] | g[0] << 8 | b[0] << 16 | r[1] << 24);
                stg<uint32_t>(rgb, o * 3u + 4u, g[1] | b[1] << 8 | r[2] << 16 | g[2] << 24);
                stg<uint32_t>(rgb, o * 3u + 8u, b[2] | r[3] << 8 | g[3] << 16 | b[3] << 24);
            }
            if (pl) {
                typedef float float4_t __attribute__((ext_vector_type(4)));
                stg<float4_t>(pl, o * 4u, float4_t{ftab[r[0]], ftab[r[1]], ftab[r[2]], ftab[r[3]]});
                stg<float4_t>(pl + plane, o * 4u, float4_t{ftab[g[0]], ftab[g[1]], ftab[g[2]], ftab[g[3]]});
                stg<float4_t>(pl + 2u * plane, o * 4u, float4_t{ftab[b[0]], ftab[b[1]], ftab[b[2]], ftab[b[3]]});
            }
        } else {
            if (rgb) {
                stg<uint8_t>(rgb, o * 3u, (uint8_t)r[0]);
                stg<uint8_t>(rgb, o * 3u + 1u, (uint8_t)g[0]);
                stg<uint8_t>(rgb, o * 3u + 2u, (uint8_t)b[0]);
            }
            if (pl) {
                stg<float>(pl, o * 4u, ftab[r[0]]);
                stg<float>(pl + plane, o * 4u, ftab[g[0]]);
                stg<float>(pl + 2u * plane, o * 4u, ftab[b[0]]);
            }
        }
    }
}

// Shortest-path navigation (cz_navigate_device): BaseAgent.walk_to_location and reachable of the reference's scripted partner
// (cooking_agents/base_agent.py:62-126) for every agent of every env and up to NAV_MAX_TARGETS candidate goals each;
// cooking_zoo_amd/nav.py is the definition and the host model.  The reference searches breadth first from the agent over the Floor
// tiles, the goal admitted whatever it is, neighbours in the order of the walk codes 1:(-1,0) 2:(+1,0) 3:(0,+1) 4:(0,-1), and
// returns the first move of the first path found: the lexicographically smallest shortest path.  So no queue order is
// reproduced: a flood fill from the GOAL over the Floor set gives field[c], and the answer for a start s is the neighbour of s
// with the smallest field, the first code on ties (steps = field + 1; no finite neighbour: action 0, steps -1; s == g: 0, 0).
// A pure function of the record, one wavefront per env and workgroup:
//   1. the Floor set (with NAV_WALKABLE_BLOCKS: and the Blocks whose walkable bit is set) and the "not the first / last column"
//      sets are wave-uniform, a ballot per 64 cells over the cell lanes (record order c = y * W + x), as agents_walk builds
//      walk_set; the column comes from the constant block's coordinate table (no division);
//   2. lane q < NA * T owns query q = (agent q / T, candidate q % T) and runs the whole fill in its own registers on bit sets of
//      CPL 64-bit words: frontier -> (west | east | south | north of it) & floor & ~visited, the shifts by 1 masked by the column
//      sets, the shifts by W carried across words.  The lane looks at every frontier for the neighbours of its start (`nb`):
//      the first frontier that holds one answers action and steps without a distance array, and the lane's fill ends there;
//   3. with a field output (the second, slower instantiation of the body) the fill runs until its frontier is empty and the
//      lane stores the distance of every cell of every frontier, then 0xFFFF for the cells it never reached: every cell of the
//      field is written exactly once, at x * H + y (a transposition table in LDS).
// The fill loop runs at most W * H times whatever the record holds (no path is longer), and ends early once every lane's
// frontier is empty.  Plain stores; a target outside the grid is "no target" (action 0, steps -1, field all 0xFFFF), and so is
// an agent whose stored location is outside the grid (no valid record has one) - nothing is indexed unchecked.
constexpr int NAV_MAX_TARGETS = 8;
constexpr uint32_t NAV_WALKABLE_BLOCKS = 1u, NAV_KNOWN_FLAGS = NAV_WALKABLE_BLOCKS;
// the cells next to the cells of `s`
template <int CPL>
__device__ __forceinline__ Mask<CPL> nav_spread(const Mask<CPL> &s, const Mask<CPL> &not_first, const Mask<CPL> &not_last, uint32_t W) {
    Mask<CPL> east, west, r;                                          // who may step to x + 1 / x - 1
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        east.w[k] = s.w[k] & not_last.w[k];
        west.w[k] = s.w[k] & not_first.w[k];
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        uint64_t v = (east.w[k] << 1) | (west.w[k] >> 1) | (s.w[k] << W) | (s.w[k] >> W);           // (1 <= W <= 32)
        if (k > 0) v |= (east.w[k - 1] >> 63) | (s.w[k - 1] >> (64u - W));
        if (k + 1 < CPL) v |= (west.w[k + 1] << 63) | (s.w[k + 1] << (64u - W));
        r.w[k] = v;
    }
    return r;
}
// the x / y of a cell from its word of the constant block's coordinate table (no division)
__device__ __forceinline__ uint32_t coord_x(uint32_t cw, uint32_t W) { return ((cw & 0xFFFFu) >> 3) - (W - 1u); }
__device__ __forceinline__ uint32_t coord_y(uint32_t cw, uint32_t H) { return (cw >> 19) - ((uint32_t)LUT_Y0 + H - 1u); }
// word k of the wave-uniform sets of a fill, from the cell lanes (lane l: cell c = l + 64 k, its byte `cv`, its coordinate word
// `cw`): the cells a path may cross - Floor, with `blocks_too` = ~0 the Blocks whose walkable bit is set as well - and the cells that
// are not in the first / last column
__device__ __forceinline__ void nav_sets_word(uint32_t c, uint32_t cv, uint32_t cw, uint32_t W, uint32_t C, uint64_t blocks_too,
                                              uint64_t &floor, uint64_t &not_first, uint64_t &not_last) {
    const uint32_t x = coord_x(cw, W);
    const uint64_t inside = ballot(c < C);
    floor = (ballot((cv & CELL_TYPE) == FLOOR) | (ballot((cv & (CELL_TYPE | CELL_WALK)) == (BLOCK | CELL_WALK)) & blocks_too)) & inside;
    not_first = ballot(x != 0u);
    not_last = ballot(x != W - 1u);
}
// one round of a fill: the frontier becomes the cells of `floor` next to it that were not visited, and they are visited
template <int CPL>
__device__ __forceinline__ void nav_advance(Mask<CPL> &fr, Mask<CPL> &vis, const Mask<CPL> &floor, const Mask<CPL> &not_first,
                                            const Mask<CPL> &not_last, uint32_t W) {
    fr = nav_spread(fr, not_first, not_last, W) & floor;
    fr = fr.andnot(vis);
#pragma unroll
    for (int k = 0; k < CPL; ++k) vis.w[k] |= fr.w[k];
}
// the four neighbours of the start s = (sx, sy) that lie in the grid, as a set ...
template <int CPL>
__device__ __forceinline__ void nav_neighbours(Mask<CPL> &nb, uint32_t s, uint32_t sx, uint32_t sy, uint32_t W, uint32_t H) {
    if (sx > 0u) nb.set((int)(s - 1u));
    if (sx + 1u < W) nb.set((int)(s + 1u));
    if (sy + 1u < H) nb.set((int)(s + W));
    if (sy > 0u) nb.set((int)(s - W));
}
// ... and the first move when the frontier `fr` holds one of them: the first walk code in the order 1:(-1,0) 2:(+1,0) 3:(0,+1) 4:(0,-1)
template <int CPL>
__device__ __forceinline__ int32_t nav_first_code(const Mask<CPL> &fr, uint32_t s, uint32_t sx, uint32_t sy, uint32_t W, uint32_t H) {
    return (sx > 0u && fr.test((int)(s - 1u))) ? 1 : (sx + 1u < W && fr.test((int)(s + 1u))) ? 2 : (sy + 1u < H && fr.test((int)(s + W))) ? 3 : 4;
}
template <int CPL, int NA, bool FIELD>
__device__ __forceinline__ void navigate_env(const Params &P, int64_t env, uint32_t i, uint32_t T, uint32_t flags, const int32_t *target,
                                             int32_t *action_out, int32_t *steps_out, uint16_t *field_out, uint16_t *tr) {
    const uint32_t lane = threadIdx.x;
    const uint32_t W = (uint32_t)P.W, H = (uint32_t)P.H, C = W * H;
    const uint32_t *rec = P.state + (size_t)env * P.RW;
    const uint32_t aw = ldg<uint32_t>(rec, (AGENT_WORD0 + (lane & 3u)) * 4u);                     // lane a = agent a
    const uint64_t blocks_too = (flags & NAV_WALKABLE_BLOCKS) ? ~0ull : 0ull;
    Mask<CPL> floor, not_first, not_last;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const uint32_t c = lane + 64u * k;
        const uint32_t cv = ldg<uint8_t>(rec, CELL_WORD0 * 4u + min(c, C - 1u));                   // (clamped: inside the record)
        const uint32_t cw = ldg<uint32_t>(P.lut, COORD_TABLE_OFFSET + c * 4u);
        nav_sets_word(c, cv, cw, W, C, blocks_too, floor.w[k], not_first.w[k], not_last.w[k]);
        if (FIELD) tr[c] = (uint16_t)(c < C ? coord_x(cw, W) * H + coord_y(cw, H) : 0u);           // (c < C: x < W, y < H, below C)
    }
    if (FIELD) __syncthreads();                                                                    // (one wave: the LDS fence)
    const uint32_t nq = (uint32_t)NA * T;                                                          // (T <= 8: at most 32 queries)
    const bool mine = lane < nq;
    const uint32_t q = mine ? lane : 0u, a = q / T;
    uint32_t sw = 0u;
#pragma unroll
    for (int b = 0; b < NA; ++b) sw = a == (uint32_t)b ? rdl(aw, b) : sw;
    const uint32_t sx = sw & 0xFFu, sy = (sw >> 8) & 0xFFu;
    const size_t q0 = (size_t)i * nq + q;
    int32_t gx = -1, gy = -1;
    if (mine) {
        gx = target[q0 * 2];
        gy = target[q0 * 2 + 1];
    }
    const bool goal_in = (uint32_t)gx < W && (uint32_t)gy < H, start_in = sx < W && sy < H;
    const uint32_t g = goal_in ? (uint32_t)gy * W + (uint32_t)gx : 0u, s = start_in ? sy * W + sx : 0u;   // both below C
    Mask<CPL> vis = Mask<CPL>::zero(), nb = Mask<CPL>::zero();
    if (goal_in) vis.set((int)g);
    bool open = goal_in && start_in && s != g;                                                     // still looking for the first move
    if (open) {
        nav_neighbours(nb, s, sx, sy, W, H);
    }
    int32_t act = 0, steps = goal_in && start_in && s == g ? 0 : -1;
    uint16_t *field = FIELD && mine ? field_out + q0 * C : nullptr;
    if (FIELD && mine && goal_in) field[tr[g]] = (uint16_t)0;
    Mask<CPL> fr = vis;                                                                            // the cells whose field is d
#pragma nounroll
    for (uint32_t d = 0; d < C; ++d) {                                                             // the hard trip limit
        if (open && (fr & nb).any()) {
            steps = (int32_t)d + 1;
            act = nav_first_code(fr, s, sx, sy, W, H);
            open = false;
        }
        if (!FIELD && !open) fr = Mask<CPL>::zero();
        if (ballot(fr.any()) == 0ull) break;
        nav_advance(fr, vis, floor, not_first, not_last, W);
        if (FIELD && mine) {
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                for (uint64_t u = fr.w[k]; u; u &= u - 1ull) field[tr[64u * k + (uint32_t)__builtin_ctzll(u)]] = (uint16_t)(d + 1u);
            }
        }
    }
    if (mine) {
        if (action_out) action_out[q0] = act;
        if (steps_out) steps_out[q0] = steps;
        if (FIELD) {
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const uint64_t cells = 64u * (k + 1) <= C ? ~0ull : 64u * k < C ? (1ull << (C - 64u * k)) - 1ull : 0ull;
                for (uint64_t u = cells & ~vis.w[k]; u; u &= u - 1ull) field[tr[64u * k + (uint32_t)__builtin_ctzll(u)]] = (uint16_t)0xFFFFu;
            }
        }
    }
}
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_navigate(const Params P, int64_t env_begin, int32_t T, uint32_t flags, const int32_t *target,
                                                 int32_t *action_out, int32_t *steps_out, uint16_t *field_out) {
    __shared__ uint16_t tr[64 * CPL];
    const uint32_t i = blockIdx.x;
    if (field_out) navigate_env<CPL, NA, true>(P, env_begin + i, i, (uint32_t)T, flags, target, action_out, steps_out, field_out, tr);
    else navigate_env<CPL, NA, false>(P, env_begin + i, i, (uint32_t)T, flags, target, action_out, steps_out, nullptr, tr);
}

// The scripted partner (cz_partner_device): CookingAgent.step of the reference (cooking_agents/cooking_agent.py:9-119,
// base_agent.py:128-198) for the chosen agents of every env - which object to walk to, and the first move of the walk;
// cooking_zoo_amd/partner.py is the definition and the host model.  A pure function of the record, one wavefront per env and
// workgroup:
//   1. the off-step kernels' shared load puts cells and slots on the lanes; the wave stages them in LDS with, per cell, its
//      coordinates and its static object's rank in world_objects[class] (the layout pool's rank table), and builds the wave-uniform
//      sets: the cells of every static type and the Floor / column sets of the fill (ballots), the cells an object lies on directly
//      (LDS atomics);
//   2. lane a < NA is agent a.  One fill from the agent's cell over the Floor set, in the lane's registers (nav_advance), gives what
//      is reachable: the fill, its 4-neighbours and the agent's cell;
//   3. the lane evaluates update_recipe_state of the asked recipe from the partner table (matched-location sets per node in LDS),
//      takes the unmarked node with the highest index and runs the condition branch: candidates in list order, the first minimum of
//      (unmet conditions, squared distance, list rank), the first unmet condition in the node's order, generic_sequence - the
//      statics by sets, `closest` as the first minimum of (squared distance, list rank);
//   4. every lane with a goal walks (nav_route: the fill from the goal of k_navigate, all lanes together); a result of 0 falls
//      through to the contains branch: counts of matching child objects per cell, the main object, the nearest child object that is
//      not at its cell; and a second walk.
// Every loop is bounded by D, W * H, the node count (16) or the conditions of a node (8) whatever the record and the tables hold;
// a slot outside the grid or of no class (no valid record has one) is not an object, an agent outside the grid is IDLE.  The
// records are only read; plain stores; the entries of agents that are not driven are not written.
enum : uint32_t { PS_DONE = 0, PS_WALK, PS_IDLE, PS_RAISES, PS_ABSENT };
// partner table, one row per recipe: the node count, then per node  class | conditions << 8 | child mask << 16  and the conditions,
// 4 bits each in the node's order: attribute (0 chop_state, 1 blend_state) | wanted value << 1 (0 fresh, 1 chopped / in progress, 2 mashed)
constexpr int PARTNER_ROW_WORDS = 1 + 2 * WIDE_NODES, PARTNER_MAX_CONDS = 8;
struct PartnerArgs {
    int64_t env_begin;
    uint32_t agents;                   // bit a: agent a is driven
    int32_t n_recipes;
    const int32_t *recipe;             // [count][A] indices into the table, or null: the env's own
    const uint32_t *table;             // [n_recipes][PARTNER_ROW_WORDS]
    const uint16_t *lay_rank;          // [L][W * H]
    unsigned long long *bad_recipe;    // agents asked for a recipe outside the table
    int32_t *action, *target;
    uint8_t *status;
};
template <int OPL, int CPL, int NA>
struct PartnerLds {
    uint32_t d0[64 * OPL], d1[64 * OPL];
    uint32_t row[NA][PARTNER_ROW_WORDS + 3];
    uint64_t type[8][CPL];             // the cells of every static type
    uint64_t direct[CPL];              // the cells an object lies on directly (not held, not in a plate)
    uint64_t reach[NA][CPL];
    uint64_t locs[NA][WIDE_NODES][CPL];
    uint16_t xy[64 * CPL], rank[64 * CPL];
    uint8_t cnt[NA][64 * CPL];
};
// getattr(obj, attr) == value for a dynamic object (an attribute the class lacks meets nothing)
__device__ __forceinline__ bool partner_meets(uint32_t d0, uint32_t cond) {
    const uint32_t cls = (d0 >> 16) & 0xFFu, attr = cond & 1u, value = (cond >> 1) & 3u;
    if (cls == PLATE) return false;
    if (attr == 0u) return value == ((d0 & D_CHOPPED) ? 1u : 0u);
    if (cls != CARROT && cls != BANANA) return false;
    return value == ((d0 & D_MASHED) ? 2u : 0u);
}
__device__ __forceinline__ uint32_t partner_unmet(uint32_t d0, uint32_t nc, uint32_t conds) {
    uint32_t n = 0;
#pragma nounroll
    for (uint32_t q = 0; q < nc && q < (uint32_t)PARTNER_MAX_CONDS; ++q) n += partner_meets(d0, (conds >> (4u * q)) & 0xFu) ? 0u : 1u;
    return n;
}
// first move towards (gx, gy) for every lane with `go`, all lanes together: action 0 at the goal or when it is unreachable
template <int CPL>
__device__ __forceinline__ int32_t nav_route(const Mask<CPL> &floor, const Mask<CPL> &not_first, const Mask<CPL> &not_last, uint32_t W, uint32_t H,
                                             bool go, uint32_t sx, uint32_t sy, uint32_t gx, uint32_t gy) {
    const uint32_t C = W * H;
    const bool ok = go && gx < W && gy < H && sx < W && sy < H;
    const uint32_t g = ok ? gy * W + gx : 0u, s = ok ? sy * W + sx : 0u;
    Mask<CPL> vis = Mask<CPL>::zero(), nb = Mask<CPL>::zero();
    bool open = ok && s != g;
    if (open) {
        vis.set((int)g);
        nav_neighbours(nb, s, sx, sy, W, H);
    }
    int32_t act = 0;
    Mask<CPL> fr = vis;
#pragma nounroll
    for (uint32_t d = 0; d < C; ++d) {                                                             // the hard trip limit
        if (open && (fr & nb).any()) {
            act = nav_first_code(fr, s, sx, sy, W, H);
            open = false;
        }
        if (!open) fr = Mask<CPL>::zero();
        if (ballot(fr.any()) == 0ull) break;
        nav_advance(fr, vis, floor, not_first, not_last, W);
    }
    return act;
}
template <int OPL, int CPL, int NA>
struct Partner {
    using L = PartnerLds<OPL, CPL, NA>;
    L &s;
    uint32_t a, W, H, C, D, sx, sy, s0, held;          // this lane's agent, its cell, slot + 1 in its hands
    uint32_t held_all[NA];
    __device__ __forceinline__ static bool bit(const uint64_t *m, uint32_t c) { return (m[c >> 6] >> (c & 63u)) & 1ull; }
    __device__ __forceinline__ uint32_t d2(uint32_t c) const {
        const int32_t dx = (int32_t)(s.xy[c] & 0xFFu) - (int32_t)sx, dy = (int32_t)(s.xy[c] >> 8) - (int32_t)sy;
        return (uint32_t)(dx * dx + dy * dy);
    }
    // slot sl holds a live object of class `cls` inside the grid: its cell, else -1
    __device__ __forceinline__ int32_t object_cell(uint32_t sl, uint32_t cls) const {
        const uint32_t w = s.d0[sl], x = w & 0xFFu, y = (w >> 8) & 0xFFu;
        return ((w & D_ALIVE) && ((w >> 16) & 0xFFu) == cls && x < W && y < H) ? (int32_t)(y * W + x) : -1;
    }
    // the first minimum of (squared distance, list rank) over the reachable cells of a static type, `empty`: nothing lies on them
    __device__ __forceinline__ int32_t closest(uint32_t type, bool empty) const {
        uint32_t best = ~0u;
        int32_t at = -1;
#pragma nounroll
        for (int k = 0; k < CPL; ++k) {
            for (uint64_t u = s.type[type][k] & s.reach[a][k] & (empty ? ~s.direct[k] : ~0ull); u; u &= u - 1ull) {
                const uint32_t c = 64u * k + (uint32_t)__builtin_ctzll(u), key = d2(c) << 16 | s.rank[c];
                if (key < best) { best = key; at = (int32_t)c; }
            }
        }
        return at;
    }
    // update_recipe_state (recipe.py:77-104): the marks, and every node's matched locations in s.locs[a]
    __device__ __forceinline__ uint32_t marks(uint32_t n) {
        uint32_t m = 0;
#pragma nounroll
        for (int32_t j = (int32_t)n - 1; j >= 0; --j) {
            const uint32_t A = s.row[a][1 + 2 * j], conds = s.row[a][2 + 2 * j], cls = A & 0xFFu, nc = (A >> 8) & 0xFu, kids = (A >> 16) & ((1u << n) - 1u);
            uint64_t *mine = s.locs[a][j];
#pragma nounroll
            for (int k = 0; k < CPL; ++k) mine[k] = 0ull;
            if (kids & ~m) continue;
            bool any = false;
            if (cls < 7u && nc == 0u) {
#pragma nounroll
                for (int k = 0; k < CPL; ++k) {
                    uint64_t w = s.type[cls][k];
#pragma nounroll
                    for (uint32_t q = kids; q; q &= q - 1u) w &= s.locs[a][__builtin_ctz(q)][k];
                    mine[k] = w;
                    any = any || w != 0ull;
                }
            } else if (cls >= 16u && cls < 26u) {
#pragma nounroll
                for (uint32_t sl = 0; sl < D; ++sl) {
                    const int32_t c = object_cell(sl, cls - 16u);
                    if (c < 0 || partner_unmet(s.d0[sl], nc, conds)) continue;
                    bool ok = true;
#pragma nounroll
                    for (uint32_t q = kids; q; q &= q - 1u) ok = ok && bit(s.locs[a][__builtin_ctz(q)], (uint32_t)c);
                    if (ok) { mine[c >> 6] |= 1ull << (c & 63); any = true; }
                }
            }
            if (any) m |= 1u << j;
        }
        return m;
    }
    // the condition branch (cooking_agent.py:41-53, base_agent.py:140-190): PS_WALK with a goal cell, PS_RAISES, or PS_IDLE for
    // "0 without a walk" (the contains branch follows)
    __device__ __forceinline__ uint32_t condition(uint32_t j, int32_t &goal) const {
        const uint32_t A = s.row[a][1 + 2 * j], conds = s.row[a][2 + 2 * j], cls = A & 0xFFu, nc = (A >> 8) & 0xFu;
        int32_t bs = -1, bc = -1;                                       // the best object's slot (dynamic) and cell
        if (cls >= 16u && cls < 26u) {
            uint32_t best = ~0u;
#pragma nounroll
            for (uint32_t sl = 0; sl < D; ++sl) {
                const int32_t c = object_cell(sl, cls - 16u);
                if (c < 0) continue;
                const uint32_t key = partner_unmet(s.d0[sl], nc, conds) << 16 | d2((uint32_t)c);
                if (key < best) { best = key; bs = (int32_t)sl; bc = c; }
            }
        } else if (cls < 7u) {
            uint32_t best = ~0u;
#pragma nounroll
            for (int k = 0; k < CPL; ++k) {
                for (uint64_t u = s.type[cls][k]; u; u &= u - 1ull) {
                    const uint32_t c = 64u * k + (uint32_t)__builtin_ctzll(u), key = d2(c) << 16 | s.rank[c];
                    if (key < best) { best = key; bc = (int32_t)c; }
                }
            }
        }
        if (bc < 0) return PS_RAISES;                                   // IndexError, cooking_agent.py:48
        uint32_t appliance = 7u;
        bool unmet = false;
#pragma nounroll
        for (uint32_t q = 0; q < nc && q < (uint32_t)PARTNER_MAX_CONDS && !unmet; ++q) {
            const uint32_t cond = (conds >> (4u * q)) & 0xFu;
            if (bs >= 0 && partner_meets(s.d0[bs], cond)) continue;
            unmet = true;
            appliance = cond == (0u | 1u << 1) ? (uint32_t)CUTBOARD : cond == (1u | 2u << 1) ? (uint32_t)BLENDER : 7u;
        }
        if (!unmet || appliance == 7u) return PS_IDLE;
        // generic_sequence
        bool in_hands = false;
#pragma unroll
        for (int b = 0; b < NA; ++b) in_hands = in_hands || (bs >= 0 && held_all[b] == (uint32_t)bs + 1u);
        const bool lies = bs >= 0 && !in_hands && (s.d1[bs] & 0xFFu) == 0u;
        bool some_empty = false;
#pragma nounroll
        for (int k = 0; k < CPL; ++k) some_empty = some_empty || (s.type[appliance][k] & s.reach[a][k] & ~s.direct[k]) != 0ull;
        if (lies && bit(s.type[appliance], (uint32_t)bc) && bit(s.reach[a], (uint32_t)bc)) goal = bc;
        else if (bs >= 0 && held == (uint32_t)bs + 1u) goal = some_empty ? closest(appliance, true) : closest(COUNTER, false);
        else if (some_empty) goal = held ? closest(COUNTER, true) : bc;
        else goal = closest(appliance, false);
        return goal < 0 ? PS_RAISES : PS_WALK;                          // TypeError, base_agent.py:64
    }
    // the contains branch (cooking_agent.py:26-39, 55-119)
    __device__ __forceinline__ uint32_t contains(uint32_t j, uint32_t n, int32_t &goal) {
        const uint32_t A = s.row[a][1 + 2 * j], cls = A & 0xFFu, kids = (A >> 16) & ((1u << n) - 1u);
        uint8_t *cnt = s.cnt[a];
#pragma nounroll
        for (uint32_t q = kids; q; q &= q - 1u) {
            const uint32_t kj = (uint32_t)__builtin_ctz(q), KA = s.row[a][1 + 2 * kj], kconds = s.row[a][2 + 2 * kj], kcls = KA & 0xFFu, knc = (KA >> 8) & 0xFu;
            if (kcls >= 16u && kcls < 26u) {
#pragma nounroll
                for (uint32_t sl = 0; sl < D; ++sl) {
                    const int32_t c = object_cell(sl, kcls - 16u);
                    if (c >= 0 && bit(s.reach[a], (uint32_t)c) && !partner_unmet(s.d0[sl], knc, kconds) && cnt[c] < 255u) cnt[c]++;
                }
            } else if (kcls < 7u && knc == 0u) {
#pragma nounroll
                for (int k = 0; k < CPL; ++k)
                    for (uint64_t u = s.type[kcls][k] & s.reach[a][k]; u; u &= u - 1ull) {
                        const uint32_t c = 64u * k + (uint32_t)__builtin_ctzll(u);
                        if (cnt[c] < 255u) cnt[c]++;
                    }
            }
        }
        int32_t main = -1;
        uint64_t best = ~0ull;                                          // most objects, then nearest, then first in the list
        if (cls >= 16u && cls < 26u) {
#pragma nounroll
            for (uint32_t sl = 0; sl < D; ++sl) {
                const int32_t c = object_cell(sl, cls - 16u);
                if (c < 0 || !bit(s.reach[a], (uint32_t)c)) continue;
                const uint64_t key = (uint64_t)(255u - cnt[c]) << 32 | (uint64_t)d2((uint32_t)c) << 16;
                if (key < best) { best = key; main = c; }
            }
        } else if (cls < 7u) {
#pragma nounroll
            for (int k = 0; k < CPL; ++k)
                for (uint64_t u = s.type[cls][k] & s.reach[a][k]; u; u &= u - 1ull) {
                    const uint32_t c = 64u * k + (uint32_t)__builtin_ctzll(u);
                    const uint64_t key = (uint64_t)(255u - cnt[c]) << 32 | (uint64_t)d2(c) << 16 | s.rank[c];
                    if (key < best) { best = key; main = (int32_t)c; }
                }
        }
        int32_t child = -1;
        uint32_t bd = ~0u;
        bool orphan = false;                                            // a reachable child object while there is no main object
#pragma nounroll
        for (uint32_t q = kids; q; q &= q - 1u) {
            const uint32_t kcls = s.row[a][1 + 2 * __builtin_ctz(q)] & 0xFFu;
            if (kcls >= 16u && kcls < 26u) {
#pragma nounroll
                for (uint32_t sl = 0; sl < D; ++sl) {
                    const int32_t c = object_cell(sl, kcls - 16u);
                    if (c < 0 || !bit(s.reach[a], (uint32_t)c)) continue;
                    orphan = orphan || main < 0;
                    if (c != main && d2((uint32_t)c) < bd) { bd = d2((uint32_t)c); child = c; }
                }
            } else if (kcls < 7u) {
                uint32_t kb = ~0u;
                int32_t kc = -1;
#pragma nounroll
                for (int k = 0; k < CPL; ++k)
                    for (uint64_t u = s.type[kcls][k] & s.reach[a][k]; u; u &= u - 1ull) {
                        const uint32_t c = 64u * k + (uint32_t)__builtin_ctzll(u), key = d2(c) << 16 | s.rank[c];
                        orphan = orphan || main < 0;
                        if ((int32_t)c != main && key < kb) { kb = key; kc = (int32_t)c; }
                    }
                if (kc >= 0 && (kb >> 16) < bd) { bd = kb >> 16; child = kc; }
            }
        }
        if (orphan) return PS_RAISES;                                   // AttributeError, cooking_agent.py:63
        if (child < 0) return PS_IDLE;
        goal = (uint32_t)child == s0 ? main : child;
        return PS_WALK;
    }
};
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_partner(const Params P, const PartnerArgs G) {
    __shared__ PartnerLds<OPL, CPL, NA> s;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint32_t W = (uint32_t)P.W, H = (uint32_t)P.H, C = W * H, D = (uint32_t)P.D;
    Ctx cx{P.W, P.H, P.D, P.W * P.H, (int)lane};
    const CoordWords<CPL> cw = load_coord_words<CPL>(P, (int)lane);
    Env<OPL, CPL, NA> e;
    load_env(P, e, cx, P.state + (size_t)(G.env_begin + i) * P.RW);
    Mask<CPL> floor, not_first, not_last;
#pragma unroll
    for (int k = 0; k < CPL; ++k) nav_sets_word(lane + 64u * k, e.cell[k], cw.w[k], W, C, 0ull, floor.w[k], not_first.w[k], not_last.w[k]);
    const uint16_t *ranks = G.lay_rank + (size_t)min(e.layout, (uint32_t)P.L - 1u) * C;            // (clamped: inside the table)
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const uint32_t c = lane + 64u * k, ty = e.cell[k] & CELL_TYPE;
        s.xy[c] = (uint16_t)(c < C ? coord_x(cw.w[k], W) | coord_y(cw.w[k], H) << 8 : 0xFFFFu);
        s.rank[c] = c < C ? ldg<uint16_t>(ranks, c * 2u) : (uint16_t)0;
        s.cnt[0][c] = 0;
        if (NA > 1) s.cnt[1 % NA][c] = 0;
        if (NA > 2) s.cnt[2 % NA][c] = 0;
        if (NA > 3) s.cnt[3 % NA][c] = 0;
#pragma unroll
        for (uint32_t t = 0; t < 8u; ++t) {
            const uint64_t m = ballot(c < C && ty == t);
            if (lane == 0u) s.type[t][k] = m;
        }
    }
#pragma unroll
    for (int k = 0; k < OPL; ++k) {
        s.d0[lane + 64u * k] = e.d0[k];                                // (lanes past D hold zeros: not alive)
        s.d1[lane + 64u * k] = e.d1[k];
    }
    if (lane < (uint32_t)CPL) s.direct[lane] = 0ull;
    __syncthreads();                                                   // (one wave: the LDS fence)
    uint32_t held_all[NA];
#pragma unroll
    for (int b = 0; b < NA; ++b) held_all[b] = rdl(e.agw, b) >> 24;
#pragma unroll
    for (int k = 0; k < OPL; ++k) {
        const uint32_t d0 = e.d0[k], x = d0 & 0xFFu, y = (d0 >> 8) & 0xFFu, s1 = lane + 64u * k + 1u;
        bool in_hands = false;
#pragma unroll
        for (int b = 0; b < NA; ++b) in_hands = in_hands || held_all[b] == s1;
        if ((d0 & D_ALIVE) && ((d0 >> 16) & 0xFFu) < 10u && x < W && y < H && !in_hands && (e.d1[k] & 0xFFu) == 0u) {
            const uint32_t c = y * W + x;
            atomicOr(reinterpret_cast<unsigned long long *>(&s.direct[c >> 6]), 1ull << (c & 63u));
        }
    }
    // who is asked for what
    const bool agent = lane < (uint32_t)NA && ((G.agents >> lane) & 1u);
    const size_t out = (size_t)i * NA + (agent ? lane : 0u);
    const uint32_t sx = e.agw & 0xFFu, sy = (e.agw >> 8) & 0xFFu;
    uint32_t status = PS_IDLE;
    int32_t recipe = -1;
    if (agent) {
        if ((e.status >> (SPAWN_GONE0 + lane)) & 1u) status = PS_ABSENT;
        else if (G.recipe) {
            recipe = G.recipe[out];
            if (recipe < 0 || recipe >= G.n_recipes) { recipe = -1; atomicAdd(G.bad_recipe, 1ull); }
        } else {
            recipe = (int32_t)((e.recipes >> (8u * lane)) & 0xFFu);
            if (recipe == 0xFF) { recipe = -1; status = PS_DONE; }
            else if (recipe >= G.n_recipes) { recipe = -1; atomicAdd(G.bad_recipe, 1ull); }
        }
    }
    bool busy = agent && recipe >= 0 && sx < W && sy < H;              // still deciding
#pragma unroll
    for (int b = 0; b < NA; ++b) {                                     // the rows of the asked recipes, one agent after the other
        const int32_t r = (int32_t)rdl((uint32_t)recipe, b);
        if (r >= 0 && lane < (uint32_t)PARTNER_ROW_WORDS) s.row[b][lane] = ldg<uint32_t>(G.table, ((uint32_t)r * PARTNER_ROW_WORDS + lane) * 4u);
    }
    // the agent's reachability: one fill from its cell
    const uint32_t s0 = busy ? sy * W + sx : 0u;
    {
        Mask<CPL> vis = Mask<CPL>::zero();
        if (busy) vis.set((int)s0);
        Mask<CPL> fr = vis;
#pragma nounroll
        for (uint32_t d = 0; d < C; ++d) {                             // the hard trip limit
            if (ballot(fr.any()) == 0ull) break;
            nav_advance(fr, vis, floor, not_first, not_last, W);
        }
        const Mask<CPL> near = nav_spread(vis, not_first, not_last, W);
        if (lane < (uint32_t)NA) {
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const uint64_t inside = 64u * (k + 1) <= C ? ~0ull : 64u * k < C ? (1ull << (C - 64u * k)) - 1ull : 0ull;
                s.reach[lane][k] = (vis.w[k] | near.w[k]) & inside;
            }
        }
    }
    __syncthreads();
    Partner<OPL, CPL, NA> p{s, lane < (uint32_t)NA ? lane : 0u, W, H, C, D, sx, sy, s0, e.agw >> 24, {}};
#pragma unroll
    for (int b = 0; b < NA; ++b) p.held_all[b] = held_all[b];
    uint32_t node = 0, n = 0;
    int32_t goal = -1;
    bool go = false;
    if (busy) {
        n = min(s.row[p.a][0], (uint32_t)WIDE_NODES);
        const uint32_t left = ~p.marks(n) & ((1u << n) - 1u);
        if (!left) { status = PS_DONE; busy = false; }
        else {
            node = 31u - (uint32_t)__builtin_clz(left);
            const uint32_t r = p.condition(node, goal);
            if (r == PS_RAISES) { status = PS_RAISES; busy = false; }
            go = r == PS_WALK;
        }
    }
    int32_t act = nav_route<CPL>(floor, not_first, not_last, W, H, go, sx, sy, go ? s.xy[goal] & 0xFFu : 0u, go ? s.xy[goal] >> 8 : 0u);
    if (busy && go && act) { status = PS_WALK; busy = false; }
    go = false;
    if (busy) {                                                        // 0 from the condition branch: the contains branch
        goal = -1;
        const uint32_t r = p.contains(node, n, goal);
        status = r;
        go = r == PS_WALK && goal >= 0;
        if (r == PS_WALK && goal < 0) status = PS_IDLE;
    }
    const int32_t act2 = nav_route<CPL>(floor, not_first, not_last, W, H, go, sx, sy, go ? s.xy[goal] & 0xFFu : 0u, go ? s.xy[goal] >> 8 : 0u);
    if (go) act = act2;
    if (agent) {
        const bool walked = status == PS_WALK;
        if (G.action) G.action[out] = walked ? act : 0;
        if (G.target) {
            G.target[out * 2] = walked ? (int32_t)(s.xy[goal] & 0xFFu) : -1;
            G.target[out * 2 + 1] = walked ? (int32_t)(s.xy[goal] >> 8) : -1;
        }
        if (G.status) G.status[out] = (uint8_t)status;
    }
}

// Action effects and masks (cz_action_effects_device): which of an agent's actions would do anything at all;
// cooking_zoo_amd/effects.py is the definition and the host model.  For an env whose done bit is clear, a present agent a and a code
// c of the env's scheme (0 .. n_actions - 1; 5 codes in scheme3, 8 in scheme1): S0 is the record after world_step with every present
// agent playing 0, Sc the record after world_step with agent a playing c and every other present agent playing 0 - world_step being
// perform_agent_actions + progress_world + the linked interactions + the free-flag normalisation (cooking_world.py:104-108), without
// handle_agent_spawn, t, recipe marks, rewards or flags; a despawned agent takes no part (action -1).  S0 is not S: a running Blender
// progresses by itself.  effects[a][c] has one bit per difference between Sc and S0, in the words store_env would write:
// MOVED agent a's (x, y), TURNED its orientation, HAND its held-slot field, OBJECTS any dyn0 / dyn1 word, CELLS any cell byte.
// effects[a][0] = 0; mask[a][c] = 1 if c == 0 or (effects[a][c] & ~ignore) != 0.  A despawned agent and every agent of a finished
// env get mask [1, 0, ...] and effects 0.  The mask speaks about one agent acting alone.
// One wavefront per (env, agent) and workgroup, no wave talks to another; the records are only read.  A wave whose agent is not in
// `agents` leaves at once and writes nothing; one whose agent is despawned or whose env is done leaves behind one load and writes the
// noop-only row.  The others load the env once and run the trials c = 0 .. n_actions - 1 serially on copies of it, in one loop that
// is not unrolled - the dynamics stand once in the kernel's code, the code c is a run-time value of lane a -, trial 0 being S0.
// Every trial runs the free-flag normalisation (Dirty::interacted set): the step kernels skip it on steps without an interaction,
// where it changes nothing on a record the step kernels made; here both sides of the comparison are normalised whatever the record.
// Nothing of Dirty is taken for the answer: the bits are per-lane compares of the slots below D and the cells below W * H, reduced
// by ballots, and three field compares of lane a's agent word.  Lane c keeps trial c's byte; lanes c < n_actions store one byte per
// form that was asked for (plain stores): rows uint8 [count][A][n_actions], dense, every element of a written row exactly once.
enum : uint32_t { FX_MOVED = 1, FX_TURNED = 2, FX_HAND = 4, FX_OBJECTS = 8, FX_CELLS = 16, FX_ALL = 31 };
struct EffectsArgs {
    int64_t env_begin;
    uint32_t agents;                   // bit a: agent a is asked for
    uint32_t ignore;                   // FX_ bits that do not make an action count
    uint8_t *mask, *effects;           // [count][A][n_actions], either may be null
};
template <int OPL, int CPL, int NA, int SCHEME>
__global__ __launch_bounds__(64) void k_action_effects(const Params P, const EffectsArgs G) {
    constexpr uint32_t N_ACT = SCHEME == 3 ? 5u : 8u;
    using O = Ops<OPL, CPL, NA, SCHEME>;
    const uint32_t i = blockIdx.x / (uint32_t)NA, a = blockIdx.x % (uint32_t)NA, lane = threadIdx.x;
    if (!((G.agents >> a) & 1u)) return;
    const uint32_t *rec = P.state + (size_t)(G.env_begin + i) * P.RW;
    const uint32_t st = rfl(rec[W_STATUS]);
    uint32_t fx = 0u;                                                  // lane c: the byte of trial c
    if (!(st & ST_DONE) && !((st >> ((uint32_t)SPAWN_GONE0 + a)) & 1u)) {
        Ctx cx{P.W, P.H, P.D, P.W * P.H, (int)lane};
        Env<OPL, CPL, NA> e, s0;
        load_env(P, e, cx, rec);
        uint64_t slots[OPL], cells[CPL];                               // what a record holds: the lanes' slots below D, cells below W * H
#pragma unroll
        for (int k = 0; k < OPL; ++k) slots[k] = ballot(lane + 64u * k < (uint32_t)cx.D);
#pragma unroll
        for (int k = 0; k < CPL; ++k) cells[k] = ballot(lane + 64u * k < (uint32_t)cx.C);
        s0 = e;
#pragma nounroll
        for (uint32_t c = 0; c < N_ACT; ++c) {
            Env<OPL, CPL, NA> t = e;
            Dirty dt{};
            dt.interacted = 1;
            O::perform_agent_actions(t, cx, lane == a ? c : 0u, dt);
            O::progress_and_link(t, cx, dt);
            if (c == 0u) {
                s0 = t;
            } else {
                uint64_t objs = 0ull, cellb = 0ull;
#pragma unroll
                for (int k = 0; k < OPL; ++k) objs |= (ballot(t.d0[k] != s0.d0[k]) | ballot(t.d1[k] != s0.d1[k])) & slots[k];
#pragma unroll
                for (int k = 0; k < CPL; ++k) cellb |= ballot(((t.cell[k] ^ s0.cell[k]) & 0xFFu) != 0u) & cells[k];
                const uint32_t x = rdl(t.agw ^ s0.agw, (int)a);
                const uint32_t byte = ((x & 0xFFFFu) ? FX_MOVED : 0u) | ((x & 0xFF0000u) ? FX_TURNED : 0u) | ((x >> 24) ? FX_HAND : 0u) |
                                      (objs ? FX_OBJECTS : 0u) | (cellb ? FX_CELLS : 0u);
                fx = lane == c ? byte : fx;
            }
        }
    }
    if (lane < N_ACT) {
        const size_t row = ((size_t)i * NA + a) * N_ACT;
        if (G.effects) stg<uint8_t>(G.effects + row, lane, (uint8_t)fx);
        if (G.mask) stg<uint8_t>(G.mask + row, lane, (uint8_t)((lane == 0u || (fx & ~G.ignore) != 0u) ? 1u : 0u));
    }
}

// The task state of every env as tensors (cz_infos_device; definition: cooking_zoo_amd/tasks.py host_infos): what the reference's
// infos and "full" observation report per agent - goal_vector = recipe_mapping[agent].goals_completed(num_goals) (cooking_env.py:277,
// recipe.py:36-40), recipe_done and task (cooking_env.py:317-331) - and the env's step counter.  It needs four header words of the
// record (t, marks, marks-hi, recipe ids), the recipe table's node counts and `counts` bits and the goal table: no load_env, no
// image, and nothing of the kernel instance - one kernel for all three, by the width of the recipe tables.
// One wavefront per env, INFOS_WAVES of them per workgroup, no wave talks to another (an idle wave of the last workgroup leaves at
// once).  Lane 16 a + j stands for node j of the recipe of slot a: the node whose `counts` bit is set is the last of node_list with
// its goal id (Recipe.flatten) and puts `not marked` at [a][id] of the env's [A][G] row in LDS, which the wave has zeroed before (ids
// no node carries stay 0; the DS operations of one wave execute in order).  The row then goes out with consecutive lanes on
// consecutive elements - an env's A * G elements are contiguous in both forms - and lanes a < A write recipe_done and task, lane 0
// t.  A recipe id outside the table (no record the library let in has one in a used slot) reads as a recipe without nodes.  Plain
// stores; every element of a written row exactly once; the records are only read.
constexpr int INFOS_WAVES = 4, GOAL_ROW_NODES = 16, INFOS_ROW_BYTES = 1024;       // (4 agents x at most 255 goals)
struct InfosArgs {
    const uint32_t *state;             // [N][RW]
    const uint32_t *recipes;           // the recipe table of the step kernels (cz_load_recipes)
    const uint8_t *goal_ids;           // [n_recipes][GOAL_ROW_NODES] (cz_load_goal_table)
    int64_t env_begin;
    int32_t count, RW, A, G, n_recipes;
    uint8_t *goal8;                    // [count][A][G]
    float *goal32;                     // [count][A][G]
    uint8_t *done;                     // [count][A]
    int32_t *task;                     // [count][A]
    int32_t *t;                        // [count]; any of the five may be null
};
template <bool WIDE>
__global__ __launch_bounds__(64 * INFOS_WAVES) void k_infos(const InfosArgs G) {
    __shared__ uint8_t rows[INFOS_WAVES][INFOS_ROW_BYTES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t i = (int64_t)blockIdx.x * INFOS_WAVES + wave;
    if (i >= G.count) return;
    constexpr uint32_t ROW_WORDS = WIDE ? 1u + 2u * WIDE_NODES : 1u + MAX_NODES;
    const uint32_t *rec = G.state + (size_t)(G.env_begin + i) * G.RW;
    const uint32_t t = rfl(rec[W_T]), m_lo = rfl(rec[W_MARKS]), m_hi = WIDE ? rfl(rec[W_MARKS_HI]) : 0u, ids = rfl(rec[W_RECIPES]);
    const uint32_t A = (uint32_t)G.A, NG = (uint32_t)G.G, row_len = A * NG;
    uint8_t *row = rows[wave];
    const auto marks_of = [&](uint32_t a) {
        return WIDE ? ((a < 2u ? m_lo : m_hi) >> (16u * (a & 1u))) & 0xFFFFu : (m_lo >> (8u * a)) & 0xFFu;
    };
    for (uint32_t k = lane; k < row_len; k += 64u) row[k] = 0;
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    {
        const uint32_t a = lane >> 4, j = lane & 15u, r = (ids >> (8u * a)) & 0xFFu;
        if (a < A && r < (uint32_t)G.n_recipes && (WIDE || j < (uint32_t)MAX_NODES)) {     // (before r or j is an index)
            const uint32_t *rr = G.recipes + (size_t)r * ROW_WORDS;
            const uint32_t nn = rr[0] & 0xFFu, w = rr[WIDE ? 1u + 2u * j : 1u + j], id = G.goal_ids[r * GOAL_ROW_NODES + j];
            if (j < nn && ((w >> 8) & 1u) && id < NG) row[a * NG + id] = (uint8_t)(((marks_of(a) >> j) & 1u) ^ 1u);
        }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const size_t out0 = (size_t)i * row_len;
    for (uint32_t k = lane; k < row_len; k += 64u) {
        const uint32_t v = row[k];
        if (G.goal8) G.goal8[out0 + k] = (uint8_t)v;
        if (G.goal32) G.goal32[out0 + k] = (float)v;
    }
    if (lane < A) {
        if (G.done) G.done[(size_t)i * A + lane] = (uint8_t)(marks_of(lane) & 1u);
        if (G.task) G.task[(size_t)i * A + lane] = (int32_t)((ids >> (8u * lane)) & 0xFFu);
    }
    if (lane == 0u && G.t) G.t[i] = (int32_t)t;
}

// ---- the MLP policy as a launch of its own (cz_policy_device; definition: cooking_zoo_amd/policy.py, device function: cz_policy.h).
// Reads the caller's float32 rows and the weight table and nothing of the records.
struct PolicyArgs {
    int64_t env_global0;           // the global id of the first env (the sampling draw is keyed by it)
    const float *obs32;            // [count][A][F]
    const float *table;            // the packed weight sets (k_policy_pack)
    int32_t F, C;
    uint32_t packed;               // policy_pack_sets: every agent's set and the mode
    uint32_t step;
    uint64_t seed;
    int32_t *actions;              // [count][A] or null
    float *logits;                 // [count][A][C] or null
};
// One wavefront per env: the env's rows go to LDS (zero behind F), then policy_hidden and policy_heads per agent with a weight set; the entries of the
// other agents are left as they are in both outputs.
template <int NA>
__global__ __launch_bounds__(64) void k_policy(const PolicyArgs G) {
    const int lane = (int)threadIdx.x;
    const size_t i = blockIdx.x;
    const int Fq = policy_quads(G.F);
    float *const x = reinterpret_cast<float *>(policy_rows);
    const float *const src = G.obs32 + i * (size_t)(NA * G.F);
#pragma unroll
    for (int a = 0; a < NA; ++a)
        for (int f = lane; f < 4 * Fq; f += 64) x[a * 4 * Fq + f] = f < G.F ? src[(size_t)a * G.F + f] : 0.0f;
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const uint32_t si = (G.packed >> (3 * a)) & 7u;
        if (si == 7u) continue;
        int action;
        float mylogit;
        const float *const set = G.table + (size_t)si * policy_set_floats(G.F);
        const uint32_t mode = (G.packed >> POLICY_VSETS_BITS) & 1u;
        const float hid = policy_hidden(set, Fq, x + a * 4 * Fq, lane);
        if (G.C == 5) policy_heads<5>(set, Fq, hid, lane, mode, G.seed, G.env_global0 + (int64_t)i, G.step, a, action, mylogit);
        else policy_heads<8>(set, Fq, hid, lane, mode, G.seed, G.env_global0 + (int64_t)i, G.step, a, action, mylogit);
        if (G.actions && lane == 0) G.actions[i * NA + a] = action;
        if (G.logits && lane < G.C) G.logits[(i * NA + a) * (size_t)G.C + lane] = mylogit;
    }
}

// ---- the value head as a launch of its own (cz_value_device; definition: policy.py step 3b).  Rows of the caller, no record read.
struct ValueArgs {
    const float *obs32;            // [rows][A][F]
    const float *table;            // the packed weight sets with the value heads behind them
    int32_t F;
    uint32_t vpacked;              // policy_pack_vsets: every agent's value set
    float *values;                 // [rows][A]
};
// One wavefront per [A][F]-row, in the shape of k_policy: the rows go to LDS (zero behind F), then policy_hidden and policy_value per
// agent with a value set; the entries of the other agents are left as they are.
template <int NA>
__global__ __launch_bounds__(64) void k_value(const ValueArgs G) {
    const int lane = (int)threadIdx.x;
    const size_t i = blockIdx.x;
    const int Fq = policy_quads(G.F);
    float *const x = reinterpret_cast<float *>(policy_rows);
    const float *const src = G.obs32 + i * (size_t)(NA * G.F);
#pragma unroll
    for (int a = 0; a < NA; ++a)
        for (int f = lane; f < 4 * Fq; f += 64) x[a * 4 * Fq + f] = f < G.F ? src[(size_t)a * G.F + f] : 0.0f;
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const uint32_t vi = (G.vpacked >> (3 * a)) & 7u;
        if (vi == 7u) continue;
        const float hid = policy_hidden(G.table + (size_t)vi * policy_set_floats(G.F), Fq, x + a * 4 * Fq, lane);
        const float v = policy_value(G.table, G.F, vi, hid, lane);
        if (lane == 0) G.values[i * NA + a] = v;
    }
}
// torch's layouts - wv [n][64], bv [n][1] - into the value heads behind the sets (cz_policy.h): one thread per float of them; heads
// past n_sets are zeroed
template <int UNUSED = 0>
__global__ __launch_bounds__(320) void k_value_pack(float *__restrict__ heads, int32_t n_sets, const float *__restrict__ wv,
                                                                    const float *__restrict__ bv) {
    const uint32_t idx = threadIdx.x, wv_end = POLICY_MAX_SETS * POLICY_HIDDEN;
    if (idx >= POLICY_VALUE_FLOATS) return;
    float v = 0.0f;
    if (idx < wv_end) { if ((idx >> 6) < (uint32_t)n_sets) v = wv[idx]; }
    else if (idx - wv_end < (uint32_t)n_sets) v = bv[idx - wv_end];
    heads[idx] = v;
}
// torch's layouts - W1 [n][64][F], b1 [n][64], W2 [n][C][64], b2 [n][C] - into the table's (cz_policy.h): one thread per float of it
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_policy_pack(float *__restrict__ table, int32_t n_sets, int32_t F, int32_t C, const float *__restrict__ w1,
                                                     const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2) {
    const uint32_t per_set = policy_set_floats(F), idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= per_set * (uint32_t)n_sets) return;
    const uint32_t s = idx / per_set, o = idx - s * per_set, w1_end = (uint32_t)policy_quads(F) * 256u;
    float v = 0.0f;
    if (o < w1_end) {
        const uint32_t q = o >> 8, j = (o >> 2) & 63u, f = 4u * q + (o & 3u);
        if (f < (uint32_t)F) v = w1[((size_t)s * POLICY_HIDDEN + j) * (size_t)F + f];
    } else if (o < w1_end + POLICY_HIDDEN) {
        v = b1[s * POLICY_HIDDEN + (o - w1_end)];
    } else if (o < w1_end + POLICY_HIDDEN + POLICY_MAX_ACTIONS * POLICY_HIDDEN) {
        const uint32_t r = o - w1_end - POLICY_HIDDEN, c = r >> 6;
        if (c < (uint32_t)C) v = w2[((size_t)s * C + c) * POLICY_HIDDEN + (r & 63u)];
    } else {
        const uint32_t c = o - w1_end - POLICY_HIDDEN - POLICY_MAX_ACTIONS * POLICY_HIDDEN;
        if (c < (uint32_t)C) v = b2[s * C + c];
    }
    table[idx] = v;
}

// ---- what a learner trains on (cz_gae_device, cz_logprob_device; definition: cooking_zoo_amd/targets.py).  Neither kernel reads a
// record: both work on the caller's dense arrays alone.
struct GaeArgs {
    int64_t n;                     // series: env_count * A; row t of every array is n contiguous elements
    int32_t T, A;
    uint32_t agents;               // bit a: agent a's series are computed; the others are neither read nor written
    const double *rewards;         // [T][n]
    const uint8_t *term, *trunc;   // [T][n]; trunc may be null
    const float *values;           // [T + 1][n]
    double gamma, gl;              // gl = gamma * lambda, rounded once by the host
    float *adv, *ret;              // [T][n]; one of them may be null
};
// One thread per series, t descending: the recurrence is serial, but no load depends on it, so the rows are loaded a block of D ahead
// of the block the chain is working on - two register blocks, the loads of the next one issued before the first use of this one.
// Rows below 0 of the last block are loaded from row 0 (in bounds, never used) so that every block's loads are one straight run.
// Without truncations the terminations stand in for them (the same byte twice): no branch between the loads.
// The library carries D in {2, 4, 8, 16} x WG in {64, 256}; a launch takes GAE_DEPTH x GAE_BLOCK unless CZ_GAE_SHAPE names another.
constexpr int GAE_DEPTH = 8, GAE_BLOCK = 64;
template <int D, int WG>
__global__ __launch_bounds__(WG) void k_gae(const GaeArgs G) {
    const size_t i = (size_t)blockIdx.x * WG + threadIdx.x, n = (size_t)G.n;
    if (i >= n || !((G.agents >> (uint32_t)(i % (size_t)G.A)) & 1u)) return;
    struct Rows { double r[D]; float v[D]; uint32_t done[D]; };
    const uint8_t *const trunc = G.trunc ? G.trunc : G.term;
    auto load = [&](int top, Rows &b) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const int t = top - k;
            const size_t o = (size_t)(t < 0 ? 0 : t) * n + i;
            b.r[k] = G.rewards[o];
            b.v[k] = G.values[o];
            b.done[k] = (uint32_t)G.term[o] | (uint32_t)trunc[o];
        }
    };
    Rows cur, nxt;
    load(G.T - 1, cur);
    double vnext = (double)G.values[(size_t)G.T * n + i], A = 0.0;
    for (int top = G.T - 1; top >= 0; top -= D) {
        load(top - D, nxt);
        double v[D], d[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {                              // off the chain: the TD errors of the block
            v[k] = (double)cur.v[k];
            d[k] = (cur.r[k] + (cur.done[k] ? 0.0 : G.gamma * (k == 0 ? vnext : v[k - 1]))) - v[k];
        }
        vnext = v[D - 1];
        if (top >= D - 1) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                A = d[k] + (cur.done[k] ? 0.0 : G.gl * A);
                const size_t o = (size_t)(top - k) * n + i;
                if (G.adv) G.adv[o] = (float)A;
                if (G.ret) G.ret[o] = (float)(A + v[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                if (k > top) continue;
                A = d[k] + (cur.done[k] ? 0.0 : G.gl * A);
                const size_t o = (size_t)(top - k) * n + i;
                if (G.adv) G.adv[o] = (float)A;
                if (G.ret) G.ret[o] = (float)(A + v[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) { cur.r[k] = nxt.r[k]; cur.v[k] = nxt.v[k]; cur.done[k] = nxt.done[k]; }      // (element by element: registers)
    }
}

struct LogprobArgs {
    int64_t total;                 // rows * A
    int32_t A;
    uint32_t sets;                 // agent a's byte 0xFF: its entries are left untouched in both outputs
    const float *logits;           // [rows][A][C]
    const int32_t *actions;        // [rows][A]
    float *logp, *entropy;         // [rows][A]; one of them may be null
};
// One thread per (row, agent): the C logits, policy_logprob (cz_policy.h) in float64, two float32 stores.
template <int C>
__global__ __launch_bounds__(256) void k_logprob(const LogprobArgs G) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)G.total) return;
    const uint32_t a = (uint32_t)(i % (size_t)G.A);
    if (((G.sets >> (8u * a)) & 0xFFu) == POLICY_NONE) return;
    float logit[C];
#pragma unroll
    for (int c = 0; c < C; ++c) logit[c] = G.logits[i * C + c];
    double logp, entropy;
    policy_logprob<C>(logit, G.actions[i], logp, entropy);
    if (G.logp) G.logp[i] = (float)logp;
    if (G.entropy) G.entropy[i] = (float)entropy;
}

// ---- PPO's gradients (cz_ppo_grad_device; definition: cooking_zoo_amd/ppo.py, device functions: cz_policy.h).  Three launches share
// one argument block.  Every (position, agent) owns two pass slots - 0: the pass into its policy set, 1: the pass into its value set
// where that is a pass of its own - and k_ppo_forward writes both slots of every (position, agent) on every call, so nothing of the
// workspace is ever read that this call did not write.
constexpr int PPO_SMALL = 12;                // a slot's scalars as 32-bit words: the float bits of g [8] and gv, the set (int32, -1: no pass), row * A + agent, 0
constexpr int PPO_TILE = 32;                 // features per workgroup of k_ppo_outer, one accumulator register each.  The library carries 16, 32
                                             // and 64 (CZ_PPO_TILE picks another, for tools/ppo_sizes.py); what each measures: profiles/r35/README.md
// one set's floats in a partial: dW1 as [F][64] (lane j's stores coalesced), db1 [64], dW2 [8][64], db2 [8], dwv [64], dbv
__host__ __device__ inline uint32_t ppo_set_floats(int F) {
    return (uint32_t)F * POLICY_HIDDEN + POLICY_HIDDEN + POLICY_MAX_ACTIONS * POLICY_HIDDEN + POLICY_MAX_ACTIONS + POLICY_HIDDEN + 1u;
}
struct PpoArgs {
    int64_t rows;                  // R: rows of the trajectory
    int32_t positions;             // M: the minibatch
    int32_t A, F, C, n_sets;       // n_sets: the loaded sets, the leading axis of every gradient
    uint32_t packed, vpacked;      // policy_pack_sets / policy_pack_vsets
    uint32_t used;                 // bit k: some agent's policy or value set is k
    const int32_t *index;          // [M] or null
    const float *obs32;            // [R][A][F]
    const int32_t *actions;        // [R][A]
    const float *logp_old, *adv, *ret;
    const float *table;
    PpoScales K;
    // the workspace (cz_ppo_reserve)
    double *terms;                 // [M * A][PPO_TERMS]
    double *chunk_stats;           // [chunks][PPO_TERMS]
    float *hid, *da;               // [slot][64]
    uint32_t *small;               // [slot][PPO_SMALL]
    float *partial;                // [chunk][n_sets][ppo_set_floats]
    // the outputs, torch's layouts behind a leading axis of n_sets
    float *gw1, *gb1, *gw2, *gb2, *gwv, *gbv;      // gwv / gbv may be null
    double *stats;                 // [8] or null
};
// element `i` of a register array, i wave-varying
template <class T, int N>
__device__ __forceinline__ T ppo_pick(const T (&v)[N], int i) {
    T out = v[0];
#pragma unroll
    for (int k = 1; k < N; ++k) out = i == k ? v[k] : out;
    return out;
}
// One wavefront per (position, agent), the shape of k_value: the row goes to LDS, then policy_hidden, the logits and the value exactly
// as the rollout computes them, the gradient with respect to the logits and the value in float64 (every lane computes all of it: the
// wave's time is one lane's), and dh_j / da_j on lane j.  Writes the two slots and the statistics' terms.
template <int C>
__global__ __launch_bounds__(64) void k_ppo_forward(const PpoArgs G) {
    const int lane = (int)threadIdx.x;
    const uint32_t e = blockIdx.x, A = (uint32_t)G.A;
    const uint32_t m = e / A, a = e - m * A;
    const int64_t r = G.index ? (int64_t)G.index[m] : (int64_t)m;
    const bool inside = r >= 0 && r < G.rows;
    const uint32_t s = (G.packed >> (3u * a)) & 7u, vs = (G.vpacked >> (3u * a)) & 7u;
    const int Fq = policy_quads(G.F);
    double term[PPO_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    term[7] = !inside && a == 0u ? 1.0 : 0.0;
    float g[POLICY_MAX_ACTIONS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float gv = 0.0f, h = 0.0f, hv = 0.0f, da0 = 0.0f, da1 = 0.0f;
    int set0 = -1, set1 = -1;
    bool both = false;
    const size_t ra = inside ? (size_t)r * A + a : 0u;
    if (inside && (s != 7u || vs != 7u)) {
        float *const x = reinterpret_cast<float *>(policy_rows);
        const float *const src = G.obs32 + ra * (size_t)G.F;
        for (int f = lane; f < 4 * Fq; f += 64) x[f] = f < G.F ? src[f] : 0.0f;
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const size_t per_set = policy_set_floats(G.F);
        const float *const heads = G.table + policy_value_offset(G.F);
        bool has_p = false, has_v = false;
        if (s != 7u) {
            const float *const set = G.table + (size_t)s * per_set;
            h = policy_hidden(set, Fq, x, lane);
            const int act = G.actions[ra];
            if ((unsigned)act < (unsigned)C) {
                has_p = true;
                float logit[C], gc[C];
                policy_all_logits<C>(set, Fq, h, lane, logit);
                policy_ppo_logit_grad<C>(logit, act, (double)G.logp_old[ra], (double)G.adv[ra], G.K, gc, term);
#pragma unroll
                for (int c = 0; c < C; ++c) g[c] = gc[c];
                term[5] = 1.0;
            }
        }
        if (vs != 7u) {
            hv = vs == s ? h : policy_hidden(G.table + (size_t)vs * per_set, Fq, x, lane);
            const double dv = (double)policy_value(G.table, G.F, vs, hv, lane) - (double)G.ret[ra];
            gv = (float)(G.K.inv_v * (G.K.c_value * dv));
            term[1] = 0.5 * (dv * dv);
            term[6] = 1.0;
            has_v = true;
        }
        both = has_p && has_v && s == vs;
        if (has_p) {
            const float *const w2 = G.table + (size_t)s * per_set + (uint32_t)Fq * 256u + POLICY_HIDDEN;
            float dh = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) dh = __builtin_fmaf(g[c], w2[c * POLICY_HIDDEN + lane], dh);
            if (both) dh = __builtin_fmaf(gv, heads[s * POLICY_HIDDEN + (uint32_t)lane], dh);
            da0 = h > 0.0f ? dh : 0.0f;
            set0 = (int)s;
        }
        if (has_v && !both) {
            const float dh = __builtin_fmaf(gv, heads[vs * POLICY_HIDDEN + (uint32_t)lane], 0.0f);
            da1 = hv > 0.0f ? dh : 0.0f;
            set1 = (int)vs;
        }
    }
    const size_t slot0 = (size_t)e * 2u, slot1 = slot0 + 1u;
    if (set0 >= 0) { G.hid[slot0 * 64u + lane] = h; G.da[slot0 * 64u + lane] = da0; }
    if (set1 >= 0) { G.hid[slot1 * 64u + lane] = hv; G.da[slot1 * 64u + lane] = da1; }
    if (lane < PPO_SMALL) {
        const uint32_t gl = __builtin_bit_cast(uint32_t, ppo_pick(g, lane)), gvb = __builtin_bit_cast(uint32_t, gv), rab = (uint32_t)ra;
        // slot 0 carries g, and gv where the value part rides on the same pass; slot 1 carries gv alone (0u is +0.0f)
        G.small[slot0 * PPO_SMALL + lane] = lane < 8 ? (set0 >= 0 ? gl : 0u) : lane == 8 ? (both ? gvb : 0u)
                                            : lane == 9 ? (uint32_t)set0 : lane == 10 ? rab : 0u;
        G.small[slot1 * PPO_SMALL + lane] = lane < 8 ? 0u : lane == 8 ? (set1 >= 0 ? gvb : 0u)
                                            : lane == 9 ? (uint32_t)set1 : lane == 10 ? rab : 0u;
    }
    if (lane < PPO_TERMS) G.terms[(size_t)e * PPO_TERMS + lane] = ppo_pick(term, lane);
}
// Grid (chunk, feature tile, set), one wavefront, lane = hidden unit j.  Walks the chunk's slots in order and takes the passes into
// its set: da_j from a coalesced load, the row's TILE features at a wave-uniform address, one fmaf per accumulator register.  Tile
// 0 also accumulates dW2, db2, dwv, dbv and db1, and tile 0 of set 0 sums the chunk's statistics' terms, lane e < 8 entry e.
template <int TILE>
__global__ __launch_bounds__(64) void k_ppo_outer(const PpoArgs G) {
    const int lane = (int)threadIdx.x;
    const uint32_t chunk = blockIdx.x, tile = blockIdx.y, k = blockIdx.z, A = (uint32_t)G.A, F = (uint32_t)G.F;
    const uint32_t m0 = chunk * PPO_CHUNK, left = (uint32_t)G.positions - m0, count = left < (uint32_t)PPO_CHUNK ? left : (uint32_t)PPO_CHUNK;
    if ((G.used >> k) & 1u) {
        const uint32_t f0 = tile * TILE, nt = F - f0 < (uint32_t)TILE ? F - f0 : (uint32_t)TILE;
        float acc[TILE], aw2[POLICY_MAX_ACTIONS], ab2[POLICY_MAX_ACTIONS], awv = 0.0f, abv = 0.0f, ab1 = 0.0f;
#pragma unroll
        for (int t = 0; t < TILE; ++t) acc[t] = 0.0f;
#pragma unroll
        for (int c = 0; c < POLICY_MAX_ACTIONS; ++c) aw2[c] = ab2[c] = 0.0f;
        const size_t slot_begin = (size_t)m0 * A * 2u, slot_end = slot_begin + (size_t)count * A * 2u;
        for (size_t slot = slot_begin; slot < slot_end; ++slot) {
            const uint32_t *const sm = G.small + slot * PPO_SMALL;
            if (sm[9] != k) continue;
            const float da = G.da[slot * 64u + lane];
            const float *const x = G.obs32 + (size_t)sm[10] * F + f0;
            if (nt == (uint32_t)TILE) {
#pragma unroll
                for (int t = 0; t < TILE; ++t) acc[t] = __builtin_fmaf(da, x[t], acc[t]);
            } else {
#pragma unroll
                for (int t = 0; t < TILE; ++t)
                    if ((uint32_t)t < nt) acc[t] = __builtin_fmaf(da, x[t], acc[t]);
            }
            if (tile == 0u) {
                const float h = G.hid[slot * 64u + lane], gv = __builtin_bit_cast(float, sm[8]);
#pragma unroll
                for (int c = 0; c < POLICY_MAX_ACTIONS; ++c) {
                    const float gc = __builtin_bit_cast(float, sm[c]);
                    aw2[c] = __builtin_fmaf(gc, h, aw2[c]);
                    ab2[c] = ab2[c] + gc;
                }
                awv = __builtin_fmaf(gv, h, awv);
                abv = abv + gv;
                ab1 = ab1 + da;
            }
        }
        float *const P = G.partial + ((size_t)chunk * (uint32_t)G.n_sets + k) * ppo_set_floats(G.F);
#pragma unroll
        for (int t = 0; t < TILE; ++t)
            if ((uint32_t)t < nt) P[(size_t)(f0 + t) * 64u + lane] = acc[t];
        if (tile == 0u) {
            float *const rest = P + (size_t)F * 64u;
            rest[lane] = ab1;
#pragma unroll
            for (int c = 0; c < POLICY_MAX_ACTIONS; ++c) rest[64 + c * 64 + lane] = aw2[c];
            if (lane < POLICY_MAX_ACTIONS) rest[64 + 512 + lane] = ppo_pick(ab2, lane);
            rest[64 + 512 + 8 + lane] = awv;
            if (lane == 0) rest[64 + 512 + 8 + 64] = abv;
        }
    }
    if (tile == 0u && k == 0u && lane < PPO_TERMS) {
        const double *const t = G.terms + (size_t)m0 * A * PPO_TERMS + lane;
        double acc = 0.0;
        for (uint32_t i = 0; i < count * A; ++i) acc = acc + t[(size_t)i * PPO_TERMS];
        G.chunk_stats[(size_t)chunk * PPO_TERMS + lane] = acc;
    }
}
// One thread per float of the partials' per-set layout (coalesced reads, chunk after chunk), summed in ascending chunk order and
// written where torch keeps it; sets nobody used get zeros.  Eight more threads finish the statistics.
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_ppo_reduce(const PpoArgs G) {
    const uint32_t PS = ppo_set_floats(G.F), total = PS * (uint32_t)G.n_sets, idx = blockIdx.x * 256u + threadIdx.x;
    const uint32_t chunks = ((uint32_t)G.positions + PPO_CHUNK - 1u) / PPO_CHUNK, F = (uint32_t)G.F, C = (uint32_t)G.C;
    if (idx < total) {
        const uint32_t k = idx / PS, o = idx - k * PS;
        float v = 0.0f;
        if ((G.used >> k) & 1u) {
            const float *const p = G.partial + (size_t)k * PS + o;
            const size_t stride = (size_t)PS * (uint32_t)G.n_sets;
            v = p[0];
#pragma unroll 8
            for (uint32_t ch = 1; ch < chunks; ++ch) v = v + p[ch * stride];
        }
        const uint32_t w1_end = F * 64u, b1_end = w1_end + 64u, w2_end = b1_end + 512u, b2_end = w2_end + 8u, wv_end = b2_end + 64u;
        if (o < w1_end) G.gw1[((size_t)k * 64u + (o & 63u)) * F + (o >> 6)] = v;
        else if (o < b1_end) G.gb1[k * 64u + (o - w1_end)] = v;
        else if (o < w2_end) { const uint32_t q = o - b1_end, c = q >> 6; if (c < C) G.gw2[((size_t)k * C + c) * 64u + (q & 63u)] = v; }
        else if (o < b2_end) { const uint32_t c = o - w2_end; if (c < C) G.gb2[k * C + c] = v; }
        else if (o < wv_end) { if (G.gwv) G.gwv[k * 64u + (o - b2_end)] = v; }
        else if (G.gbv) G.gbv[k] = v;
    } else if (idx < total + PPO_TERMS && G.stats) {
        const uint32_t e = idx - total;
        double v = G.chunk_stats[e];
#pragma unroll 8
        for (uint32_t ch = 1; ch < chunks; ++ch) v = v + G.chunk_stats[(size_t)ch * PPO_TERMS + e];
        G.stats[e] = e == 1u ? G.K.inv_v * v : e == 0u || (e >= 2u && e <= 4u) ? G.K.inv_p * v : v;
    }
}

}  // namespace cz

#include "cz_adam.h"
