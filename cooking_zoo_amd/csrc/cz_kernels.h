// cz_kernels.h -- kernel templates of the step path (included by the per-size instantiation units).
#pragma once
#include "cz_device.h"
#include <type_traits>

namespace cz {

// Diagnostic build only (make prof -> libcookingzoo_hip_prof.so, -DCZ_PROFILE): s_memrealtime stamps (100 MHz, one clock for
// the whole device, so that first start / last end of a launch can be read across XCDs) at phase boundaries,
// written to a buffer of their own (Params::stamps, 16 slots per env: 0..7 the phases, 8..10 inside the reward phase); the
// shipped library contains none of this.
#ifdef CZ_PROFILE
#define CZ_STAMP(i)                                                                                    \
    do {                                                                                               \
        unsigned long long _t;                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                 \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        if (lane == 0 && P.stamps) P.stamps[(size_t)env * 16 + (i)] = _t;                               \
    } while (0)
#elif defined(CZ_MARKERS)
// marker build (tools/phase_cut.py, never loaded): an assembler comment at every phase boundary and no instruction - if the
// instruction stream equals the shipped one (tools/isa_diff.py), the comments are positions in the shipped code
#define CZ_STAMP(i) asm volatile("; CZ_MARK " #i)
#else
#define CZ_STAMP(i) do { } while (0)
#endif

// Parameters that are needed late (output pointers, statistics, the reward constants of the rare "a recipe node changed"
// path, the layout pool of the reset path) are read from the argument segment where they are used, through a pointer the
// optimiser cannot see through -- otherwise every one of them is fetched at kernel entry and held in SGPRs for the whole
// kernel (~30 SGPRs: spills in the non-fused kernel, ~90 spilled SGPRs in the fused one).
typedef const __attribute__((address_space(4))) Params *KParams;
struct StepArgsMirror { uint32_t *a; const int32_t *b; const double *c; int32_t i[8]; Params p; };   // k_step's argument list (7 ints + one of padding)
struct LeanArgsMirror { uint32_t *a; const int32_t *b; const double *c; int32_t i[8]; LeanParams p; };   // ... and k_step_lean's / k_step_lean_cfg's
static_assert(offsetof(LeanArgsMirror, p) == LEADING_SCALAR_BYTES && offsetof(StepArgsMirror, p) == LEADING_SCALAR_BYTES, "leading scalars");
template <class B> constexpr unsigned block_offset() {
    return std::is_same<B, LeanParams>::value ? (unsigned)offsetof(LeanArgsMirror, p) : (unsigned)offsetof(StepArgsMirror, p);
}
// (B: the block of the kernel that asks - Params or LeanParams)
template <class B = Params>
__device__ __forceinline__ const __attribute__((address_space(4))) B *late_params(unsigned offset) {
    const __attribute__((address_space(4))) char *k =
        (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));                      // loads through the result stay behind this point
    return reinterpret_cast<const __attribute__((address_space(4))) B *>(k + offset);
}
#define CZ_LATE_STEP() late_params<typename V::Block>(block_offset<typename V::Block>())

// The variants of the step kernel: cz::k_step<OPL, CPL, NA, SCHEME, mode> and, for STEP only, cz::k_step_lean<OPL, CPL, NA, SCHEME>.
// (choose_step in cz_api.hip says which launch gets which; DESIGN.md section 4 has the same table.)
enum StepMode : int {
    STEP = 0,                 // one step, actions from memory
    ROLLOUT = 1,              // P.T steps, on-device action stream, outputs [t][env] (cz_rollout)
    ROLLOUT_ACTIONS = 2,      // P.T steps over the caller's actions [t][env][agent] (cz_rollout_actions, fused rings; its own instance so that the
                              // on-device stream's loop carries none of it: as a run-time branch it cost the random-action rollout 4 %)
    STEP_CODES = 3,           // one step that also (or only) writes the compact observation (cz_step_device_compact / cz_set_compact_output;
                              // its own instance as well: compiled into the ordinary one-step kernel the path cost every launch 0.2 us, register
                              // allocation and a longer prologue, even when unused)
    ROLLOUT_CODES = 4,        // P.T steps over the on-device action stream with a compact trajectory [t][env][agent][pitch] (cz_rollout_compact)
    ROLLOUT_CODES_ONLY = 5,   // the same without a float64 trajectory beside it
    STEP_F32 = 6,             // one step that writes the observation as dense float32 rows float[N][A][F] (cz_step_device_f32 / cz_set_f32_output)
                              // and nothing else: its own instance for the reason STEP_CODES is one
    ROLLOUT_F32 = 7,          // P.T steps over the on-device action stream with a float32 trajectory float[T][N][A][F] and no other form of
                              // the observation (cz_rollout_f32)
    ROLLOUT_ACTIONS_F32 = 8,  // the same over the caller's actions [t][env][agent] (cz_rollout_actions_f32): its own instance for the reason
                              // ROLLOUT_ACTIONS is one; always writes row t (the in-place form of fused ring runs is not offered in float32)
};
template <int MODE, bool LEAN = false>
struct StepTraits {
    static_assert(MODE >= STEP && MODE <= ROLLOUT_ACTIONS_F32 && (!LEAN || MODE == STEP), "no such variant");
    static constexpr bool fused = MODE == ROLLOUT || MODE == ROLLOUT_ACTIONS || MODE == ROLLOUT_CODES || MODE == ROLLOUT_CODES_ONLY ||
                                  MODE == ROLLOUT_F32 || MODE == ROLLOUT_ACTIONS_F32;   // P.T steps per launch
    static constexpr bool ext_actions = MODE == ROLLOUT_ACTIONS || MODE == ROLLOUT_ACTIONS_F32;   // a fused launch that reads the caller's actions
    static constexpr bool codes = MODE == STEP_CODES || MODE == ROLLOUT_CODES || MODE == ROLLOUT_CODES_ONLY;   // writes the compact observation
    // a fused rollout that writes codes ONLY (cz_rollout_compact without a float64 trajectory).  Without the float64 path - its six
    // descriptor registers, its encode - the codes' own descriptor words fit the registers for the whole launch (ROLLOUT_CODES reloads
    // them every step: held there they cost 136 vector registers, three waves per SIMD)
    static constexpr bool codes_only = MODE == ROLLOUT_CODES_ONLY;
    // the float32 rows: np.float32 of the float64 feature (round to nearest even), gathered from a float32 copy of the table that the
    // workgroup makes while it stages the table into LDS - no arithmetic on values, no float64 path beside it
    static constexpr bool f32 = MODE == STEP_F32 || MODE == ROLLOUT_F32 || MODE == ROLLOUT_ACTIONS_F32;
    static constexpr bool f64 = !codes_only && !f32;                                     // carries the float64 observation path
    // The CodesPrefetch words (the b128 descriptor loads of the codes and of the float32 rows): fetched once behind the prologue and held
    // in registers - a fused launch fetches them again only when a reset pass has moved the env to another layout - or, desc_per_step,
    // fetched at the top of every fused step.  The float32 rollouts hold them: held, no instance loses a wave per SIMD against
    // ROLLOUT_CODES_ONLY (profiles/r14/README.md has the register counts of both forms; CZ_ROLLOUT_F32_HOLD=0 builds the other one).
#ifndef CZ_ROLLOUT_F32_HOLD
#define CZ_ROLLOUT_F32_HOLD 1
#endif
    static constexpr bool desc_held = (codes || f32) && (!fused || codes_only || (f32 && CZ_ROLLOUT_F32_HOLD != 0));
    static constexpr bool desc_per_step = (codes || f32) && fused && !desc_held;
    // k_step_lean: the one-step kernel with the handle's uniform settings fixed at compile time - narrow recipe tables, no despawn /
    // respawn, float64 observations of at most 128 * OBS_PAIRS features with write-through stores, no compact output and no marks
    // buffer (choose_step in cz_api.hip picks it when all of that holds).  The code is the one-step kernel with those tests folded
    // away: same results, fewer scalar instructions and registers per wave.
    static constexpr bool lean = LEAN;
    // the argument block of the kernel, and what its device functions read it through (LeanView: the block plus the leading scalars)
    using Block = std::conditional_t<LEAN, LeanParams, Params>;
    using View = std::conditional_t<LEAN, LeanView, Params>;
};
// k_step_lean_cfg: the lean kernel with the handle's recipe count, end condition and walk_touches fixed too (LeanViewFixed)
template <int R, int END_ALL, int WALK_TOUCHES>
struct LeanCfgTraits : StepTraits<STEP, true> {
    using View = LeanViewFixed<R, END_ALL, WALK_TOUCHES>;
};
// (The pieces below the kernel - load_env, all_marks, observe, step_env - are templates over the one or two properties they ask
// for, fed from the traits by step_kernel: k_reset / k_observe and several variants then share one instance of each, as they always
// have, and the optimiser's view of a piece - hence the shipped instruction streams - depends on who shares it.)

// LDS image of one env (halfwords, cooking_zoo_amd/soa.py IMG_*): every halfword is a BYTE offset into `lut`
// Two layouts: up to 128 slots / 256 cells (CPL <= 4), and the "huge" one for up to 256 slots / 1024 cells (CPL = 16).
template <int CPL>
struct Img {
    static constexpr bool HUGE = CPL > 4;
    static constexpr int OBJ0 = 0, CELL0 = HUGE ? 1536 : 768, AG0 = CELL0 + (HUGE ? 4096 : 1024), ZERO = AG0 + 32, HALFWORDS = ZERO + 8;
};
constexpr int LUT_ABSENT = 255, LUT_SIZE = 256;
#ifndef CZ_ENVS_PER_WG
#define CZ_ENVS_PER_WG 8
#endif
constexpr int ENVS_PER_WG = CZ_ENVS_PER_WG;   // one wavefront per env, this many per workgroup (no cross-wave communication)
// the huge instance keeps 13.6 KB of LDS per env: four of them (the minimum that still stages the 256-entry table with one
// entry per thread) fit the 64 KB a workgroup may declare
template <int CPL> constexpr int envs_per_wg() { return CPL > 4 ? 4 : ENVS_PER_WG; }
constexpr int OBS_PAIRS = 3;       // feature pairs per lane and chunk: 3 x 128 = 384 features per chunk
constexpr int OBS_CHUNK = 2 * OBS_PAIRS;   // descriptor words held per lane

// (the quotient table `lut` itself is shared by the waves of a workgroup: [0..2W-2] (i-(W-1))/W | [63..63+2H-2] (i-(H-1))/H |
// [126] 0.0 | [127] 1.0 | [128..255] 0.0)
template <int CPL>
struct Lds {
    int32_t sub[MAX_AGENTS][16];         // per observer: what to subtract (x8) for each axis code (first: two of its rows are read
                                         // with one ds_read2_b32, whose offsets reach 1 KB)
    uint16_t img[Img<CPL>::HALFWORDS];   // objects 6 hw each | cells 4 hw each | agents 8 hw each | the "absent" halfword
    // recipe evaluation scratch: node bits per cell, per object kind and per cell type (recipe_marks_cells; instances with up
    // to 4 cells per lane) or matched-location bit sets per node, CPL words each (recipe_marks of the 32x32 instance,
    // recipe_marks_wide)
    uint64_t locs[CPL <= 4 ? 64 * CPL + 8 : WIDE_NODES * CPL];
};

// Memory access helpers: a wave-uniform base pointer plus a 32-bit unsigned per-lane byte offset, which the backend
// turns into the `global_load/store v, v_off, s[base:base+1]` form (no 64-bit per-lane address arithmetic).
template <class T>
__device__ __forceinline__ T ldg(const void *sbase, uint32_t voff) {
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(sbase) + voff);
}
template <class T>
__device__ __forceinline__ void stg(void *sbase, uint32_t voff, T v) {
    *reinterpret_cast<T *>(reinterpret_cast<char *>(sbase) + voff) = v;
}
// write-through store (`global_store ... sc1`): the bytes leave the XCD's L2 right away instead of staying dirty until
// the end-of-kernel write-back, which would otherwise serialise ~B / 6 TB/s behind the kernel (MI355X_MICROARCH.md,
// "boundary" and "publish-large" rows).  Used for the streaming outputs (observations), which nobody re-reads on the GPU.
template <class T>
__device__ __forceinline__ void stg_wt(void *sbase, uint32_t voff, T v) {
    __hip_atomic_store(reinterpret_cast<T *>(reinterpret_cast<char *>(sbase) + voff), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef uint32_t uint2_t __attribute__((ext_vector_type(2)));
typedef uint32_t uint4_t __attribute__((ext_vector_type(4)));

// Loads are clamped instead of exec-masked (no branches): every address stays inside the record.
template <int OPL, int CPL, int NA, bool LEAN = false, class PB>
__device__ __forceinline__ void load_env(const PB &P, Env<OPL, CPL, NA> &e, const Ctx &cx, const uint32_t *__restrict__ rec) {
    const uint32_t lane = (uint32_t)cx.lane;
    // header words: wave-uniform, one scalar load (nothing in this kernel writes a record before its loads are done, and the
    // scalar cache is cold at kernel start like every other cache)
    uint32_t hw[HDR_WORDS];
    {
        typedef const __attribute__((address_space(4))) uint32_t *kconst_u32;
        const kconst_u32 hp = (kconst_u32)rec;
#pragma unroll
        for (int i = 0; i < HDR_WORDS; ++i) hw[i] = hp[i];
    }
    const uint32_t aw = ldg<uint32_t>(rec, (AGENT_WORD0 + (lane & 3u)) * 4u);        // agent words, lane a = agent a
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const uint32_t c = lane + 64u * k;
        const uint32_t v = ldg<uint8_t>(rec, CELL_WORD0 * 4u + min(c, (uint32_t)cx.C - 1u));
        e.cell[k] = (c < (uint32_t)cx.C) ? v : 0u;
    }
#pragma unroll
    for (int k = 0; k < OPL; ++k) {
        const uint32_t s = lane + 64u * k, sc = min(s, (uint32_t)cx.D - 1u);
        const uint32_t a = ldg<uint32_t>(rec, ((uint32_t)P.dyn0_off + sc) * 4u), b = ldg<uint32_t>(rec, ((uint32_t)P.dyn1_off + sc) * 4u);
        e.d0[k] = (s < (uint32_t)cx.D) ? a : 0u;
        e.d1[k] = (s < (uint32_t)cx.D) ? b : 0u;
    }
    // every load of the record is issued before anything looks at a header word (whose first use waits for the scalar load:
    // without the fence the scheduler puts that wait, a memory round trip, in front of the remaining vector loads)
    __builtin_amdgcn_sched_barrier(0);
    e.t = hw[W_T]; e.marks = hw[W_MARKS]; e.layout = hw[W_LAYOUT]; e.status = hw[W_STATUS];
    e.episode = hw[W_EPISODE]; e.recipes = hw[W_RECIPES]; e.pool = hw[W_POOL];
    // (this test is also where the wave waits for its late scalar arguments -- before any LDS traffic is in flight, which
    // shares the wait counter with scalar loads: measured 0.1 us better than letting the first use wait further down)
    e.marks_hi = !LEAN && P.wide ? hw[W_MARKS_HI] : 0u;
    e.agw = (lane < (uint32_t)NA) ? aw : 0u;
}

// header + agents in one 12-lane store (v_writelane assembles the words), cells / objects only when they changed;
template <int OPL, int CPL, int NA, class PB>
__device__ __forceinline__ void store_env(const PB &P, const Env<OPL, CPL, NA> &e, const Ctx &cx, uint32_t *__restrict__ rec,
                                          bool cells_dirty, bool objs_dirty, bool header_dirty = true) {
    const uint32_t lane = (uint32_t)cx.lane;
    if (header_dirty) {
        uint32_t h = 0;
        h = wrl(e.t, W_T, h);
        h = wrl(e.marks, W_MARKS, h);
        h = wrl(e.layout, W_LAYOUT, h);
        h = wrl(e.status, W_STATUS, h);
        h = wrl(e.episode, W_EPISODE, h);
        h = wrl(e.recipes, W_RECIPES, h);
        h = wrl(e.pool, W_POOL, h);
        h = wrl(e.marks_hi, W_MARKS_HI, h);
        if (lane < (uint32_t)HDR_WORDS) stg<uint32_t>(rec, lane * 4u, h);
    } else if (lane == 0u) {
        stg<uint32_t>(rec, W_T * 4u, e.t);                          // the step counter is all that changed (the usual case)
    }
    if (lane < (uint32_t)MAX_AGENTS) stg<uint32_t>(rec, (AGENT_WORD0 + lane) * 4u, e.agw);
    if (cells_dirty) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const uint32_t c = lane + 64u * k;
            if (c < (uint32_t)cx.C) stg<uint8_t>(rec, CELL_WORD0 * 4u + c, (uint8_t)e.cell[k]);
        }
    }
    if (objs_dirty) {
#pragma unroll
        for (int k = 0; k < OPL; ++k) {
            const uint32_t s = lane + 64u * k;
            if (s < (uint32_t)cx.D) {
                stg<uint32_t>(rec, ((uint32_t)P.dyn0_off + s) * 4u, e.d0[k]);
                stg<uint32_t>(rec, ((uint32_t)P.dyn1_off + s) * 4u, e.d1[k]);
            }
        }
    }
}

// the recipe rows of this env, one word per lane: lane 9r + i = word i of the row of recipe r (which r, i a lane stands for is
// a constant of the lane, made by the host: 8 r | 4 i << 8; lanes past the rows repeat the last word)
// (the selector does not depend on the record: step_kernel fetches it with its first loads, load_row_selector, and hands it over -
// fetched here, behind the wait for the header's `recipes`, it is a second memory round trip in front of the row's load)
template <class PB>
__device__ __forceinline__ uint32_t load_row_selector(const PB &P, int lane) { return ldg<uint32_t>(P.lut, ROWSEL_TABLE_OFFSET + (uint32_t)lane * 4u); }
template <class PB>
__device__ __forceinline__ uint32_t load_recipe_rows(const PB &P, uint32_t recipes, uint32_t sel) {
    const uint32_t id = (recipes >> (sel & 0xFFu)) & 0xFFu;
    return ldg<uint32_t>(P.recipes, __umul24(id, (1u + MAX_NODES) * 4u) + (sel >> 8));
}
template <class PB>
__device__ __forceinline__ uint32_t load_recipe_rows(const PB &P, uint32_t recipes, int lane) {
    return load_recipe_rows(P, recipes, load_row_selector(P, lane));
}

// every recipe of the env from scratch (reset): sets e.marks (and e.marks_hi for wide tables)
template <int OPL, int CPL, int NA, bool LEAN = false, class PB>
__device__ __forceinline__ void all_marks(const PB &P, Env<OPL, CPL, NA> &e, const Ctx &cx, uint32_t rowv, Lds<CPL> &s) {
    uint32_t lo = 0, hi = 0;
    if (!LEAN && __builtin_expect(P.wide != 0, 0)) {
#pragma nounroll
        for (int r = 0; r < P.R; ++r) {
            const uint32_t id = (e.recipes >> (8 * r)) & 0xFFu;
            const uint32_t m = Ops<OPL, CPL, NA, 3>::recipe_marks_wide(e, cx, P.recipes + (size_t)id * (1 + 2 * WIDE_NODES), s.locs);
            if (r < 2) lo |= m << (16 * r); else hi |= m << (16 * (r - 2));
        }
    } else {
        if constexpr (CPL <= 4) {
            lo = Ops<OPL, CPL, NA, 3>::recipe_marks_cells(e, cx, rowv, 0xFu, P.R, s.locs);
        } else {
#pragma nounroll
            for (int r = 0; r < P.R; ++r) lo |= Ops<OPL, CPL, NA, 3>::recipe_marks(e, cx, rowv, 9 * r, s.locs) << (8 * r);
        }
    }
    e.marks = lo; e.marks_hi = hi;
}

// the per-lane constant of the subtrahend table (observe): word `lane` behind the 256 doubles of the quotient table
template <class PB>
__device__ __forceinline__ uint32_t load_submask(const PB &P, int lane) { return ldg<uint32_t>(P.lut, (uint32_t)(LUT_SIZE * 8 + lane * 4)); }

// once per kernel and workgroup: the quotient table (thread `tid` of `nthreads`), followed by a workgroup barrier
__device__ __forceinline__ void init_lut(const Params &P, double *lut, int tid, int nthreads) {
    for (int i = tid; i < LUT_SIZE; i += nthreads) lut[i] = ldg<double>(P.lut, (uint32_t)i * 8u);
}

// once per kernel and env: the constant part of the image (cell coordinates: a host-made table, one word per cell)
// (the table's words are constants of the lane, load_coord_words: step_kernel fetches them with its first loads and hands them over;
// k_reset and k_observe, which wait for nothing in front of this, fetch them here)
template <int CPL> struct CoordWords { uint32_t w[CPL]; };
template <int CPL, class PB>
__device__ __forceinline__ CoordWords<CPL> load_coord_words(const PB &P, int lane) {
    CoordWords<CPL> cw;
#pragma unroll
    for (int k = 0; k < CPL; ++k) cw.w[k] = ldg<uint32_t>(P.lut, COORD_TABLE_OFFSET + (uint32_t)(lane + 64 * k) * 4u);
    return cw;
}
template <int CPL>
__device__ __forceinline__ void init_lds(const Ctx &cx, Lds<CPL> &s, const CoordWords<CPL> &cw) {
    const int lane = cx.lane;
    s.img[Img<CPL>::ZERO] = (uint16_t)(LUT_ABSENT * 8);           // (every lane, same value: cheaper than switching lanes off)
    uint32_t *img32 = reinterpret_cast<uint32_t *>(s.img);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const uint32_t c = (uint32_t)(lane + 64 * k);
        img32[(Img<CPL>::CELL0 >> 1) + 2 * c] = cw.w[k];
    }
}
template <int CPL, class PB>
__device__ __forceinline__ void init_lds(const PB &P, const Ctx &cx, Lds<CPL> &s) {
    const int lane = cx.lane;
    s.img[Img<CPL>::ZERO] = (uint16_t)(LUT_ABSENT * 8);
    uint32_t *img32 = reinterpret_cast<uint32_t *>(s.img);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const uint32_t c = (uint32_t)(lane + 64 * k);
        img32[(Img<CPL>::CELL0 >> 1) + 2 * c] = ldg<uint32_t>(P.lut, COORD_TABLE_OFFSET + c * 4u);
    }
}

// the descriptor words of this lane for one chunk: pair i of a chunk covers features [(chunk*OBS_PAIRS + i)*128 + 2*lane, +1].
// Buffer loads over one resource that spans the whole descriptor table (the layout's row is the scalar offset): no clamps, no
// masks, no branches on F.  Words past the row's F descriptors are the next layout's - valid image offsets like any other,
// read for nothing since the stores of features past F are out of their row's range - or, behind the table's end, 0.
template <class PB>
__device__ __forceinline__ void load_desc(const PB &P, uint32_t layout, int chunk, int lane, uint32_t (&dsc)[OBS_CHUNK]) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(P.lay_desc), 0, P.L * P.F * 4, 0x00020000);
    const uint32_t row = layout * (uint32_t)P.F * 4u;                                       // uniform
#pragma unroll
    for (int i = 0; i < OBS_CHUNK / 2; ++i) {
        const uint32_t f = (uint32_t)(chunk * (OBS_CHUNK / 2) + i) * 128u + 2u * (uint32_t)lane;
        const uint2_t d = __builtin_bit_cast(uint2_t, __builtin_amdgcn_raw_buffer_load_b64(rs, f * 4u, row, 0));
        dsc[2 * i] = d.x; dsc[2 * i + 1] = d.y;
    }
}

// cooking_env.py:352-373 get_feature_vector for every agent of the env: out[a][f] = lut[img[desc.hw] - sub[a][desc.code]]
// P.wt selects the cache policy of the observation stores (wave-uniform; policy in cz_api.hip launch_step):
//   1 = write-through (`buffer_store_dwordx4 ... sc1`): the bytes leave the XCD's L2 while the kernel still computes instead
//       of staying dirty until the end-of-kernel write-back (which serialises ~B / 6 TB/s behind every launch:
//       MI355X_MICROARCH.md "boundary" / "publish-large").  Pays for one launch per step of a moderate batch.
//   2 = streaming (`... nt`): for output buffers larger than the memory-side cache.  With plain stores a launch's 278+ MiB of
//       observations sweep the 256 MiB Infinity Cache, so the records, tables and descriptors the NEXT waves read come
//       from HBM, queued behind the writes: a one-step launch of 65 536 envs takes 80 us with plain stores and 56 us with
//       streaming ones (profiles/r03/aux_sweep.txt).
//   0 = plain: the fused kernel (its launch boundary is amortised over T steps) and batches in between.
// `codes` (optional, cz_step_device_compact): the same observation as ONE BYTE per feature - the index of the table entry
// the feature's value is, out[a][f] == lut[codes[a][f]] bit for bit - in rows of codes_pitch(F) bytes (padding: 255, an entry
// that is 0.0): 1/8 of the bytes for consumers that stay on the device.  Lanes take four adjacent features each, one
// descriptor b128 load and one 4-byte store per observer and 256 features; no table reads at all.  `out` may be null then.
__host__ __device__ inline int codes_pitch(int F) { return (F + 15) & ~15; }
// the descriptor words of this lane's first four features, fetched with the prologue's loads (layout: which row they are of)
constexpr int CODES_PREFETCH = 2;               // rounds of 256 features (F = 278: both)
struct CodesPrefetch { uint4_t d[CODES_PREFETCH]; uint32_t layout; };
template <class PB>
__device__ __forceinline__ uint4_t load_desc4(const PB &P, uint32_t layout, uint32_t f) {
    const auto rd = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(P.lay_desc), 0, P.L * P.F * 4, 0x00020000);
    return __builtin_bit_cast(uint4_t, __builtin_amdgcn_raw_buffer_load_b128(rd, f * 4u, layout * (uint32_t)P.F * 4u, 0));
}
typedef unsigned short ushort2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_sub_u16(uint32_t a, uint32_t b) {                       // v_pk_sub_u16: two 16-bit lanes, no borrow across
    return __builtin_bit_cast(uint32_t, (ushort2_t)(__builtin_bit_cast(ushort2_t, a) - __builtin_bit_cast(ushort2_t, b)));
}
// The LDS image of one env, which every form of the observation is gathered from: objects, cells, agents and the per-observer
// subtrahend table, up to the wave barrier behind them.
template <int OPL, int CPL, int NA, class PB>
__device__ __forceinline__ void build_image(const PB &P, const Env<OPL, CPL, NA> &e, const Ctx &cx, Lds<CPL> &s, uint32_t submask,
                                            bool objs_changed, bool cells_changed) {
    uint32_t *img32 = reinterpret_cast<uint32_t *>(s.img);
    const uint32_t dead = (uint32_t)(LUT_ABSENT * 8) * 0x10001u;
    const uint32_t c01 = (uint32_t)((P.W - 1) * 8) | ((uint32_t)((LUT_Y0 + P.H - 1) * 8) << 16);
    // Flags are not computed: the halfword of a flag is the entry of a small truth table, indexed by the raw state bits
    // (LUT_NDONE0 / LUT_CH0 / LUT_MA0 by chopped | mashed << 1, LUT_CF0 by the cell's ACTIVE | WALK << 1 bits, LUT_OR0 + 8 k
    // by the orientation), so an image word is one multiply-add of the extracted field.
    constexpr uint32_t PICK_XY = 0x0C010C00u;                       // v_perm_b32: bytes x, 0, y, 0 of a word x | y << 8 | ...
    // ---- objects: 3 dwords per slot (in a fused rollout only when an object moved or changed state since the last encode)
    if (objs_changed)
#pragma unroll
    for (int k = 0; k < OPL; ++k) {
        const uint32_t w = e.d0[k];
        const bool alive = (w & D_ALIVE) != 0u;
        const uint32_t st = (w >> 25) & 3u;
        uint32_t q0 = (__builtin_amdgcn_perm(0u, w, PICK_XY) << 3) + c01;
        uint32_t q1 = __umul24(st, 0x80008u) + ((uint32_t)(LUT_NDONE0 * 8) | ((uint32_t)(LUT_CH0 * 8) << 16));
        uint32_t q2 = (st << 3) + ((uint32_t)(LUT_MA0 * 8) | ((uint32_t)(LUT_ONE * 8) << 16));
        q0 = alive ? q0 : dead; q1 = alive ? q1 : dead; q2 = alive ? q2 : dead;
        const int slot = cx.lane + 64 * k;
        img32[(Img<CPL>::OBJ0 >> 1) + 3 * slot] = q0;
        img32[(Img<CPL>::OBJ0 >> 1) + 3 * slot + 1] = q1;
        img32[(Img<CPL>::OBJ0 >> 1) + 3 * slot + 2] = q2;
    }
    // ---- cells: the mutable flag (switch_active / block walkable) + the constant 1
    if (cells_changed)
#pragma unroll
    for (int k = 0; k < CPL; ++k)
        img32[(Img<CPL>::CELL0 >> 1) + 2 * (cx.lane + 64 * k) + 1] =
            ((e.cell[k] >> 2) & 0x18u) | ((uint32_t)(LUT_CF0 * 8) | ((uint32_t)(LUT_ONE * 8) << 16));
    // ---- agents: 4 dwords each (lane a builds agent a's), and the per-observer subtrahend table
    {
        const uint32_t A = e.agw;
        const uint32_t o8 = __umul24((A >> 16) & 7u, 0x80008u);
        if (cx.lane < NA) {
            uint4_t agv;
            agv.x = (__builtin_amdgcn_perm(0u, A, PICK_XY) << 3) + c01;
            agv.y = o8 + ((uint32_t)((LUT_OR0 + 0) * 8) | ((uint32_t)((LUT_OR0 + 8) * 8) << 16));
            agv.z = o8 + ((uint32_t)((LUT_OR0 + 16) * 8) | ((uint32_t)((LUT_OR0 + 24) * 8) << 16));
            agv.w = (uint32_t)(LUT_ONE * 8);
            *reinterpret_cast<uint4_t *>(img32 + (Img<CPL>::AG0 >> 1) + 4 * cx.lane) = agv;
        }
        // sub[a][code]: lane 16a + code.  axis codes: 1 -> x, 2 -> y, 4+2j -> x unless j == a, 5+2j -> y unless j == a.  Which
        // coordinate a lane's entry takes is a constant of the lane: `submask` (0x7F8 in the low half: x, in the high half:
        // y), made by the host next to the quotient table and loaded with the prologue's loads.
        const uint32_t Ao = (uint32_t)__builtin_amdgcn_ds_bpermute((cx.lane >> 4) << 2, (int)A);     // the observer's word
        const uint32_t q = ((__builtin_amdgcn_perm(0u, Ao, PICK_XY) << 3) & submask);               // x * 8 | y * 8 << 16, masked
        (&s.sub[0][0])[cx.lane] = (int)((q & 0xFFFFu) + (q >> 16));         // (rows of observers >= NA: never read)
    }
    __builtin_amdgcn_wave_barrier();             // one wave owns this LDS region: DS ops of a wave execute in order
}

// The float32 rows (STEP_F32, k_observe_f32) from the image build_image has made: `out32` is float[A][F] of this env - dense rows, no
// pitch - and `lut` the FLOAT32 table (256 floats: every entry the float64 one rounded to nearest even).  Shaped like observe's codes
// path: a lane takes four adjacent features per round of 256, one descriptor b128 load (`pre` holds the first rounds'), and one 16-byte
// store per observer whose range, F * 4 bytes from the row's base, drops what lies past the row - nothing is written behind a row, there
// is no padding.  P.wt selects the stores' cache policy as in observe.
// (The descriptor / image / subtrahend gather is spelled out here and in observe's codes loop: moved into one helper of both, 32 of the
// small instance's 76 instruction streams change and k_observe grows by 46 to 78 instructions.)
template <int OPL, int CPL, int NA>
__device__ __forceinline__ void write_rows_f32(const Params &P, const Env<OPL, CPL, NA> &e, const Ctx &cx, Lds<CPL> &s, const float *lut,
                                               float *__restrict__ out32 /* [A][F] of this env */, CodesPrefetch *pre) {
    const char *lutb = reinterpret_cast<const char *>(lut);
    const char *imgb = reinterpret_cast<const char *>(s.img);
    const char *subb = reinterpret_cast<const char *>(s.sub);
    decltype(__builtin_amdgcn_make_buffer_rsrc(out32, 0, 0, 0)) r32[NA];
    // (a row starts wherever the rows before it end: 4-byte aligned when F is odd.  Buffer stores of several dwords need dword
    // alignment only, and the range check works dword by dword - what the float64 rows of an odd F, 8-byte aligned, rely on too)
#pragma unroll
    for (int a = 0; a < NA; ++a) r32[a] = __builtin_amdgcn_make_buffer_rsrc(out32 + (size_t)a * (uint32_t)P.F, 0, P.F * 4, 0x00020000);
    const uint32_t wt = (uint32_t)P.wt;                                              // wave-uniform
    for (int f0 = 0; f0 < P.F; f0 += 256) {
        const uint32_t f = (uint32_t)f0 + 4u * (uint32_t)cx.lane;                       // this lane's first feature
        uint4_t d;
        if (pre && f0 < 256 * CODES_PREFETCH) d = f0 == 0 ? pre->d[0] : pre->d[1];
        else d = load_desc4(P, e.layout, f);
        const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
        uint32_t b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = *reinterpret_cast<const uint16_t *>(imgb + (dw[k] & 0xFFFFu));
        int sb[NA][4];
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int k = 0; k < 4; ++k) sb[a][k] = *reinterpret_cast<const int32_t *>(subb + 64 * a + (dw[k] >> 16));
        // image halfword - subtrahend: the byte offset into the float64 table (a multiple of 8); halved, into the float32 one
        uint4_t v[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = *reinterpret_cast<const uint32_t *>(lutb + (((int)b[k] - sb[a][k]) >> 1));
            v[a].x = w[0]; v[a].y = w[1]; v[a].z = w[2]; v[a].w = w[3];
        }
#define CZ_OBS_WRITE_ROWS32(AUX)                                                                                             \
    _Pragma("unroll") for (int a = 0; a < NA; ++a) __builtin_amdgcn_raw_buffer_store_b128(v[a], r32[a], f * 4u, 0, AUX)
        if (wt == 1u) { CZ_OBS_WRITE_ROWS32(16); }          // sc1: write-through
        else if (wt == 2u) { CZ_OBS_WRITE_ROWS32(2); }      // nt: streaming
        else { CZ_OBS_WRITE_ROWS32(0); }
#undef CZ_OBS_WRITE_ROWS32
    }
    __builtin_amdgcn_wave_barrier();
}

// LEAN (k_step_lean, see StepTraits): float64 rows present, write-through stores and F <= 128 * OBS_PAIRS, all known at compile
// time - one chunk, no store-flavour switch, no descriptor reload.  F64 = false: the codes-only variant, which carries no float64 path.
// (The codes loop and the float64 loop stay in this function: moved into functions of their own, 20 of the small instance's 76
// instruction streams change by an instruction - k_reset, k_observe and some k_step<..., 3 / 5> among them.)
template <int OPL, int CPL, int NA, bool F64 = true, bool LEAN = false, class PB>
__device__ __forceinline__ void observe(const PB &P, const Env<OPL, CPL, NA> &e, const Ctx &cx, Lds<CPL> &s,
                                        const double *lut, uint32_t (&dsc)[OBS_CHUNK], uint32_t submask, double *__restrict__ out /* [A][F] of this env */,
                                        bool objs_changed = true, bool cells_changed = true, uint8_t *__restrict__ codes = nullptr /* [A][Fp] */,
                                        CodesPrefetch *pre = nullptr) {
    build_image<OPL, CPL, NA>(P, e, cx, s, submask, objs_changed, cells_changed);
    // One buffer resource per observer whose range is exactly that observer's row (F * 8 bytes): the per-lane offset
    // (feature index * 8) is range-checked by the hardware, dword by dword (the scalar offset would be part of that check,
    // so the row's base goes into the resource).  Features past F - whole pairs, or the second half of the last pair when
    // F is odd - are dropped by the memory pipeline and the store sequence needs no lane masks or branches at all.
    const char *lutb = reinterpret_cast<const char *>(lut);
    const char *imgb = reinterpret_cast<const char *>(s.img);
    const char *subb = reinterpret_cast<const char *>(s.sub);
    if (codes) {
        const int Fp = codes_pitch(P.F);
        decltype(__builtin_amdgcn_make_buffer_rsrc(codes, 0, 0, 0)) rc[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) rc[a] = __builtin_amdgcn_make_buffer_rsrc(codes + (size_t)a * (uint32_t)Fp, 0, Fp, 0x00020000);
        // (the first rounds' descriptor words come in registers: fetched behind the prologue or at the top of a fused step, and
        // fetched again by the caller when a reset pass has moved the env to another layout - `pre` is of e.layout here)
        for (int f0 = 0; f0 < P.F; f0 += 256) {
            const uint32_t f = (uint32_t)f0 + 4u * (uint32_t)cx.lane;                       // this lane's first feature
            uint4_t d;
            if (pre && f0 < 256 * CODES_PREFETCH) d = f0 == 0 ? pre->d[0] : pre->d[1];
            else d = load_desc4(P, e.layout, f);
            const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
            uint32_t b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = *reinterpret_cast<const uint16_t *>(imgb + (dw[k] & 0xFFFFu));
            int sb[NA][4];
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int k = 0; k < 4; ++k) sb[a][k] = *reinterpret_cast<const int32_t *>(subb + 64 * a + (dw[k] >> 16));
            // A code is (image halfword - subtrahend) >> 3, both multiples of 8 below 2048: two features share a register as 16-bit
            // halves (v_pk_sub_u16), one 32-bit shift by 3 leaves each code in the low byte of its half, v_perm_b32 gathers the
            // four bytes of a lane; bytes past F are forced to the padding value by an OR (vector-only: no scalar work per round)
            const uint32_t p01 = b[0] | (b[1] << 16), p23 = b[2] | (b[3] << 16);
            const int left = P.F - (int)f;                                                  // features of this lane that exist
            const uint32_t pad = left >= 4 ? 0u : left <= 0 ? 0xFFFFFFFFu : (0xFFFFFFFFu << (8u * (uint32_t)left));
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const uint32_t s01 = (uint32_t)sb[a][0] | ((uint32_t)sb[a][1] << 16), s23 = (uint32_t)sb[a][2] | ((uint32_t)sb[a][3] << 16);
                const uint32_t c01 = pk_sub_u16(p01, s01) >> 3, c23 = pk_sub_u16(p23, s23) >> 3;
                // (write-through like the float64 rows of a one-step launch: nothing stays dirty until the end-of-kernel write-back)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_amdgcn_perm(c23, c01, 0x06040200u) | pad, rc[a], f, 0, 16);
            }
        }
    }
    if (!F64 || (!LEAN && !out)) { __builtin_amdgcn_wave_barrier(); return; }
    decltype(__builtin_amdgcn_make_buffer_rsrc(out, 0, 0, 0)) rs[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) rs[a] = __builtin_amdgcn_make_buffer_rsrc(out + (size_t)a * (uint32_t)P.F, 0, P.F * 8, 0x00020000);
    const uint32_t wt = LEAN ? 1u : (uint32_t)P.wt;                                  // wave-uniform
    for (int chunk = 0; LEAN ? chunk == 0 : chunk * 128 * OBS_PAIRS < P.F; ++chunk) {
        if (chunk > 0) load_desc(P, e.layout, chunk, cx.lane, dsc);
        // branch-free stages so that the LDS reads of all pairs and observers are in flight together
        // (descriptor words past F are 0: they read image halfword 0 and their stores are out of range)
        uint32_t b[OBS_CHUNK];
        int sb[NA][OBS_CHUNK];
        double2_t v[NA][OBS_PAIRS];
#pragma unroll
        for (int j = 0; j < OBS_CHUNK; ++j) b[j] = *reinterpret_cast<const uint16_t *>(imgb + (dsc[j] & 0xFFFFu));
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int j = 0; j < OBS_CHUNK; ++j) sb[a][j] = *reinterpret_cast<const int32_t *>(subb + 64 * a + (dsc[j] >> 16));
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int i = 0; i < OBS_PAIRS; ++i) {
                v[a][i].x = *reinterpret_cast<const double *>(lutb + ((int)b[2 * i] - sb[a][2 * i]));
                v[a][i].y = *reinterpret_cast<const double *>(lutb + ((int)b[2 * i + 1] - sb[a][2 * i + 1]));
            }
        const uint32_t f0b = (uint32_t)(chunk * OBS_PAIRS * 128 + 2 * cx.lane) * 8u;      // byte offset of this lane's first pair
#define CZ_OBS_WRITE_ROWS(AUX)                                                                                               \
    _Pragma("unroll") for (int i = 0; i < OBS_PAIRS; ++i)                                                                    \
        _Pragma("unroll") for (int a = 0; a < NA; ++a)                                                                       \
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, v[a][i]), rs[a], f0b + (uint32_t)i * 1024u, 0, AUX)
        if (wt == 1u) { CZ_OBS_WRITE_ROWS(16); }            // sc1: write-through
        else if (wt == 2u) { CZ_OBS_WRITE_ROWS(2); }        // nt: streaming
        else { CZ_OBS_WRITE_ROWS(0); }
#undef CZ_OBS_WRITE_ROWS
    }
    // the caller keeps the descriptors of chunk 0 across steps (fused rollout): restore them if later chunks replaced them
    if (!LEAN && P.F > 128 * OBS_PAIRS) load_desc(P, e.layout, 0, cx.lane, dsc);
    __builtin_amdgcn_wave_barrier();
}

struct StepOut {
    double myrew;                  // lane a < NA: the reward of agent a (cooking_env.py:255-261); 0.0 on the other lanes
    uint32_t term, trunc;
    bool stepped, finished;        // a world step was executed / it ended the episode
    bool header;                   // a header word other than `t` changed (marks, status, episode, layout)
    uint32_t gone;                 // despawn / respawn: bit a = agent a left in this step (reported truncated once)
#ifdef CZ_TIMELINE
    uint32_t dbg;                  // timeline build: 1 an object moved or changed, 2 recipe graphs re-evaluated, 4 marks changed, 8 somebody interacted
#endif
};

// One accumulated_step (cooking_env.py:243-269) of one env held in registers.
// FUSED (CZ_RARE): the reset pass and the end of an episode are laid out off the fall-through path - one step in max_steps + 1
// takes them; in the one-step kernels the same hint cost the launches under a cooking policy 1.5 % (profiles/r05/ab_experiments.txt)
#define CZ_RARE(hint, x) ((hint) ? __builtin_expect(!!(x), 0) : !!(x))
template <int OPL, int CPL, int NA, int SCHEME, bool FUSED, bool LEAN, class PB>
__device__ __forceinline__ void step_env(const PB &P, unsigned kp_off, Env<OPL, CPL, NA> &e, const Ctx &cx, uint32_t acts,
                                         int64_t env_global, uint32_t &rowv, Lds<CPL> &lds, uint32_t (&dsc)[OBS_CHUNK], Dirty &dt, StepOut &o) {
    using O = Ops<OPL, CPL, NA, SCHEME>;
    o.myrew = 0.0;
    o.term = 0; o.trunc = 0; o.stepped = false; o.finished = false; o.header = false; o.gone = 0u;
#ifdef CZ_TIMELINE
    o.dbg = 0u;
#endif
    // P.auto_reset: bit 0 = next-step auto-reset, bit 1 = agent despawn / respawn is on (cz_set_spawn)
    const bool spawning = !LEAN && (P.auto_reset & 2) != 0;
    const SpawnCfg *const spawn_cfg = reinterpret_cast<const SpawnCfg *>(reinterpret_cast<const char *>(P.lut) + SPAWN_CFG_OFFSET);
    if (CZ_RARE(FUSED, (e.status & ST_DONE) != 0u)) {
        o.header = true;
        if (P.auto_reset & 1) {
            // next-step autoreset: reset() of cooking_env.py:178-210 from the layout pool
            e.episode += 1;
            const uint32_t *const lay0 = late_params<block_of<PB>>(kp_off)->lay_init;
            // (the control words are constant while a kernel runs: the host changes them between launches, in stream order)
            typedef const __attribute__((address_space(4))) uint32_t *kconst_u32;
            const kconst_u32 ctl = (kconst_u32)(lay0 - LAY_CTL_WORDS);
            uint32_t lay = next_layout(env_global, e.episode, e.pool, (uint32_t)P.L, ctl[LC_GROUPS], ctl[LC_ACTIVE]);
            uint32_t recipes = e.recipes, episode = e.episode, pool = e.pool;
            load_env<OPL, CPL, NA, LEAN>(P, e, cx, lay0 + (size_t)lay * P.RW);
            e.t = 0; e.layout = lay; e.status = 0; e.episode = episode; e.recipes = recipes; e.pool = pool;
            if (spawning) {       // a fresh world: everybody present, grace periods running (load_level.py:67-68, parsing.py:142)
                typedef const __attribute__((address_space(4))) SpawnCfg *kcfg;
                e.status = spawn_initial_status(((kcfg)spawn_cfg)->grace_period, NA);
            }
            all_marks<OPL, CPL, NA, LEAN>(P, e, cx, rowv, lds);
            if (LEAN || P.obs) load_desc(P, lay, 0, cx.lane, dsc);
            dt.cells = 1; dt.touched = 1; dt.interacted = 1;          // everything must be written back
        } else {
            o.term = (e.status & ST_TERM) ? 1u : 0u;
            o.trunc = (e.status & ST_TRUNC) ? 1u : 0u;
        }
        return;
    }
    o.stepped = true;
    e.t += 1;                                                        // cooking_env.py:244
    // (a despawned agent is not in the list world_step acts on, cooking_world.py:105-108: agents_walk takes it out like an
    // agent with action -1)
#if defined(CZ_PROFILE)
    const int lane = cx.lane; const long long env = env_global - P.env_id_base;
#endif
    O::perform_agent_actions(e, cx, acts, dt);                      // cooking_world.py:104-108
    CZ_STAMP(2);
    O::progress_and_link(e, cx, dt);
    if (spawning) {                             // :109-110 handle_agent_spawn
        o.gone = O::handle_agent_spawn(e, cx, spawn_cfg, env_global);
        o.header = true;                        // (the grace counters live in the status word)
    }
    CZ_STAMP(3);
    // compute_rewards cooking_env.py:290-315
    const bool truncated = (int)e.t >= P.max_steps;                 // compute_truncated :333-350
    const uint32_t before = e.marks;
    uint32_t after = before;
    o.myrew = cx.lane < NA ? P.reward_idle : 0.0;
    if (dt.moved & (uint32_t)P.walk_touches) { dt.touched = 1; dt.kinds = ~0ull; }
    if (dt.kinds & 0xFull) dt.kinds = ~0ull;                        // a Plate moved: it drags its content along -> anything
    bool done = false;
    if (!LEAN && __builtin_expect(P.wide != 0, 0)) {
        // Wide recipe tables (a graph with more than 8 nodes in the book): no filters, every recipe of the env is
        // re-evaluated whenever an object moved or changed; marks are 16 bits per recipe (recipes 0, 1 in `marks`, 2, 3 in
        // `marks_hi`).  Without a change the marks, hence `done` (false, or the env would not be stepping), stay.
        if (dt.touched) {
            uint32_t lo = 0, hi = 0;
#pragma nounroll
            for (int r = 0; r < P.R; ++r) {
                const uint32_t id = (e.recipes >> (8 * r)) & 0xFFu;
                const uint32_t *row = P.recipes + (size_t)id * (1 + 2 * WIDE_NODES);
                const uint32_t mb_r = ((r < 2 ? e.marks : e.marks_hi) >> (16 * (r & 1))) & 0xFFFFu;
                const uint32_t ma = O::recipe_marks_wide(e, cx, row, lds.locs);
                if (r < 2) lo |= ma << (16 * r); else hi |= ma << (16 * (r - 2));
                if (ma != mb_r) {
                    uint32_t countmask = 0;
                    const int n = (int)(rfl(row[0]) & 0xFFu);
#pragma nounroll
                    for (int j = 0; j < n; ++j) countmask |= ((rfl(row[1 + 2 * j]) >> 8) & 1u) << j;
                    const int goals_before = __popc(~mb_r & countmask), goals_after = __popc(~ma & countmask);
                    const bool completed = ma & 1, completion_before = mb_r & 1;
                    const bool malus = !completed && completion_before, bonus = completed && !completion_before;
                    const auto kp = late_params<block_of<PB>>(kp_off);
                    double x = 0.0;
                    x += (double)(goals_before - goals_after) * kp->node_reward;
                    x += (bonus ? 1.0 : 0.0) * kp->recipe_reward;
                    x += (malus ? 1.0 : 0.0) * kp->recipe_penalty;
                    x += kp->time_penalty_step;
                    if (cx.lane == r && r < NA) o.myrew = x;
                }
            }
            o.header |= lo != e.marks || hi != e.marks_hi;
            e.marks = lo; e.marks_hi = hi;
        }
        // recipe roots are bit 0 of each 16-bit field
        const uint32_t rlo = e.marks & (P.R >= 2 ? 0x00010001u : 0x00000001u);
        const uint32_t rhi = P.R >= 3 ? (e.marks_hi & (P.R >= 4 ? 0x00010001u : 0x00000001u)) : 0u;
        const int n_roots = __popc(rlo) + __popc(rhi);
        done = P.end_all ? (n_roots == P.R) : (n_roots != 0);
    } else {
        if (dt.touched) {
            // Which recipes must be re-evaluated?  Marks are a pure function of object state, and (recipe.py:77-104)
            //  * an object that matches no node of a recipe (class + state conditions) neither before nor after its change is
            //    in no node's matched list either way, and nothing else asks where it is: the recipe cannot see it;
            //  * a mere MOVE leaves every leaf's mark alone (leaves have no location constraint), so it can only matter to a
            //    node that has children, and such a node is only looked at when all its children are marked: if no node of
            //    the recipe is in that position now, no mark can change (induction from the leaves up).
            // Both tests run for all nodes of all recipes at once: lane 9r + 1 + j holds node j of recipe r (rowv).
            const uint32_t nw = rowv, lane_u = (uint32_t)cx.lane;
            const uint32_t r_of = (lane_u * 57u) >> 9;                                   // lane / 9
            const uint32_t seen = (uint32_t)(dt.kinds >> ((nw >> 14) & 0x3Cu)) & ((nw >> 24) & 0xFu);
            const uint32_t kids = nw & 0xFFu, mb = (before >> (8u * (r_of & 3u))) & 0xFFu;
            constexpr uint64_t NODE_LANES = 0x1FEull | (0x1FEull << 9) | (0x1FEull << 18) | (0x1FEull << 27);
            const bool rel = (nw & 0x2000u) != 0u && seen != 0u, sens = kids != 0u && (mb & kids) == kids;
            // the rewards of recipe r whose marks went from mb_r to ma (cooking_env.py:255-261, recipe.py:36-40)
            // (the wide path above carries its own copy of this: folded into one function, both forms tried, the compiler commutes
            // operands of two scalar instructions in every k_step - and the shipped streams are kept instruction for instruction)
            const auto reward_of = [&](int r, uint32_t mb_r, uint32_t ma) {
                // goals_completed sums (recipe.py:36-40): open goal slots before / after
                const uint32_t countmask = (uint32_t)((ballot((nw & 0x100u) != 0u) >> (9 * r + 1)) & 0xFFull);
                const int goals_before = __popc(~mb_r & countmask), goals_after = __popc(~ma & countmask);
                const bool completed = ma & 1, completion_before = mb_r & 1;
                const bool malus = !completed && completion_before, bonus = completed && !completion_before;
                const auto kp = late_params<block_of<PB>>(kp_off);
                double x = 0.0;
                x += (double)(goals_before - goals_after) * kp->node_reward;
                x += (bonus ? 1.0 : 0.0) * kp->recipe_reward;
                x += (malus ? 1.0 : 0.0) * kp->recipe_penalty;
                x += kp->time_penalty_step;
                if (cx.lane == r && r < NA) o.myrew = x;                       // recipe r is agent r's (cooking_env.py:255-261)
            };
            CZ_STAMP(8);
            if constexpr (CPL <= 4) {
                // "some node of recipe r" for both tests in one OR over the wave: bit r = visible, bit 4 + r = sensitive
                const uint32_t flags = (rel ? 1u : 0u) | (sens ? 16u : 0u);
                const uint32_t any = O::wave_or(lanes(NODE_LANES) ? (flags << (r_of & 3u)) : 0u);
                const uint32_t which = any & (dt.statechg != 0u ? 0xFu : (any >> 4)) & ((1u << P.R) - 1u);   // the recipes to re-evaluate
                if (which) {
                    CZ_SETPRIO(3);
#ifdef CZ_TIMELINE
                    o.dbg |= 2u;
#endif
                    const uint32_t fresh = O::recipe_marks_cells(e, cx, rowv, which, P.R, lds.locs);
                    CZ_STAMP(9);
                    const uint32_t bytes = ((which * 0x204081u) & 0x01010101u) * 0xFFu;    // bit r -> byte r
                    after = (before & ~bytes) | (fresh & bytes);
                    if (after != before) {
#pragma nounroll
                        for (int r = 0; r < P.R; ++r) {
                            const uint32_t mb_r = (before >> (8 * r)) & 0xFFu, ma = (after >> (8 * r)) & 0xFFu;
                            if (ma != mb_r) reward_of(r, mb_r, ma);
                        }
                    }
                }
            } else {
                const uint64_t relmask = ballot(rel) & NODE_LANES, sensmask = ballot(sens) & NODE_LANES;
                after = 0;
#pragma nounroll
                for (int r = 0; r < P.R; ++r) {
                    const uint32_t mb_r = (before >> (8 * r)) & 0xFF;
                    const bool visible = ((relmask >> (9 * r + 1)) & 0xFFull) != 0ull;
                    const bool sensitive = dt.statechg != 0u || ((sensmask >> (9 * r + 1)) & 0xFFull) != 0ull;
                    uint32_t ma = mb_r;
                    if (visible && sensitive) {
                        CZ_SETPRIO(3);
                        ma = O::recipe_marks(e, cx, rowv, 9 * r, lds.locs);
                    }
                    after |= ma << (8 * r);
                    if (ma != mb_r) reward_of(r, mb_r, ma);
                }
            }
            CZ_STAMP(10);
        }
        e.marks = after;
        o.header |= after != before;
#ifdef CZ_TIMELINE
        o.dbg |= (dt.touched ? 1u : 0u) | (after != before ? 4u : 0u) | (dt.interacted ? 8u : 0u);
#endif
        // recipe roots are bit 0 of each marks byte
        const uint32_t roots = after & 0x01010101u & (P.R >= 4 ? 0xFFFFFFFFu : ((1u << (8 * P.R)) - 1u));
        done = P.end_all ? (__popc(roots) == P.R) : (roots != 0u);
    }
    o.term = done ? 1u : 0u;
    o.trunc = truncated ? 1u : 0u;
    if (CZ_RARE(FUSED, done || truncated)) {
        e.status |= ST_DONE | (done ? ST_TERM : 0u) | (truncated ? ST_TRUNC : 0u);
        o.finished = true;
        o.header = true;
    }
}

// ENVS_PER_WG envs per workgroup (one wavefront each, no cross-wave communication); V: the variant (StepTraits).
// What the very first loads of a wave need travels as leading scalar kernel arguments: the build preloads them into
// SGPRs at wave launch (-mllvm -amdgpu-kernarg-preload-count, gfx940+), so the record / action / table loads are issued
// without waiting for an argument fetch; everything else stays in the by-value block `P0`, fetched meanwhile.
struct Early {
    uint32_t *state;               // Params::state
    const int32_t *actions;        // Params::actions
    const double *lut;             // Params::lut
    int32_t N, RW, W, H, D, dyn0_off, dyn1_off;
};
__host__ __device__ inline Early early_of(const Params &P) {
    return Early{P.state, P.actions, P.lut, P.N, P.RW, P.W, P.H, P.D, P.dyn0_off, P.dyn1_off};
}

template <int OPL, int CPL, int NA, int SCHEME, class V>
__device__ __forceinline__ void step_kernel(uint32_t *e_state, const int32_t *e_actions, const double *e_lut, int32_t e_N,
                                            int32_t e_RW, int32_t e_W, int32_t e_H, int32_t e_D, int32_t e_dyn0,
                                            int32_t e_dyn1, const typename V::Block &P0) {
#ifdef CZ_TIMELINE
    // Timeline build (make timeline -> libcookingzoo_hip_tl.so): the shipped kernel plus two reads of the device-wide 100 MHz
    // clock per wave - at its first instruction and behind its last store - and
    // one 16-byte store of lane 0.  No waits are added in between (unlike the phase stamps of `make prof`).
    const uint64_t tl_in = wall_clock64();
#endif
    typename V::View P{P0};
    P.state = e_state; P.actions = e_actions; P.lut = e_lut; P.N = e_N; P.RW = e_RW; P.W = e_W; P.H = e_H; P.D = e_D;
    P.dyn0_off = e_dyn0; P.dyn1_off = e_dyn1;
    constexpr int EPW = envs_per_wg<CPL>();
    __shared__ Lds<CPL> lds_all[EPW];
    __shared__ double lut[LUT_SIZE];
    int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)rfl(threadIdx.x >> 6);
    // (the last workgroup may be partial: its spare waves shadow the last env up to the barrier, then leave)
    const int env_raw = (int)blockIdx.x * EPW + wave;
    const int env = min(env_raw, P.N - 1);
    static_assert(64 * EPW >= LUT_SIZE, "one table entry per thread");
    // the quotient table is shared by the workgroup: its load joins the other loads of the prologue (no branch here:
    // a branch would split the kernel-argument fetch into several dependent round trips)
    const double lutv = ldg<double>(P.lut, min(threadIdx.x, (unsigned)LUT_SIZE - 1u) * 8u);
    // The encode's per-lane constant, fetched in front of the record: the wait for the record then covers it.  Fetched behind
    // the record (as until round 4) its first use - in the image build, behind the reward / termination stores - needed an
    // `s_waitcnt vmcnt(0)`: gfx950 counts loads and stores in one in-order counter, so that wait also stood for the
    // acknowledgement of every store issued before it (in a fused launch: the previous step's observation rows).
    // (The larger instances keep the late fetch, i.e. their round-3 code: their launches are bound by HBM writes, and on the
    // one box where the two forms differed the wait in front of the encode helped - config 5: 318-323 us per launch with it,
    // 338-342 us without.  Config 5 varies by +-4 % between boxes and allocations anyway, profiles/r04/cfg5_boxes.txt.)
    constexpr bool SUBMASK_EARLY = CPL == 1;
    uint32_t submask = 0;
    if (SUBMASK_EARLY) submask = load_submask(P, (int)(threadIdx.x & 63u));
    // The other two constants of the lane - the coordinate words of its cells (init_lds) and its recipe-row selector
    // (load_recipe_rows) - go out here as well, in front of load_env: none of them needs the record, and behind load_env's fence
    // the scheduler is free to put them behind the wait for the header words, where they are a second round trip into a cold L2
    // in front of the workgroup's barrier (k_step_lean was built that way until round 9).  The small instance only, like the
    // submask: the larger ones would hold up to 16 more registers across the record's loads, and their launches are bound by HBM.
    constexpr bool TABLES_EARLY = CPL == 1;
    CoordWords<CPL> coordw{};
    uint32_t rowsel = 0;
    if (TABLES_EARLY) {
        coordw = load_coord_words<CPL>(P, lane);
        rowsel = load_row_selector(P, lane);
    }
    Lds<CPL> &lds = lds_all[wave];
    Ctx cx{P.W, P.H, P.D, P.W * P.H, lane};
    CZ_STAMP(0);
    uint32_t *rec = P.state + (uint32_t)env * (uint32_t)P.RW;        // (cz_create: the records of a handle stay below 4 GiB)
    double *retp = reinterpret_cast<double *>(rec + RET_WORD0);
    int av = 0;
#ifdef CZ_TIMELINE
    const uint64_t tl_seen = wall_clock64();
#endif
    // ---- every load of the step is issued here, before anything waits
    if (!V::fused) av = ldg<int>(P.actions, ((uint32_t)env * (uint32_t)NA + (uint32_t)min(lane, NA - 1)) * 4u);
    double ret = ldg<double>(retp, ((uint32_t)lane & 3u) * 8u);                                       // running episode return, lane a = agent a
    Env<OPL, CPL, NA> e;
    load_env<OPL, CPL, NA, V::lean>(P, e, cx, rec);
    if constexpr (TABLES_EARLY) init_lds<CPL>(cx, lds, coordw); else init_lds<CPL>(P, cx, lds);
    uint32_t rowv = TABLES_EARLY ? load_recipe_rows(P, e.recipes, rowsel) : load_recipe_rows(P, e.recipes, lane);
    uint32_t dsc[OBS_CHUNK];
    if (V::f64 && (V::lean || P.obs)) load_desc(P, e.layout, 0, lane, dsc);
    if (!SUBMASK_EARLY) submask = load_submask(P, lane);
    const int64_t env_global = P.env_id_base + env;
    bool cells_dirty = false, objs_dirty = false, header_dirty = V::fused;
    bool img_objs = true, img_cells = true;                 // which parts of the LDS image the next encode must rebuild
    // (the float32 variants - STEP_F32, ROLLOUT_F32, ROLLOUT_ACTIONS_F32: the same array holds the float32 table - every entry rounded to
    // nearest even, v_cvt_f32_f64 in the default rounding mode, which is what cz_obs_table_f32 hands the host - so the float32 form adds
    // no load to the prologue)
    float *const lutf = reinterpret_cast<float *>(lut);
    if (V::f32) { if (threadIdx.x < (unsigned)LUT_SIZE) lutf[threadIdx.x] = (float)lutv; }
    else if (threadIdx.x < (unsigned)LUT_SIZE) lut[threadIdx.x] = lutv;
    __syncthreads();
    if (env_raw >= P.N) return;
    CZ_STAMP(1);
    // the compact observation's descriptor words (cz_step_device_compact): fetched here, behind the prologue's waits - a branch
    // on a late argument in front of the prologue's loads costs every launch 0.4 us - and hidden by the dynamics
    CodesPrefetch cpre;
    cpre.layout = e.layout;
    // (this fetch is spelled out at its three sites: behind a shared function - tried with and without the layout word - the code
    // variants come out with a few instructions more or fewer, and the shipped streams are kept instruction for instruction)
    if (V::desc_held) {
#pragma unroll
        for (int r = 0; r < CODES_PREFETCH; ++r) cpre.d[r] = load_desc4(P, e.layout, 256u * r + 4u * (uint32_t)lane);
    }

    const int T = V::fused ? P.T : 1;
#ifdef CZ_TIMELINE
    uint32_t tl_dbg = 0u;
#endif
    // a fused rollout over caller-supplied actions (cz_rollout_actions: [T][N][A] int32): step t's action words are loaded one
    // step ahead, so the round trip hides behind the previous step's work
    const uint32_t act_lane = ((uint32_t)env * (uint32_t)NA + (uint32_t)min(lane, NA - 1)) * 4u;
    if (V::ext_actions) av = ldg<int>(e_actions, act_lane);
#pragma nounroll
    for (int t = 0; t < T; ++t) {
        // The fused kernel re-reads its argument block every step (scalar loads that hit the constant cache): nothing of
        // it then stays live across the loop's back edge, which is what used to spill ~90 SGPRs.
        typename V::View Pt;
        if constexpr (V::fused) {
            static_assert(sizeof(Params) % 8 == 0, "copied as 64-bit words");
            typedef uint64_t __attribute__((may_alias)) word_t;
            const __attribute__((address_space(4))) word_t *src = (const __attribute__((address_space(4))) word_t *)CZ_LATE_STEP();
            word_t *dst = reinterpret_cast<word_t *>(&Pt);
#pragma unroll
            for (unsigned i = 0; i < sizeof(Params) / 8; ++i) dst[i] = src[i];
            Pt.state = e_state; Pt.actions = e_actions; Pt.lut = e_lut; Pt.N = e_N; Pt.RW = e_RW; Pt.W = e_W; Pt.H = e_H; Pt.D = e_D;
            Pt.dyn0_off = e_dyn0; Pt.dyn1_off = e_dyn1;
        } else {
            Pt = P;
        }
        if (V::desc_per_step) {
            // (a fused rollout fetches the code descriptors again at the top of every step - hidden by the step's dynamics - instead
            // of holding eight more registers across the loop: with them the kernel no longer fits four waves per SIMD)
            cpre.layout = e.layout;
#pragma unroll
            for (int r = 0; r < CODES_PREFETCH; ++r) cpre.d[r] = load_desc4(Pt, e.layout, 256u * r + 4u * (uint32_t)lane);
        }
        uint32_t acts;                                             // lane a = action of agent a
        if (!V::fused) acts = (uint32_t)av;
        else if (V::ext_actions) {
            acts = (uint32_t)av;
            // (cz_rollout_actions checks that T * N * A * 4 fits 32 bits; the last step re-reads its own row)
            av = ldg<int>(e_actions, act_lane + (uint32_t)min(t + 1, T - 1) * ((uint32_t)Pt.N * (uint32_t)NA * 4u));
        } else acts = action_hash(Pt.seed, env_global, lane & 3, Pt.step0 + (uint32_t)t, SCHEME == 3 ? 5u : 8u);
        Dirty dt{};
        StepOut o;
        step_env<OPL, CPL, NA, SCHEME, V::fused, V::lean>(Pt, block_offset<typename V::Block>(), e, cx, acts, env_global, rowv, lds, dsc, dt, o);
#ifdef CZ_TIMELINE
        tl_dbg |= o.dbg;
#endif
        CZ_STAMP(4);
        cells_dirty |= dt.cells != 0;
        objs_dirty |= (dt.touched | dt.interacted | dt.moved) != 0;
        header_dirty |= o.header;
        // ---- running return (lane a = agent a) and, at episode end only, the per-env statistics
        const double myrew = o.myrew;
        if (o.stepped) ret += myrew;
        const auto kp = CZ_LATE_STEP();
        // The statistics are a read-modify-write of words in memory (across launches: device-scope loads, write-through stores,
        // like the record).  A wave that ends an episode issues the loads here and adds / stores behind the encode: the round
        // trip (~1 us after a launch boundary) used to make exactly these waves the last ones of a launch in which nobody acts.
        uint32_t su_old = 0u;
        double sf_old = 0.0, ret_done = 0.0;
        if (CZ_RARE(V::fused, o.finished)) {
            const uint32_t *su = kp->stat_u + (size_t)env * SU_WORDS;
            const double *sf = kp->stat_f + (size_t)env * SF_WORDS;
            su_old = ldg<uint32_t>(su, ((uint32_t)lane & 15u) * 4u);
            sf_old = ldg<double>(sf, (uint32_t)(SF_SUM0 + ((uint32_t)lane & 3u)) * 8u);
            ret_done = ret;
            ret = 0.0;
        }
        // ---- outputs of this step.  One wave-uniform base pointer per array and a 32-bit per-lane offset (cz_rollout checks
        // that T * N * A * 8 fits): the `global_store v, v_off, s[base]` form, no 64-bit per-lane address arithmetic.  The
        // one-step kernels store unconditionally - the host hands them a scratch row for an array the caller does not want.
        // (ROLLOUT_ACTIONS with P.step0 & 1 - cz_set_ring_fused: the steps of an action ring fused into one launch - writes every step's
        // outputs to row `env`, like the one-step launches it stands in for; a wave's stores to one address keep their order.
        // ROLLOUT_ACTIONS_F32 has no such form: it always writes row t)
        const bool in_place = V::ext_actions && !V::f32 && (Pt.step0 & 1u) != 0u;
        const size_t row = V::fused ? ((size_t)(in_place ? 0 : t) * Pt.N + env) : (size_t)env;
        // (the compact path's descriptor words were fetched long ago; waiting for them HERE costs nothing, while behind the
        // stores below the same wait would also stand for those stores' acknowledgement - one counter for loads and stores)
        if (V::codes || V::f32) {
            if (CZ_RARE(V::fused, cpre.layout != e.layout)) {                 // a reset pass has moved the env to another layout
                cpre.layout = e.layout;
#pragma unroll
                for (int r = 0; r < CODES_PREFETCH; ++r) cpre.d[r] = load_desc4(Pt, e.layout, 256u * r + 4u * (uint32_t)lane);
            }
#pragma unroll
            for (int r = 0; r < CODES_PREFETCH; ++r) asm volatile("" :: "v"(cpre.d[r]));
        }
        {
            const uint32_t oidx = (uint32_t)row * (uint32_t)NA + (uint32_t)lane;          // [row][agent]
            double *const rewards = kp->rewards;
            uint8_t *const term = kp->term, *const trunc = kp->trunc;
            if (lane < NA) {
                if (!V::fused || rewards) stg<double>(rewards, oidx * 8u, myrew);
                if (!V::fused || term) stg<uint8_t>(term, oidx, (uint8_t)o.term);
                if (!V::fused || trunc) {
                    stg<uint8_t>(trunc, oidx, (uint8_t)o.trunc);
                    // whoever was despawned in this step is reported truncated once (cooking_env.py:344-349): a second store by
                    // those lanes, on the rare steps on which somebody leaves
                    if (o.gone && ((o.gone >> lane) & 1u)) stg<uint8_t>(trunc, oidx, (uint8_t)1);
                }
            }
        }
        if constexpr (!V::fused && !V::lean) {
            uint32_t *const marks_out = kp->marks_out;
            if (marks_out && lane < 2) stg<uint32_t>(marks_out, (2u * (uint32_t)env + (uint32_t)lane) * 4u, lane == 0 ? e.marks : e.marks_hi);   // infos["recipe_done"] of the host API
        }
        CZ_STAMP(5);
        img_objs |= (dt.touched | dt.moved) != 0;
        img_cells |= dt.cells != 0;
        if constexpr (V::f32) {
            // (choose_step takes these variants only with a float32 buffer: the rows are written unconditionally.  Fused: row t * N + env of
            // float[T][N][A][F], a 64-bit product like the float64 trajectory's, and the image is rebuilt where the step changed it)
            float *const obs_row = Pt.obs32 + (uint64_t)(uint32_t)row * (uint64_t)(uint32_t)(NA * Pt.F);
            build_image<OPL, CPL, NA>(Pt, e, cx, lds, submask, img_objs, img_cells);
            write_rows_f32<OPL, CPL, NA>(Pt, e, cx, lds, lutf, obs_row, &cpre);
            if (V::fused) { img_objs = false; img_cells = false; }
        } else if (V::lean || Pt.obs || V::codes) {
            // (env row x row length: a 32 x 32 -> 64-bit product, two scalar multiplies)
            uint8_t *const codes = V::codes ? Pt.codes + (uint64_t)(uint32_t)row * (uint64_t)(uint32_t)(NA * codes_pitch(Pt.F)) : nullptr;
            double *const obs_row = V::f64 && Pt.obs ? Pt.obs + (uint64_t)(uint32_t)row * (uint64_t)(uint32_t)(NA * Pt.F) : nullptr;
            observe<OPL, CPL, NA, V::f64, V::lean>(Pt, e, cx, lds, lut, dsc, submask, obs_row, img_objs, img_cells, codes, V::codes ? &cpre : nullptr);
            img_objs = false; img_cells = false;
        }
        if (CZ_RARE(V::fused, o.finished)) {      // (the state is still that of the finished episode: the reset is the next pass)
            uint32_t *su = kp->stat_u + (size_t)env * SU_WORDS;
            double *sf = kp->stat_f + (size_t)env * SF_WORDS;
            const uint32_t a_of = (uint32_t)lane - SU_COMPLETED0;               // lane SU_COMPLETED0 + a: recipe a completed?
            const uint32_t root = !V::lean && Pt.wide ? (((a_of < 2u ? e.marks : e.marks_hi) >> (16u * (a_of & 1u))) & 1u) : ((e.marks >> (8u * (a_of & 3u))) & 1u);
            const uint32_t inc = lane == (int)SU_EPISODES ? 1u : lane == (int)SU_LENSUM ? e.t : lane == (int)SU_TRUNC ? (uint32_t)o.trunc
                                 : lane == (int)SU_TERM ? (uint32_t)o.term : a_of < (uint32_t)NA ? root : 0u;
            if (lane < (int)SU_COMPLETED0 + NA && lane != (int)SU_STEPS) stg<uint32_t>(su, (uint32_t)lane * 4u, su_old + inc);
            if (lane < NA) stg<double>(sf, (uint32_t)(SF_SUM0 + lane) * 8u, sf_old + ret_done);
            // the env's "last finished episode" row (cz_episodes_collect; cooking_env.py:248,264,329): plain overwrites of words no
            // step reads - length, episode index, flags (bit 0 terminated, bit 1 truncated, bit 4 + a the root mark of recipe a) in
            // the counters' free words, the per-agent returns in the doubles in front of the sums
            const uint32_t roots = (uint32_t)(ballot(a_of < (uint32_t)NA && root != 0u) >> SU_COMPLETED0) & 0xFu;
            const uint32_t last = lane == (int)SU_LAST_LENGTH ? e.t : lane == (int)SU_LAST_EPISODE ? e.episode
                                  : (uint32_t)o.term | ((uint32_t)o.trunc << 1) | (roots << 4);
            if (lane >= (int)SU_LAST_LENGTH && lane <= (int)SU_LAST_FLAGS) stg<uint32_t>(su, (uint32_t)lane * 4u, last);
            if (lane < NA) stg<double>(sf, (uint32_t)(SF_LAST0 + lane) * 8u, ret_done);
        }
        CZ_STAMP(6);
    }
    store_env(P, e, cx, rec, cells_dirty, objs_dirty, header_dirty);
    if (lane < NA) stg<double>(retp, (uint32_t)lane * 8u, ret);
    CZ_STAMP(7);
#ifdef CZ_TIMELINE
    {
        // word 0: entry time (low 32 bits) | HW_ID << 32 (wave, SIMD, CU, SH, SE);  word 1: exit time | XCC_ID << 32
        const uint64_t tl_out = wall_clock64();
        const uint32_t hw_id = __builtin_amdgcn_s_getreg(4 | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));
        unsigned long long *const tl = CZ_LATE_STEP()->timeline;
        if (tl && lane == 0) {
            typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
            ull2 v;
            v.x = (tl_in & 0xFFFFFFFFull) | ((unsigned long long)(hw_id & 0xFFFFu) << 32) | ((unsigned long long)tl_dbg << 48);
            v.y = (tl_out & 0xFFFFFFFFull) | ((unsigned long long)(xcc & 15u) << 32) | (((tl_seen - tl_in) & 0xFFFFFFFull) << 36);
            *reinterpret_cast<ull2 *>(tl + 2 * (size_t)env) = v;
        }
    }
#endif
}

// (experiment switch: occupancy target of the one-step kernels of the small and the middle instance.  All of them reach six
// waves per SIMD by themselves except the middle instance with four agents - config 5's kernel: 82 vector registers, four
// waves - and forcing that one to six (80 registers, 3 spilled) changed nothing: 195 against 197 M env-steps/s,
// profiles/r03/wpe_ab.txt)
#ifdef CZ_STEP_MIN_WPE
#define CZ_STEP_ATTR __attribute__((amdgpu_waves_per_eu((!StepTraits<FUSED>::fused && OPL <= 2) ? CZ_STEP_MIN_WPE : 1)))
#else
#define CZ_STEP_ATTR
#endif
template <int OPL, int CPL, int NA, int SCHEME, int FUSED /* a StepMode */>
__global__ __launch_bounds__(64 * envs_per_wg<CPL>()) CZ_STEP_ATTR void k_step(uint32_t *e_state, const int32_t *e_actions, const double *e_lut, int32_t e_N,
                                                          int32_t e_RW, int32_t e_W, int32_t e_H, int32_t e_D, int32_t e_dyn0,
                                                          int32_t e_dyn1, const Params P0) {
    step_kernel<OPL, CPL, NA, SCHEME, StepTraits<FUSED>>(e_state, e_actions, e_lut, e_N, e_RW, e_W, e_H, e_D, e_dyn0, e_dyn1, P0);
}
// the lean one-step kernel (see StepTraits; small instance only: launchers_small)
template <int OPL, int CPL, int NA, int SCHEME>
__global__ __launch_bounds__(64 * envs_per_wg<CPL>()) void k_step_lean(uint32_t *e_state, const int32_t *e_actions, const double *e_lut, int32_t e_N,
                                                                       int32_t e_RW, int32_t e_W, int32_t e_H, int32_t e_D, int32_t e_dyn0,
                                                                       int32_t e_dyn1, const LeanParams P0) {
    step_kernel<OPL, CPL, NA, SCHEME, StepTraits<STEP, true>>(e_state, e_actions, e_lut, e_N, e_RW, e_W, e_H, e_D, e_dyn0, e_dyn1, P0);
}
// ... with the handle's recipe count, end condition and walk_touches as template arguments (LeanCfgTraits; the combinations that
// exist: CZ_LEAN_CFGS below)
template <int OPL, int CPL, int NA, int SCHEME, int R, int END_ALL, int WALK_TOUCHES>
__global__ __launch_bounds__(64 * envs_per_wg<CPL>()) void k_step_lean_cfg(uint32_t *e_state, const int32_t *e_actions, const double *e_lut, int32_t e_N,
                                                                           int32_t e_RW, int32_t e_W, int32_t e_H, int32_t e_D, int32_t e_dyn0,
                                                                           int32_t e_dyn1, const LeanParams P0) {
    step_kernel<OPL, CPL, NA, SCHEME, LeanCfgTraits<R, END_ALL, WALK_TOUCHES>>(e_state, e_actions, e_lut, e_N, e_RW, e_W, e_H, e_D, e_dyn0, e_dyn1, P0);
}
// ---- what the five off-step kernels below share; nothing here is inlined by a step kernel ----
// the float32 table: every entry of the quotient table rounded to nearest even, staged by one wavefront
__device__ __forceinline__ void init_lut_f32(const Params &P, float *lutf, int lane) {
    for (int i = lane; i < LUT_SIZE; i += 64) lutf[i] = (float)ldg<double>(P.lut, (uint32_t)i * 8u);
}
// row `i` of a buffer with `pitch` elements per row; no buffer: null
template <class T>
__device__ __forceinline__ T *row_of(T *base, size_t i, size_t pitch) { return base ? base + i * pitch : nullptr; }
// The rows of one env in whichever forms were asked for: `obs`, `obs32` and `codes` are the buffers, any of them null, and `row` is
// this env's row in them (its pointers are taken where they are used: taken by the caller, their null checks stood in front of the
// subtrahend-mask load and on the path of a call without rows - 3 us of k_restore_where's 27 at 65 536 envs, profiles/r18/README.md).
// The float64 table is staged only when float64 rows are wanted, the float32 one only for float32 rows - which are gathered from the
// image observe has built, or from one built here when neither other form is wanted.  A kernel that cannot write a form passes a
// literal null for it and for its table: the branch folds away, and the kernel carries no __shared__ table for that form.
template <int OPL, int CPL, int NA>
__device__ __forceinline__ void write_forms(const Params &P, const Env<OPL, CPL, NA> &e, const Ctx &cx, Lds<CPL> &lds, double *lut, float *lutf,
                                            double *obs, float *obs32, uint8_t *codes, size_t row) {
    const uint32_t submask = load_submask(P, cx.lane);
    if (obs || codes) {
        if (obs) init_lut(P, lut, cx.lane, 64);
        uint32_t dsc[OBS_CHUNK];
        load_desc(P, e.layout, 0, cx.lane, dsc);
        observe(P, e, cx, lds, lut, dsc, submask, row_of(obs, row, (size_t)NA * P.F), true, true, row_of(codes, row, (size_t)NA * codes_pitch(P.F)));
    }
    if (obs32) {
        init_lut_f32(P, lutf, cx.lane);
        if (!(obs || codes)) build_image<OPL, CPL, NA>(P, e, cx, lds, submask, true, true);      // (else observe has built it)
        write_rows_f32<OPL, CPL, NA>(P, e, cx, lds, lutf, obs32 + row * NA * P.F, nullptr);
    }
}
// A fresh episode on layout `lay` (reset(), cooking_env.py:178-210): the layout's initial record with t and the status word zeroed
// (despawn on: everybody present, grace running), every recipe's marks from scratch, stored to `rec`, and the running returns zeroed.
// (The auto-reset pass of step_env keeps a copy of its own: sharing this one would change the step kernels.)
template <int OPL, int CPL, int NA>
__device__ __forceinline__ void begin_episode(const Params &P, Env<OPL, CPL, NA> &e, const Ctx &cx, Lds<CPL> &lds, uint32_t *rec, uint32_t lay,
                                              uint32_t episode, uint32_t recipes, uint32_t pool) {
    load_env(P, e, cx, P.lay_init + (size_t)lay * P.RW);
    e.t = 0; e.layout = lay; e.status = 0; e.episode = episode; e.recipes = recipes; e.pool = pool;
    if (P.auto_reset & 2)
        e.status = spawn_initial_status(rfl(reinterpret_cast<const SpawnCfg *>(reinterpret_cast<const char *>(P.lut) + SPAWN_CFG_OFFSET)->grace_period), NA);
    uint32_t rowv = load_recipe_rows(P, e.recipes, cx.lane);
    all_marks(P, e, cx, rowv, lds);
    store_env(P, e, cx, rec, true, true);
    if (cx.lane < MAX_AGENTS) reinterpret_cast<double *>(rec + RET_WORD0)[cx.lane] = 0.0;
}

// reset(): cooking_env.py:178-210 for envs [env_begin, env_begin + count)
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_reset(const Params P, int64_t env_begin, const int32_t *__restrict__ layout_ids,
                                              const uint32_t *__restrict__ recipe_words, const uint32_t *__restrict__ pool_words,
                                              double *obs_out) {
    __shared__ Lds<CPL> lds;
    __shared__ double lut[LUT_SIZE];
    const int i = blockIdx.x;
    Ctx cx{P.W, P.H, P.D, P.W * P.H, (int)threadIdx.x};
    init_lds<CPL>(P, cx, lds);
    Env<OPL, CPL, NA> e;
    uint32_t *rec = P.state + (size_t)(env_begin + i) * P.RW;
    const uint32_t old_episode = rfl(rec[W_EPISODE]);
    begin_episode(P, e, cx, lds, rec, rfl((uint32_t)layout_ids[i]), old_episode, rfl(recipe_words[i]), rfl(pool_words[i]));
    write_forms(P, e, cx, lds, lut, nullptr, obs_out, nullptr, nullptr, (size_t)i);
}

// observe() only (after cz_set_state)
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_observe(const Params P, int64_t env_begin, double *obs_out, uint8_t *codes_out) {
    __shared__ Lds<CPL> lds;
    __shared__ double lut[LUT_SIZE];
    const int i = blockIdx.x;
    Ctx cx{P.W, P.H, P.D, P.W * P.H, (int)threadIdx.x};
    init_lds<CPL>(P, cx, lds);
    Env<OPL, CPL, NA> e;
    load_env(P, e, cx, P.state + (size_t)(env_begin + i) * P.RW);
    write_forms(P, e, cx, lds, lut, nullptr, obs_out, nullptr, codes_out, (size_t)i);
}

// ... as float32 rows float[count][A][F] (cz_observe_device_f32): the form of STEP_F32, for the first observation after cz_reset /
// cz_set_state.  A kernel of its own next to k_observe: each carries one table in LDS, and both are write_forms with the other
// forms literally null.
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_observe_f32(const Params P, int64_t env_begin, float *obs_out) {
    __shared__ Lds<CPL> lds;
    __shared__ float lutf[LUT_SIZE];
    const int i = blockIdx.x;
    Ctx cx{P.W, P.H, P.D, P.W * P.H, (int)threadIdx.x};
    init_lds<CPL>(P, cx, lds);
    Env<OPL, CPL, NA> e;
    load_env(P, e, cx, P.state + (size_t)(env_begin + i) * P.RW);
    write_forms(P, e, cx, lds, nullptr, lutf, nullptr, obs_out, nullptr, (size_t)i);
}

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

// reset() of cooking_env.py:178-210 for CHOSEN envs of the whole batch, everything in device memory (cz_reset_device): env e is chosen
// when mask[e] != 0 or, without a mask, when its status word has the done bit - what the auto-reset pass of step_env does to such an
// env, without spending a step.  One wavefront per env and workgroup: the wave of an env that is not chosen leaves behind one load,
// before anything is staged, and strands no barrier.  A chosen env: episode + 1; the layout is layout_ids[e] when that is >= 0, else
// the keyed draw of the auto-reset pass (same control words); an explicit id >= L is refused - the env stays as it was, `refused`
// counts it.  Then k_reset's work (begin_episode) - recipes and pool word are the old record's - and write_forms' rows, in
// buffers laid out for the whole batch: rows e of the chosen envs only.  P.wt is 0 here (plain stores).
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_reset_where(const Params P, const uint8_t *__restrict__ mask, const int32_t *__restrict__ layout_ids,
                                                    double *obs_out, float *obs32_out, uint8_t *codes_out, unsigned long long *refused) {
    __shared__ Lds<CPL> lds;
    __shared__ double lut[LUT_SIZE];
    __shared__ float lutf[LUT_SIZE];
    const uint32_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    uint32_t *rec = P.state + (size_t)env * P.RW;
    uint32_t old_status = 0u;
    if (mask) {
        if (rfl((uint32_t)mask[env]) == 0u) return;
        old_status = rfl(rec[W_STATUS]);
    } else {
        old_status = rfl(rec[W_STATUS]);
        if (!(old_status & ST_DONE)) return;
    }
    const int32_t want = layout_ids ? (int32_t)rfl((uint32_t)layout_ids[env]) : -1;
    if (want >= P.L) {                                               // refused: nothing of the env or of its rows is touched
        if (lane == 0) atomicAdd(refused, 1ull);
        return;
    }
    // the old record's words, read before anything overwrites them
    const uint32_t old_t = rfl(rec[W_T]), episode = rfl(rec[W_EPISODE]) + 1u, recipes = rfl(rec[W_RECIPES]), pool = rfl(rec[W_POOL]);
    // an episode cut short: its steps stay counted as env-steps (k_count_aborted of cz_reset); a finished one was counted when it ended
    if (!(old_status & ST_DONE) && lane == 0) P.stat_u[(size_t)env * SU_WORDS + SU_STEPS] += old_t;
    uint32_t lay = (uint32_t)want;
    if (want < 0) {
        const uint32_t *ctl = P.lay_init - LAY_CTL_WORDS;
        lay = next_layout(P.env_id_base + (int64_t)env, episode, pool, (uint32_t)P.L, rfl(ctl[LC_GROUPS]), rfl(ctl[LC_ACTIVE]));
    }
    Ctx cx{P.W, P.H, P.D, P.W * P.H, lane};
    init_lds<CPL>(P, cx, lds);
    Env<OPL, CPL, NA> e;
    begin_episode(P, e, cx, lds, rec, lay, episode, recipes, pool);
    write_forms(P, e, cx, lds, lut, lutf, obs_out, obs32_out, codes_out, env);
}

// A record enters the batch (cz_restore_device): env e becomes row slot[e] of the caller's archive, word for word (no slot array:
// row e; the host has checked capacity >= N); any number of envs may name one row.  One wavefront per env and workgroup: the wave of
// an env whose slot is negative leaves behind one load, before anything is staged, and strands no barrier.  The row is read with
// per-lane loads - the raw words (lane l: words l, l + 64, ...) and load_env's typed view of them, neither of which uses a word of
// the row as an index - and then checked by the functions cz_set_state checks a record with on the host: record_header_faults and,
// in a ballot over the lanes that hold the slots, slot_dead_but_tagged (cz_device.h).  A slot >= capacity or a failing row is refused: the env and its rows stay as they were, `refused` counts it.  Otherwise the raw
// words go to the env's record (byte-exact: store_env plays no part), lane 0 corrects SU_STEPS - plus the old record's t when that
// episode was running (k_count_aborted's rule: its steps stay counted), minus the new record's t when this one is (k_stats_clear's
// rule: steps that arrive already taken are not this handle's) - and the rows of whichever forms were asked for are written as
// k_reset_where writes them, from the env load_env made of the row: the same words as the new record, but read from memory this
// kernel does not write (load_env's header load goes through the scalar cache, which a store of this wave does not update).
// The archive must not overlap the handle's own records.  P.wt is 0 here (plain stores).
template <int OPL, int CPL>
constexpr int record_chunks() { return ((CELL_WORD0 + 16 * CPL + 128 * OPL + 15) / 16 * 16 + 63) / 64; }   // 64-word chunks that cover the largest RW of the instance
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_restore_where(const Params P, const int32_t *__restrict__ slot, const uint32_t *__restrict__ records,
                                                      int64_t capacity, uint32_t n_recipes, double *obs_out, float *obs32_out,
                                                      uint8_t *codes_out, unsigned long long *refused) {
    __shared__ Lds<CPL> lds;
    __shared__ double lut[LUT_SIZE];
    __shared__ float lutf[LUT_SIZE];
    constexpr int NW = record_chunks<OPL, CPL>();
    const uint32_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    int64_t s = (int64_t)env;
    if (slot) {
        const int32_t v = (int32_t)rfl((uint32_t)slot[env]);
        if (v < 0) return;
        s = v;
    }
    if (s >= capacity) {                                             // refused: nothing of the env or of its rows is touched
        if (lane == 0) atomicAdd(refused, 1ull);
        return;
    }
    const uint32_t *row = records + (size_t)s * P.RW;
    uint32_t *rec = P.state + (size_t)env * P.RW;
    const uint32_t RW = (uint32_t)P.RW;
    uint32_t raw[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) raw[k] = ldg<uint32_t>(row, min((uint32_t)lane + 64u * k, RW - 1u) * 4u);   // clamped, like load_env's
    Ctx cx{P.W, P.H, P.D, P.W * P.H, lane};
    Env<OPL, CPL, NA> e;
    load_env(P, e, cx, row);
    // the record rules of cz_set_state (cz_device.h), before any of these words is an index
    bool tagged_dead = false;
#pragma unroll
    for (int k = 0; k < OPL; ++k) tagged_dead = tagged_dead || slot_dead_but_tagged(e.d0[k], e.d1[k]);   // (lanes past D hold zeros)
    if (record_header_faults(e.layout, e.recipes, e.pool, (uint32_t)P.L, P.R, n_recipes) || ballot(tagged_dead) != 0ull) {
        if (lane == 0) atomicAdd(refused, 1ull);
        return;
    }
    // the old record's words, read before anything overwrites them
    const uint32_t old_status = rfl(rec[W_STATUS]), old_t = rfl(rec[W_T]);
    const uint32_t correction = ((old_status & ST_DONE) ? 0u : old_t) - ((e.status & ST_DONE) ? 0u : e.t);
    if (lane == 0) P.stat_u[(size_t)env * SU_WORDS + SU_STEPS] += correction;       // a signed word (k_stats_chains)
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const uint32_t w = (uint32_t)lane + 64u * k;
        if (w < RW) stg<uint32_t>(rec, w * 4u, raw[k]);
    }
    init_lds<CPL>(P, cx, lds);
    write_forms(P, e, cx, lds, lut, lutf, obs_out, obs32_out, codes_out, env);
}

// launchers exported by each instantiation unit
// cfg: with `lean`, the row of CZ_LEAN_CFGS whose k_step_lean_cfg the launch takes, or -1: k_step_lean
struct StepChoice { StepMode mode; bool lean; int cfg; };       // which variant a launch takes (choose_step, cz_api.hip)
// The k_step_lean_cfg kernels of the small instance: X(agents, action scheme, recipes, end_all, walk_touches), nine kernels, all under
// scheme3.  Two agents - the headline workload and BASELINE configs 3 and 4 are (2, 3, 2, 0, 0) - with every recipe count a handle of
// two agents can have (cz_create: agents <= recipes <= 4) and both end conditions; one recipe means one agent; walk_touches = 1 where
// a handle cannot avoid it: more than two agents (cz_load_recipes).
#define CZ_LEAN_CFGS(X) \
    X(1, 3, 1, 0, 0) X(1, 3, 1, 1, 0) X(2, 3, 2, 0, 0) X(2, 3, 2, 1, 0) X(2, 3, 3, 0, 0) X(2, 3, 3, 1, 0) X(2, 3, 4, 0, 0) X(2, 3, 4, 1, 0) \
    X(3, 3, 3, 0, 1)
struct LeanCfg { int A, scheme, R, end_all, walk_touches; };
constexpr LeanCfg LEAN_CFGS[] = {
#define CZ_X(a, s, r, ea, wt) {a, s, r, ea, wt},
    CZ_LEAN_CFGS(CZ_X)
#undef CZ_X
};
constexpr int N_LEAN_CFGS = (int)(sizeof LEAN_CFGS / sizeof LEAN_CFGS[0]);
static_assert(N_LEAN_CFGS <= 16, "build time: each row is one more kernel of the small instance");
// the row a handle's settings select, or -1
inline int lean_cfg_of(const Params &P) {
    for (int i = 0; i < N_LEAN_CFGS; ++i) {
        const LeanCfg &c = LEAN_CFGS[i];
        if (P.A == c.A && P.scheme == c.scheme && P.R == c.R && P.end_all == c.end_all && P.walk_touches == c.walk_touches) return i;
    }
    return -1;
}
// the lean block of a launch (choose_step has checked that everything it leaves out is off)
inline LeanParams lean_block_of(const Params &P) {
    LeanParams B{};
    B.recipes = P.recipes; B.lay_desc = P.lay_desc; B.L = P.L; B.F = P.F; B.max_steps = P.max_steps; B.auto_reset = P.auto_reset;
    B.reward_idle = P.reward_idle; B.rewards = P.rewards; B.term = P.term; B.trunc = P.trunc; B.obs = P.obs;
    B.settings = (uint32_t)P.R | ((uint32_t)(P.end_all != 0) << 8) | ((uint32_t)(P.walk_touches != 0) << 16);
    B.stat_u = P.stat_u; B.stat_f = P.stat_f; B.lay_init = P.lay_init; B.env_id_base = P.env_id_base;
    B.node_reward = P.node_reward; B.recipe_reward = P.recipe_reward; B.recipe_penalty = P.recipe_penalty; B.time_penalty_step = P.time_penalty_step;
#ifdef CZ_PROFILE
    B.stamps = P.stamps;
#endif
#ifdef CZ_TIMELINE
    B.timeline = P.timeline;
#endif
    return B;
}
struct Launchers {
    // lean: k_step_lean (mode STEP, and only where has_lean); otherwise k_step<..., mode>.  Fused modes run P.T steps per launch
    hipError_t (*step)(const Params &, hipStream_t, StepChoice);
    hipError_t (*reset)(const Params &, hipStream_t, int64_t, int, const int32_t *, const uint32_t *, const uint32_t *, double *);
    hipError_t (*observe)(const Params &, hipStream_t, int64_t, int, double *, uint8_t *);
    bool has_lean;             // the instance carries the k_step_lean kernels
    hipError_t (*observe_f32)(const Params &, hipStream_t, int64_t, int, float *);
    // k_reset_where over all P.N envs: mask, layout ids, float64 rows, float32 rows, codes, refused counter
    hipError_t (*reset_where)(const Params &, hipStream_t, const uint8_t *, const int32_t *, double *, float *, uint8_t *, unsigned long long *);
    // k_restore_where over all P.N envs: slots, archive, its rows, recipes in the table, float64 rows, float32 rows, codes, refused counter
    hipError_t (*restore_where)(const Params &, hipStream_t, const int32_t *, const uint32_t *, int64_t, uint32_t, double *, float *, uint8_t *,
                                unsigned long long *);
    // k_observe_grid: first env, count, extended, then bits, grid8, grid32, agent_xy (any may be null)
    hipError_t (*observe_grid)(const Params &, hipStream_t, int64_t, int, int32_t, uint32_t *, uint8_t *, float *, int32_t *);
    // k_navigate: first env, count, T, flags, targets, then actions, steps, field (any may be null)
    hipError_t (*navigate)(const Params &, hipStream_t, int64_t, int, int32_t, uint32_t, const int32_t *, int32_t *, int32_t *, uint16_t *);
    // k_partner: count, then its argument block
    hipError_t (*partner)(const Params &, hipStream_t, int, const PartnerArgs &);
    // k_action_effects: count envs (one workgroup per env and agent), then its argument block; by agent count and action scheme
    hipError_t (*action_effects)(const Params &, hipStream_t, int, const EffectsArgs &);
    // k_render: count envs (one workgroup per env and row of cells), then its argument block
    hipError_t (*render)(const Params &, hipStream_t, int, const RenderArgs &);
};

// the run-time agent count (1..4; anything else: 4) and action scheme (3; anything else: 1) as template arguments of f's call
template <class F>
inline hipError_t with_agents(int A, F &&f) {
    switch (A) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
    }
}
template <class F>
inline hipError_t with_scheme(int scheme, F &&f) {
    return scheme == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 1>{});
}
// one launch of a step kernel: one wavefront per env, the leading scalar arguments spelled out for the preload (Early)
// (`block`: the kernel's by-value block - P itself, or its lean block)
template <int CPL, class K, class B>
inline hipError_t launch_step_kernel(K kernel, const Params &P, const B &block_arg, hipStream_t st) {
    constexpr int EPW = envs_per_wg<CPL>();
    const dim3 grid((unsigned)((P.N + EPW - 1) / EPW)), block(64 * EPW);
    const Early E = early_of(P);
    hipLaunchKernelGGL(kernel, grid, block, 0, st, E.state, E.actions, E.lut, E.N, E.RW, E.W, E.H, E.D, E.dyn0_off, E.dyn1_off, block_arg);
    return hipGetLastError();
}
template <int CPL, class K>
inline hipError_t launch_step_kernel(K kernel, const Params &P, hipStream_t st) { return launch_step_kernel<CPL>(kernel, P, P, st); }

template <int OPL, int CPL, bool HAS_LEAN = false>
struct Inst {
    static hipError_t step(const Params &P, hipStream_t st, StepChoice c) {
        if constexpr (HAS_LEAN) {
            if (c.lean && c.cfg >= 0) {
                if (c.cfg != lean_cfg_of(P)) return hipErrorInvalidValue;
                const LeanParams B = lean_block_of(P);
                int row = 0;
#define CZ_X(a, s, r, ea, wt) if (c.cfg == row++) return launch_step_kernel<CPL>(k_step_lean_cfg<OPL, CPL, a, s, r, ea, wt>, P, B, st);
                CZ_LEAN_CFGS(CZ_X)
#undef CZ_X
                return hipErrorInvalidValue;
            }
        }
        return with_agents(P.A, [&](auto na) {
            return with_scheme(P.scheme, [&](auto scheme) {
                constexpr int NA = decltype(na)::value, S = decltype(scheme)::value;
                if (c.lean) {
                    if constexpr (HAS_LEAN) return launch_step_kernel<CPL>(k_step_lean<OPL, CPL, NA, S>, P, lean_block_of(P), st);
                    return hipErrorInvalidValue;
                }
                switch (c.mode) {
                case STEP: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, STEP>, P, st);
                case ROLLOUT: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, ROLLOUT>, P, st);
                case ROLLOUT_ACTIONS: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, ROLLOUT_ACTIONS>, P, st);
                case STEP_CODES: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, STEP_CODES>, P, st);
                case ROLLOUT_CODES: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, ROLLOUT_CODES>, P, st);
                case ROLLOUT_CODES_ONLY: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, ROLLOUT_CODES_ONLY>, P, st);
                case STEP_F32: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, STEP_F32>, P, st);
                case ROLLOUT_F32: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, ROLLOUT_F32>, P, st);
                case ROLLOUT_ACTIONS_F32: return launch_step_kernel<CPL>(k_step<OPL, CPL, NA, S, ROLLOUT_ACTIONS_F32>, P, st);
                }
                return hipErrorInvalidValue;
            });
        });
    }
    // one launch of an off-step kernel K<OPL, CPL, NA>, one wavefront per env: `envs` workgroups, Params first
#define CZ_LAUNCH_PER_ENV(K, envs, ...)                                                                                             \
    with_agents(P.A, [&](auto na) {                                                                                                 \
        hipLaunchKernelGGL((K<OPL, CPL, decltype(na)::value>), dim3((unsigned)(envs)), dim3(64), 0, st, P, __VA_ARGS__);            \
        return hipGetLastError();                                                                                                   \
    })
    static hipError_t reset(const Params &P, hipStream_t st, int64_t b, int n, const int32_t *lay, const uint32_t *rec,
                            const uint32_t *pool, double *obs) {
        return CZ_LAUNCH_PER_ENV(k_reset, n, b, lay, rec, pool, obs);
    }
    static hipError_t observe(const Params &P, hipStream_t st, int64_t b, int n, double *obs, uint8_t *codes) {
        return CZ_LAUNCH_PER_ENV(k_observe, n, b, obs, codes);
    }
    static hipError_t observe_f32(const Params &P, hipStream_t st, int64_t b, int n, float *obs) {
        return CZ_LAUNCH_PER_ENV(k_observe_f32, n, b, obs);
    }
    static hipError_t reset_where(const Params &P, hipStream_t st, const uint8_t *mask, const int32_t *lay, double *obs, float *obs32,
                                  uint8_t *codes, unsigned long long *refused) {
        return CZ_LAUNCH_PER_ENV(k_reset_where, P.N, mask, lay, obs, obs32, codes, refused);
    }
    static hipError_t restore_where(const Params &P, hipStream_t st, const int32_t *slot, const uint32_t *records, int64_t capacity,
                                    uint32_t n_recipes, double *obs, float *obs32, uint8_t *codes, unsigned long long *refused) {
        return CZ_LAUNCH_PER_ENV(k_restore_where, P.N, slot, records, capacity, n_recipes, obs, obs32, codes, refused);
    }
    static hipError_t observe_grid(const Params &P, hipStream_t st, int64_t b, int n, int32_t extended, uint32_t *bits, uint8_t *grid8,
                                   float *grid32, int32_t *agent_xy) {
        return CZ_LAUNCH_PER_ENV(k_observe_grid, n, b, extended, bits, grid8, grid32, agent_xy);
    }
    static hipError_t navigate(const Params &P, hipStream_t st, int64_t b, int n, int32_t T, uint32_t flags, const int32_t *target,
                               int32_t *action, int32_t *steps, uint16_t *field) {
        return CZ_LAUNCH_PER_ENV(k_navigate, n, b, T, flags, target, action, steps, field);
    }
    static hipError_t partner(const Params &P, hipStream_t st, int n, const PartnerArgs &G) { return CZ_LAUNCH_PER_ENV(k_partner, n, G); }
    static hipError_t action_effects(const Params &P, hipStream_t st, int n, const EffectsArgs &G) {
        return with_agents(P.A, [&](auto na) {
            return with_scheme(P.scheme, [&](auto scheme) {
                constexpr int NA = decltype(na)::value, S = decltype(scheme)::value;
                hipLaunchKernelGGL((k_action_effects<OPL, CPL, NA, S>), dim3((unsigned)n * (unsigned)NA), dim3(64), 0, st, P, G);
                return hipGetLastError();
            });
        });
    }
    static hipError_t render(const Params &P, hipStream_t st, int n, const RenderArgs &G) {
        return with_agents(P.A, [&](auto na) {
            hipLaunchKernelGGL((k_render<OPL, CPL, decltype(na)::value>), dim3((unsigned)n * (unsigned)P.H, (G.P + RENDER_BAND - 1u) / RENDER_BAND), dim3(RENDER_THREADS), 0, st,
                               P, G);
            return hipGetLastError();
        });
    }
#undef CZ_LAUNCH_PER_ENV
    static Launchers launchers() {
        return Launchers{&step, &reset, &observe, HAS_LEAN, &observe_f32, &reset_where, &restore_where, &observe_grid, &navigate, &partner, &action_effects,
                         &render};
    }
};

Launchers launchers_small();   // D <= 64 slots, W*H <= 64 cells
Launchers launchers_large();   // D <= 128 slots, W*H <= 256 cells
Launchers launchers_huge();    // D <= 255 slots, W*H <= 1024 cells

}  // namespace cz
