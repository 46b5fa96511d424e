// cz_offstep.h -- the kernels that begin or restore an episode or write observation rows outside a step: k_reset, k_observe,
// k_observe_f32, k_reset_where and k_restore_where, and what they share (init_lut_f32, row_of, write_forms, begin_episode); and
// k_set_tasks, which gives an env other recipes on the world it has.
// Nothing here is inlined by a step kernel.
#pragma once
#include "cz_kernels.h"

namespace cz {

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

// The row of a K-row task list that env `env_global` plays in episode `episode` (cooking_zoo_amd/tasks.py task_draw): the keyed
// stream of the spawn code at t = 0 under an agent key of its own (spawn draws: agents 0..3, the layout generator: 0x100)
constexpr uint32_t TASK_KEY = 0x200u;
__host__ __device__ inline uint32_t task_draw(uint64_t seed, int64_t env_global, uint32_t episode, uint32_t K) {
    const uint32_t k = (uint32_t)(spawn_uniform(seed, (uint64_t)env_global, (uint64_t)episode << 32, TASK_KEY, 0u) * (double)K);
    return k < K ? k : K - 1u;
}

// New recipes for CHOSEN envs of the whole batch, everything in device memory (cz_set_tasks_device; definition:
// cooking_zoo_amd/tasks.py host_set_tasks): lines 197-201 of the reference's reset() applied to fresh graphs of other names on
// the env's current world.  Env e is chosen when mask[e] != 0 or, without a mask, when its record has t == 0 (the start of an
// episode).  One wavefront per env and workgroup: the wave of an env that is not chosen leaves behind one load, before anything
// is staged.  The new ids: row e of `ids` (4 bytes per env) or, without it, row task_draw(seed, global env id, the record's
// episode, K) of `list` - an index below K by construction.  The bytes of slots >= R are forced to 0xFF; a byte >= n_recipes in
// one of the first R slots refuses the env BEFORE any of them is an index: it stays word for word as it was, `refused` counts it.
// Otherwise every recipe's marks are evaluated from scratch (all_marks) and the header words that change are stored: the recipe
// ids, the marks and, for wide tables, word 7.  No cell, no object, no status word, no statistics.
template <int OPL, int CPL, int NA>
__global__ __launch_bounds__(64) void k_set_tasks(const Params P, const uint8_t *__restrict__ mask, const uint32_t *__restrict__ ids,
                                                  const uint32_t *__restrict__ list, uint32_t K, uint64_t seed, uint32_t n_recipes,
                                                  unsigned long long *refused) {
    __shared__ Lds<CPL> lds;
    const uint32_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    uint32_t *rec = P.state + (size_t)env * P.RW;
    if (mask) {
        if (rfl((uint32_t)mask[env]) == 0u) return;
    } else {
        if (rfl(rec[W_T]) != 0u) return;
    }
    uint32_t want;
    if (ids) want = rfl(ids[env]);
    else want = rfl(list[task_draw(seed, P.env_id_base + (int64_t)env, rfl(rec[W_EPISODE]), K)]);
    bool bad = false;
    for (int r = 0; r < MAX_AGENTS; ++r) {
        if (r >= P.R) want |= 0xFFu << (8 * r);
        else if (((want >> (8 * r)) & 0xFFu) >= n_recipes) bad = true;
    }
    if (bad) {                                                       // refused: nothing of the env is touched
        if (lane == 0) atomicAdd(refused, 1ull);
        return;
    }
    Ctx cx{P.W, P.H, P.D, P.W * P.H, lane};
    Env<OPL, CPL, NA> e;
    load_env(P, e, cx, rec);
    e.recipes = want;
    const uint32_t rowv = load_recipe_rows(P, e.recipes, lane);
    all_marks(P, e, cx, rowv, lds);
    // a header-only store (store_env's header path also writes t, layout, status, episode, the pool word and the agents)
    uint32_t h = 0;
    h = wrl(e.marks, W_MARKS, h);
    h = wrl(e.recipes, W_RECIPES, h);
    h = wrl(e.marks_hi, W_MARKS_HI, h);
    const uint32_t ul = (uint32_t)lane;
    if (ul == W_MARKS || ul == W_RECIPES || (P.wide && ul == W_MARKS_HI)) stg<uint32_t>(rec, ul * 4u, h);
}

}  // namespace cz
