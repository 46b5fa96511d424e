// cz_api.hip -- C-ABI (include/cookingzoo.h) of the MI355X-native CookingZoo step path: handle, tables, launches,
// statistics, RCCL.  The kernels live in cz_kernels.h / cz_offstep.h / cz_query.h / cz_device.h (one wavefront per env instance) and are
// instantiated in cz_inst_small.hip / cz_inst_large.hip.  gfx950 only.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <string>
#include <vector>

#include "../../include/cookingzoo.h"
#include "cz_launch.h"
#include "cz_generate.h"
#include "cz_owned.h"

using namespace cz;

// Deterministic reduction of the per-env statistics into one cz_stats, in two launches.
// env_steps = finished-episode lengths + steps of the episode in flight + the signed correction word SU_STEPS
// (steps of episodes aborted by cz_reset, minus what was in flight at cz_reset_stats).
// Summation order (fixed, independent of the grid): 256 chains, chain c adds envs c, c + 256, c + 512, ... one after
// the other; the 256 chain sums are then combined by a fixed binary tree.  Stage 1 spreads the chains over 64
// single-wave workgroups (4 chains each, 16 lanes per chain: lane j of a chain owns output column j), so the records
// are pulled in by 64 CUs instead of one; stage 2 is the tree.  Integer columns are exact in any order; the float64
// columns are bitwise reproducible because the order never changes.
constexpr int STAT_CHAINS = 256, STAT_COLS = 13;      // columns: 9 integer sums (u64), 4 return sums (f64)
__global__ __launch_bounds__(64) void k_stats_chains(const uint32_t *__restrict__ su, const double *__restrict__ sf,
                                                     const uint32_t *__restrict__ state, int RW, int N,
                                                     unsigned long long *__restrict__ part /* [256][16] */) {
    const int chain = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 4), col = (int)threadIdx.x & 15;
    // which word of the per-env counters this lane's column sums (branch-free loop body: every load of a batch of envs is
    // issued before anything is added, so the chain pays one memory round trip per batch, not per env)
    const int widx = col == 0 ? (int)SU_STEPS : col == 1 ? (int)SU_EPISODES : col == 2 ? (int)SU_LENSUM : col == 3 ? (int)SU_TRUNC
                   : col == 4 ? (int)SU_TERM : col < 9 ? (int)SU_COMPLETED0 + col - 5 : 0;
    const int fidx = (col >= 9 && col < STAT_COLS) ? (int)SF_SUM0 + col - 9 : (int)SF_SUM0;
    unsigned long long acc = 0;
    double ret = 0.0;
    constexpr int B = 8;
    for (int e0 = chain; e0 < N; e0 += STAT_CHAINS * B) {
        uint32_t a[B], len[B], st[B], t[B];
        double f[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const int e = min(e0 + j * STAT_CHAINS, N - 1);                    // clamped: the value is dropped below
            const uint32_t *p = su + (size_t)e * SU_WORDS;
            const uint32_t *rec = state + (size_t)e * RW;
            a[j] = p[widx]; len[j] = p[SU_LENSUM]; st[j] = rec[W_STATUS]; t[j] = rec[W_T];
            f[j] = sf[(size_t)e * SF_WORDS + fidx];
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
            if (e0 + j * STAT_CHAINS >= N) break;
            const long long steps = (long long)(int)a[j] + (long long)len[j] + ((st[j] & ST_DONE) ? 0 : (long long)t[j]);
            acc += col == 0 ? (unsigned long long)steps : (unsigned long long)a[j];
            ret += f[j];                                                        // env order within the chain: fixed
        }
    }
    part[(size_t)chain * 16 + col] = (col >= 9 && col < STAT_COLS) ? (unsigned long long)__double_as_longlong(ret) : acc;
}
__global__ __launch_bounds__(256) void k_stats_tree(const unsigned long long *__restrict__ part, cz_stats *out) {
    __shared__ unsigned long long su64[256][9];
    __shared__ double sd[256][4];
    for (int j = 0; j < 9; ++j) su64[threadIdx.x][j] = part[(size_t)threadIdx.x * 16 + j];
    for (int a = 0; a < 4; ++a) sd[threadIdx.x][a] = __longlong_as_double((long long)part[(size_t)threadIdx.x * 16 + 9 + a]);
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) {
            for (int j = 0; j < 9; ++j) su64[threadIdx.x][j] += su64[threadIdx.x + stride][j];
            for (int a = 0; a < 4; ++a) sd[threadIdx.x][a] += sd[threadIdx.x + stride][a];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out->env_steps = su64[0][0]; out->episodes = su64[0][1]; out->length_sum = su64[0][2];
        out->truncations = su64[0][3]; out->terminations = su64[0][4];
        for (int a = 0; a < 4; ++a) { out->recipes_completed[a] = su64[0][5 + a]; out->return_sum[a] = sd[0][a]; }
    }
}

// cz_reset_stats: zero the counters, the last-episode row and what cz_episodes_collect has seen; steps already taken by episodes in
// flight must not be counted again
__global__ void k_stats_clear(uint32_t *su, double *sf, uint32_t *ep_seen, const uint32_t *__restrict__ state, int RW, int N) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    uint32_t *p = su + (size_t)e * SU_WORDS;
    const uint32_t *rec = state + (size_t)e * RW;
    for (int j = 0; j < (int)SU_WORDS; ++j) p[j] = 0;
    p[SU_STEPS] = (rec[W_STATUS] & ST_DONE) ? 0u : (uint32_t)(-(int)rec[W_T]);
    for (int a = 0; a < 4; ++a) sf[(size_t)e * SF_WORDS + SF_SUM0 + a] = 0.0;
    for (int a = 0; a < 4; ++a) sf[(size_t)e * SF_WORDS + SF_LAST0 + a] = 0.0;
    ep_seen[e] = 0u;
}

// cz_episodes_collect: which envs finished an episode since the last collect (cooking_env.py:248,264,329 - the `episode` entries of
// `infos` - for the whole batch).  Env e is found when its episode counter, stat_u[e][SU_EPISODES], differs from ep_seen[e], the
// counter's value at the last collect; what is reported is the env's last-episode row, which the wave that ended the episode left in
// stat_u / stat_f (step_kernel).  The packed list is in ascending env order by construction: a found env's rank is the number of found
// envs in front of it - the blocks in front of its block (k_episodes_count's totals, added up in block order), the waves in front of
// its wave, the lanes in front of its lane (ballot and prefix count).  No atomic decides an order.  The counter words and the row were
// written by earlier launches: device-scope loads.
constexpr int EP_BLOCK = 256;
__device__ __forceinline__ uint32_t ep_load_u32(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ep_load_f64(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// how many envs of each block are found: block_count[blockIdx.x] (launched only when a rank is needed: d_list or d_count)
__global__ __launch_bounds__(EP_BLOCK) void k_episodes_count(const uint32_t *su, const uint32_t *ep_seen, int N, int32_t *block_count) {
    __shared__ int32_t wave_count[EP_BLOCK / 64];
    const int e = (int)blockIdx.x * EP_BLOCK + (int)threadIdx.x;
    bool found = false;
    if (e < N) found = ep_load_u32(su + (size_t)e * SU_WORDS + SU_EPISODES) != ep_load_u32(ep_seen + e);
    const uint64_t b = ballot(found);
    if ((threadIdx.x & 63u) == 0u) wave_count[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0u) {
        int32_t n = 0;
        for (int w = 0; w < EP_BLOCK / 64; ++w) n += wave_count[w];
        block_count[blockIdx.x] = n;
    }
}
// the outputs, and the mark.  block_count: null when neither the list nor the count was asked for.
__global__ __launch_bounds__(EP_BLOCK) void k_episodes_collect(const uint32_t *su, const double *sf, uint32_t *ep_seen, int N, int A,
                                                               int64_t env_id_base, const int32_t *block_count, uint8_t *mask,
                                                               double *ret, int32_t *length, uint32_t *flags, cz_episode *list,
                                                               int32_t capacity, int32_t *count) {
    __shared__ int32_t wave_count[EP_BLOCK / 64];
    __shared__ int32_t before, total;
    const int e = (int)blockIdx.x * EP_BLOCK + (int)threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0u) { before = 0; total = 0; }
    uint32_t episodes = 0u, seen = 0u;
    if (e < N) {
        episodes = ep_load_u32(su + (size_t)e * SU_WORDS + SU_EPISODES);
        seen = ep_load_u32(ep_seen + e);
    }
    const bool found = episodes != seen;
    const uint64_t b = ballot(found);
    if (lane == 0) wave_count[wave] = __popcll(b);
    __syncthreads();
    int32_t rank = 0;
    if (block_count) {
        // found envs in the blocks in front of this one (and, block 0: in all of them) - integer sums, the same in any order
        int32_t mine = 0, all = 0;
        for (int j = (int)threadIdx.x; j < (int)gridDim.x; j += EP_BLOCK) {
            const int32_t c = block_count[j];
            all += c;
            if (j < (int)blockIdx.x) mine += c;
        }
        if (mine) atomicAdd(&before, mine);
        if (blockIdx.x == 0u && all) atomicAdd(&total, all);
        __syncthreads();
        rank = before;
        for (int w = 0; w < wave; ++w) rank += wave_count[w];
        rank += __popcll(b & ((1ull << lane) - 1ull));
        if (count && blockIdx.x == 0u && threadIdx.x == 0u) *count = total;
    }
    if (e >= N) return;
    if (mask) mask[e] = found ? (uint8_t)1 : (uint8_t)0;
    if (!found) return;
    ep_seen[e] = episodes;
    const uint32_t *p = su + (size_t)e * SU_WORDS;
    const double *q = sf + (size_t)e * SF_WORDS + SF_LAST0;
    const uint32_t len = ep_load_u32(p + SU_LAST_LENGTH), fl = ep_load_u32(p + SU_LAST_FLAGS);
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    for (int a = 0; a < A; ++a) r[a] = ep_load_f64(q + a);
    if (ret) for (int a = 0; a < A; ++a) ret[(size_t)e * A + a] = r[a];
    if (length) length[e] = (int32_t)len;
    if (flags) flags[e] = fl;
    if (list && rank < capacity) {
        cz_episode ep;
        ep.env = env_id_base + e;
        ep.episode = ep_load_u32(p + SU_LAST_EPISODE); ep.length = len; ep.flags = fl; ep.finished = episodes - seen;
        for (int a = 0; a < 4; ++a) ep.ret[a] = r[a];
        list[rank] = ep;
    }
}

// cz_reset on envs whose episode is still running: their steps stay counted as env-steps
// measurement aid (cz_probe_output_only): a grid of the step kernel's shape that does nothing but write `bytes` with the
// same write-through 16-byte stores the observation encode uses -- the floor of any launch that has to emit that much
__global__ __launch_bounds__(64 * ENVS_PER_WG) void k_probe_fill(void *dst, uint32_t bytes) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(dst, 0, (int)bytes, 0x00020000);
    const uint32_t stride = gridDim.x * blockDim.x * 16u;
    for (uint32_t off = (blockIdx.x * blockDim.x + threadIdx.x) * 16u; off + 16u <= bytes; off += stride)
        __builtin_amdgcn_raw_buffer_store_b128(u4{0, 0, 0, 0}, rs, off, 0, 16);
}

// measurement aid (cz_probe_closed_loop): the smallest "policy" there is - every agent's next action is a hash of a few
// doubles of the observation it was just given - so that step k + 1 depends on step k's observation through a kernel of the
// caller, as in any reinforcement-learning loop
__global__ void k_probe_policy(const double *__restrict__ obs, int32_t *__restrict__ actions, int n_rows, int F, uint32_t n_actions) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;               // (env, agent)
    if (row >= n_rows) return;
    const unsigned long long *o = reinterpret_cast<const unsigned long long *>(obs) + (size_t)row * F;
    unsigned long long x = o[0] ^ (o[F / 3] * 3ull) ^ (o[(2 * F) / 3] * 5ull) ^ (o[F - 1] * 7ull) ^ ((unsigned long long)row << 17);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33;
    actions[row] = (int32_t)(((x & 0xFFFFFFFFull) * n_actions) >> 32);
}

// ... the same policy for a consumer of the COMPACT observation (cz_step_device_compact): the four features come as table
// indices, the table turns them into the very doubles k_probe_policy reads - so both loops take the same actions
__global__ void k_probe_policy_codes(const uint8_t *__restrict__ codes, const double *__restrict__ table, int32_t *__restrict__ actions,
                                     int n_rows, int F, int Fp, uint32_t n_actions) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;               // (env, agent)
    if (row >= n_rows) return;
    const uint8_t *c = codes + (size_t)row * Fp;
    const unsigned long long *t = reinterpret_cast<const unsigned long long *>(table);
    unsigned long long x = t[c[0]] ^ (t[c[F / 3]] * 3ull) ^ (t[c[(2 * F) / 3]] * 5ull) ^ (t[c[F - 1]] * 7ull) ^ ((unsigned long long)row << 17);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33;
    actions[row] = (int32_t)(((x & 0xFFFFFFFFull) * n_actions) >> 32);
}

// cz_load_layouts with a smaller pool: how many resident records still point past the new pool (layout id or redraw slice)
__global__ void k_layout_misfits(const uint32_t *__restrict__ state, int RW, int N, uint32_t n_new, unsigned long long *count) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const uint32_t *rec = state + (size_t)e * RW;
    const uint32_t base = rec[W_POOL] & 0xFFFFu, cnt = rec[W_POOL] >> 16;
    if (rec[W_LAYOUT] >= n_new || (cnt && base + cnt > n_new)) atomicAdd(count, 1ull);
}

// cz_set_spawn across the 31-step boundary: the countdown fields of the status word change their width (spawn_grace_bits); the
// resident records are re-packed so that no env reads another agent's bits (a countdown that does not fit the narrower field is
// clamped to its maximum, 31 - the new period is at most 31 then, so the agent is protected for at most one period)
__global__ void k_repack_grace(uint32_t *state, int RW, int N, int n_agents, uint32_t old_bits, uint32_t new_bits) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    uint32_t *rec = state + (size_t)e * RW;
    const uint32_t st = rec[W_STATUS];
    uint32_t out = st & ((1u << SPAWN_GRACE0) - 1u);
    for (int a = 0; a < n_agents; ++a) {
        const uint32_t g = (st >> (SPAWN_GRACE0 + old_bits * a)) & ((1u << old_bits) - 1u);
        out |= min(g, (1u << new_bits) - 1u) << (SPAWN_GRACE0 + new_bits * a);
    }
    rec[W_STATUS] = out;
}

__global__ void k_count_aborted(uint32_t *su, const uint32_t *__restrict__ state, int RW, long long env_begin, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *rec = state + (size_t)(env_begin + i) * RW;
    if (!(rec[W_STATUS] & ST_DONE)) su[(size_t)(env_begin + i) * SU_WORDS + SU_STEPS] += rec[W_T];
}

// A record leaves the batch (cz_save_device): env e copies its RW words, the running-return words included, to row slot[e] of the
// caller's archive uint32[capacity][RW] (no slot array: row e; the host has checked capacity >= N).  A negative slot skips the env, a
// slot >= capacity writes nothing.  One wavefront per env and workgroup; nothing of the handle changes.  Two envs that name one row
// race for it: the caller's contract.
__global__ __launch_bounds__(64) void k_save_where(const uint32_t *__restrict__ state, int32_t RW, const int32_t *__restrict__ slot,
                                                   uint32_t *__restrict__ records, int64_t capacity) {
    const uint32_t env = blockIdx.x;
    int64_t s = (int64_t)env;
    if (slot) {
        const int32_t v = (int32_t)rfl((uint32_t)slot[env]);
        if (v < 0) return;
        s = v;
    }
    if (s >= capacity) return;
    const uint32_t *rec = state + (size_t)env * RW;
    uint32_t *row = records + (size_t)s * RW;
    for (uint32_t w = threadIdx.x; w < (uint32_t)RW; w += 64u) stg<uint32_t>(row, w * 4u, ldg<uint32_t>(rec, w * 4u));
}

// ======================================================================================================
// host: handle + C-ABI
// ======================================================================================================

// the owners of everything a handle (or a call) has to give back
template <class T> using DevMem = Owned<T *, hipFree>;          // hipMalloc
template <class T> using PinnedMem = Owned<T *, hipHostFree>;   // hipHostMalloc
using OwnedStream = Owned<hipStream_t, hipStreamDestroy>;
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;
using OwnedGraph = Owned<hipGraph_t, hipGraphDestroy>;
using OwnedGraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;

struct cz_handle_s {
    cz_config cfg;
    Params P;
    hipStream_t stream = nullptr;      // the stream every call of this handle is ordered on (not owned: own_stream, or a caller's)
    // Members are destroyed in reverse order of declaration: the streams stand in front of every buffer, event and graph that work on
    // them may still reference, so they outlive them (cz_destroy has waited for all four by then).
    OwnedStream own_stream;            // the one cz_create made (cz_set_stream may point `stream` at a caller's)
    OwnedStream rank_stream;           // cz_load_layout_ranks: its copies run here; the handle's stream waits for them on the device
    OwnedStream copy_stream;           // cz_update_layouts copies run here, beside the steps
    OwnedStream split_stream;          // the second chain of a split run (made by its first one)
    Launchers kl;
    int n_layouts = 0, n_recipes = 0;
    DevMem<uint32_t> d_state, d_lay_desc, d_recipes;
    DevMem<uint32_t> d_lay_block;          // the allocation behind d_lay_init: LAY_CTL_WORDS control words, then the records
    uint32_t *d_lay_init = nullptr;        // a view: the records inside d_lay_block
    DevMem<uint16_t> d_lay_rank;           // [L][W * H]: the position of a cell's static object in world_objects[class] (cz_load_layout_ranks, cz_generate_layouts)
    std::vector<uint8_t> rank_ok;          // per pool slot: its rank row belongs to its layout
    int rank_missing = 0;                  // how many do not
    PinnedMem<uint16_t> h_rank_stage;      // pinned staging of cz_load_layout_ranks, a place per slot
    OwnedEvent ev_rank_done;               // behind its copies on rank_stream
    DevMem<float> d_policy;                // cz_load_policy_device: POLICY_MAX_SETS packed weight sets (cz_policy.h), allocated on the first load
    int32_t n_policy_sets = 0;             // sets the last load filled; 0: no table
    int32_t n_value_sets = 0;              // cz_load_value_device: sets whose value head (behind the sets, same allocation) the last load filled
    DevMem<unsigned char> d_ppo;           // cz_ppo_reserve: the workspace of cz_ppo_grad_device (ppo_carve), for ...
    int64_t ppo_positions = 0;             // ... minibatches of up to this many positions (0: none reserved) over ...
    int32_t ppo_sets = 0;                  // ... this many loaded sets
    DevMem<double> d_adam;                 // cz_adam_reserve: the chunk partials of cz_adam_step_device for POLICY_MAX_SETS sets, then its control words (cz_adam.h)
    DevMem<uint32_t> d_partner;            // cz_load_partner_table: [n_partner][PARTNER_ROW_WORDS], then the bad-recipe counter (8 bytes)
    int n_partner = 0;                     // rows in use (0: none, or dropped by cz_load_recipes)
    int partner_rows_alloc = 0;            // rows the allocation was made for (the counter lies behind them)
    PinnedMem<char> h_lay_stage;           // pinned staging of cz_update_layouts: [L] records, then [L] descriptors
    OwnedEvent ev_copy_done, ev_steps_issued;
    bool copy_pending = false;             // a copy has been issued that no cz_set_layout_group has waited for yet
    struct SlotRange { int32_t first, count; };
    std::vector<SlotRange> upd_ranges;     // staged by cz_update_layouts, not copied yet (flush_updates)
    std::vector<SlotRange> staged_on_copy, staged_on_main;   // slots of copies issued on the copy stream / in order on the handle's stream whose completion nobody has seen yet
    OwnedEvent ev_main_copy_done;
    int32_t lay_groups = 1, lay_active = 0;
    int64_t n_layout_updates = 0;
    DevMem<void> d_gen_tables;             // cz_load_level_programs: failure counter | program offsets | programs | level of every slot
    GenParams gen = {};                     // ... and where its parts are
    int gen_layouts = 0;                   // the pool size those tables were made for
    std::vector<SlotRange> gen_slices;     // per pool slot: the run of slots of its level (the pool slice an env of that level draws from)
    DevMem<void> d_spawn_tables;           // cz_set_spawn: exhausted-respawn counter | spawn areas per (level, agent) | level of every layout
    int spawn_layouts = 0;                 // the pool size those tables were made for
    uint32_t spawn_bits = 5;               // width of the countdown fields the resident records are packed with (spawn_grace_bits)
    DevMem<uint32_t> d_stat_u;
    DevMem<double> d_stat_f;
    DevMem<uint32_t> d_ep_seen;        // [N]: stat_u[e][SU_EPISODES] at the last cz_episodes_collect
    DevMem<int32_t> d_ep_blocks;       // [ceil(N / EP_BLOCK)]: found envs per block, between the two launches of a collect
    DevMem<cz_stats> d_stats_out;
    DevMem<unsigned long long> d_stats_part;      // [256 chains][16 columns] between the two stages of the reduction
    DevMem<double> d_lut;
    DevMem<void> d_sprites;            // cz_load_sprites: float table [256] | sheet [RENDER_SPRITES][M][M] RGBA
    int32_t sprites_M = 0;             // 0: no sheet loaded
    double obs_table[LUT_SIZE];        // host copy of the quotient table (cz_obs_table: what the compact observation's codes index)
    DevMem<int32_t> d_reset_words;     // [3][N]: layout ids, recipe words, pool words of a cz_reset call
    DevMem<unsigned long long> d_reset_refused;      // cz_reset_device: envs whose explicit layout id was out of range (cz_reset_device_refused)
    DevMem<unsigned long long> d_restore_refused;    // cz_restore_device: envs whose slot or row was refused (cz_restore_device_refused)
    DevMem<unsigned long long> d_tasks_refused;      // cz_set_tasks_device: envs whose new recipe ids were out of range (cz_set_tasks_refused)
    DevMem<uint8_t> d_goal;                // cz_load_goal_table: [n_goal_rows][GOAL_ROW_NODES] goal ids
    int n_goal_rows = 0;                   // rows in use (0: none, or dropped by cz_load_recipes)
    int num_goals = 0;                     // the length of a goal vector
    uint8_t *codes = nullptr;          // cz_set_compact_output: one-step launches also write the compact observation here
    float *obs32 = nullptr;            // cz_set_f32_output: one-step launches called with d_obs = NULL write float32 rows here
    DevMem<void> d_codes_stage;        // cz_step_compact with pageable host memory: device staging of the codes
    DevMem<void> d_dump;               // [N][4] doubles: where a one-step launch writes an output array the caller passed as NULL
    // staging for the host-pointer API
    DevMem<int32_t> d_actions;
    DevMem<double> d_obs;
    DevMem<char> d_small;                          // rewards | terminations | truncations | marks: one device block, one pinned block
    PinnedMem<char> h_small;
    PinnedMem<uint32_t> h_marks;                   // pinned, device-mapped marks buffer of the direct path
    uint32_t *d_marks_mapped = nullptr;            // ... as the device sees it (a view)
    std::vector<uint32_t> last_marks;          // recipe marks after the most recent cz_step (cz_last_marks)
    PinnedMem<char> h_stage;                       // small batches: pinned, device-mapped staging block of cz_step
    char *d_stage = nullptr;                       // ... as the device sees it (a view)
    // cz_step_device_ring: which ring / output buffers / tables the cached graphs were captured for
    struct RingKey {
        const int32_t *ring = nullptr; int64_t stride = 0; int32_t period = 0;
        double *obs = nullptr, *rew = nullptr; uint8_t *term = nullptr, *trunc = nullptr; hipStream_t stream = nullptr; uint64_t version = 0;
        int32_t parts = 1;             // launch chains per run (cz_set_ring_split)
        bool operator==(const RingKey &o) const {
            return ring == o.ring && stride == o.stride && period == o.period && obs == o.obs && rew == o.rew && term == o.term &&
                   trunc == o.trunc && stream == o.stream && version == o.version && parts == o.parts;
        }
    } ring_key;
    // (hidden: the std::vector<RunGraph> members and its destructor are instantiated with it and must not join the library's exports)
    struct __attribute__((visibility("hidden"))) RunGraph { int32_t slot, len; OwnedGraphExec ge, ge2; uint64_t used; };   // ge2: the second chain of a split run, or null
    std::vector<RunGraph> ring_graphs;             // replayable runs of this ring, keyed by (first slot, length)
    uint64_t ring_clock = 0;
    int64_t n_graph_kernels = 0, n_direct_kernels = 0;
    uint64_t tables_version = 0;                   // bumped whenever something the launches capture by value changes
    OwnedEvent ev0, ev1;
    // kernel timing
    bool ktime = false;
    std::vector<OwnedEvent> kev;
    size_t kev_used = 0;
    double ktime_ms = 0.0;
    int64_t klaunches = 0;
    // RCCL (lazy)
    void *rccl = nullptr;
    void *comm = nullptr;
    int n_ranks = 1, rank = 0;
    int wt_override = -1;          // CZ_WT experiment switch, read once
    bool lean_enabled = true;      // CZ_LEAN=0: one-step launches always take the generic kernel (A/B runs, tests)
    bool lean_cfg_enabled = true;  // CZ_LEAN_CFG=0: lean launches always take k_step_lean, never a k_step_lean_cfg (A/B runs)
    int ppo_tile = PPO_TILE;               // CZ_PPO_TILE=<features per workgroup>: k_ppo_outer's instance (tools/ppo_sizes.py)
    int gae_shape = GAE_DEPTH * 1000 + GAE_BLOCK;   // CZ_GAE_SHAPE=<rows ahead>x<workgroup size>: k_gae's instance (tools/targets_sizes.py)
    int last_step_variant = -1;    // cz_diag_last_step_variant
    int last_step_lean = -1;       // which kernel the most recent launch_step took: 1 k_step_lean, 0 another one (cz_diag_last_step_lean)
    int last_step_mode = -1;       // the StepMode of that launch (cz_diag_last_step_mode)
    bool huge = false;             // the 256-slot / 1024-cell instance (its own LDS image layout)
    int instance = 0;              // which kernel instance cz_create picked: 0 small, 1 large, 2 huge (cz_diag_instance)
    unsigned long long *tl_base = nullptr;   // timeline build: stamp buffer, its capacity in launches, launches so far
    int32_t tl_cap = 0;
    int64_t tl_count = 0;
    bool graphs_enabled = true;    // CZ_GRAPHS=0: cz_step_device_ring launches everything directly
    bool ring_fused = false;       // cz_set_ring_fused: runs of cz_step_device_ring / _many go out as fused launches (outputs in place)
    int64_t n_ring_fused_steps = 0;
    int32_t graph_min_run = 48;    // CZ_GRAPH_MIN_RUN: shorter pieces of a ring run are launched directly (see ring_walk)
    int32_t ring_prefix = 0;       // CZ_RING_PREFIX: steps of a cz_step_device_ring call launched directly in front of its first graph
    int32_t ring_split = -1;       // cz_set_ring_split / CZ_RING_SPLIT: -1 automatic, 0 off, 2 two launch chains (run_split)
    bool few_queues = false;       // GPU_MAX_HW_QUEUES below 4 in the environment of cz_create: runs are never split
    OwnedEvent ev_fork, ev_join;                   // in front of and behind the second chain of a split run
    size_t zero_copy_bytes = (size_t)256 << 10;   // cz_step: batches whose buffers fit use the pinned device-mapped block (CZ_ZERO_COPY_BYTES)
    DevMem<cz_stats> d_gather;
    std::string err;
};

static thread_local std::string g_err;
static int ready(cz_handle h);
static int set_device(cz_handle h);
static int begin_ranged_call(cz_handle h, int64_t b, int64_t c);
static void mark_ranks(cz_handle h, int32_t first, int32_t count, int ok);
static int flush_updates(cz_handle h, bool force);

static int fail(cz_handle h, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_err = buf;
    return 1;
}

#define HIPCHK(h, call)                                                                      \
    do {                                                                                     \
        hipError_t _e = (call);                                                              \
        if (_e != hipSuccess) return fail(h, "%s failed: %s", #call, hipGetErrorString(_e)); \
    } while (0)

extern "C" const char *cz_last_error(cz_handle h) { return h ? h->err.c_str() : g_err.c_str(); }

// one counter (a T) in device memory, as it stands behind everything on the handle's stream (waits for it); -1 on error
template <class T>
static int64_t read_counter(cz_handle h, const void *d_counter, const char *who) {
    T n = 0;
    if (hipSetDevice(h->cfg.device_id) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
        hipMemcpy(&n, d_counter, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) { fail(h, "%s: copy failed", who); return -1; }
    return (int64_t)n;
}
// the level of every slot of the resident pool (`level_of`; null: all of them level 0), each < n_levels: `misfit` is the caller's
// message for a slot that is not - its slot, its level, n_levels
static int pool_levels(cz_handle h, const uint8_t *level_of, int32_t n_levels, const char *misfit, std::vector<uint8_t> &levels) {
    levels.assign((size_t)h->n_layouts, 0);
    for (int i = 0; i < h->n_layouts; ++i) {
        const int lv = level_of ? level_of[i] : 0;
        if (lv >= n_levels) return fail(h, misfit, i, lv, n_levels);
        levels[(size_t)i] = (uint8_t)lv;
    }
    return 0;
}

// Is the stream this handle's work goes to (a stream of the caller, cz_set_stream) being captured - hipStreamBeginCapture,
// torch.cuda.graph - right now?  The device-pointer steps (cz_step_device, _compact, _f32, _many, _ring, cz_rollout*), cz_reset_device, cz_set_tasks_device, cz_infos_device, cz_save_device and cz_restore_device are then pure
// kernel launches: nothing that queries or synchronises (a staged layout update stays staged until the first call outside the
// capture; no graphs of the library's own inside the caller's), so the capture stays valid and replays do what the launches did.
static bool caller_capturing(cz_handle h) {
    if (h->stream == h->own_stream) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

extern "C" int32_t cz_stream_capturing(cz_handle h) { return h && caller_capturing(h) ? 1 : 0; }

extern "C" int32_t cz_abi_version(void) { return CZ_ABI_VERSION; }
// diagnostic builds only (tools/phase_profile.py): where the kernels write their s_memtime stamps
extern "C" int cz_debug_set_stamps(cz_handle h, void *d_buf) {
    if (!h) return 1;
#ifdef CZ_PROFILE
    h->P.stamps = (unsigned long long *)d_buf;
#else
    (void)d_buf;
    return fail(h, "cz_debug_set_stamps: this is not the diagnostic build (make prof)");
#endif
    return 0;
}
// timeline builds only (tools/timeline.py): launch k of the step kernel writes its waves' entry / exit stamps to
// d_buf + (k % cap_launches) * num_envs * 2 (uint64); cap_launches = 0 switches it off
extern "C" int cz_debug_set_timeline(cz_handle h, void *d_buf, int32_t cap_launches) {
    if (!h) return 1;
#ifdef CZ_TIMELINE
    h->tl_base = (unsigned long long *)d_buf;
    h->tl_cap = d_buf ? cap_launches : 0;
    h->tl_count = 0;
    return 0;
#else
    (void)d_buf; (void)cap_launches;
    return fail(h, "cz_debug_set_timeline: this is not the timeline build (make timeline)");
#endif
}
extern "C" int32_t cz_sizeof_config(void) { return (int32_t)sizeof(cz_config); }
extern "C" int32_t cz_sizeof_stats(void) { return (int32_t)sizeof(cz_stats); }
extern "C" uint32_t cz_action(uint64_t seed, int64_t env_global, int32_t agent, uint32_t step, uint32_t n_actions) {
    return action_hash(seed, env_global, agent, step, n_actions);
}
extern "C" uint32_t cz_next_layout(int64_t env_global, uint32_t episode, uint32_t pool_word, uint32_t n_layouts) {
    return next_layout(env_global, episode, pool_word, n_layouts);
}
extern "C" uint32_t cz_next_layout_group(int64_t env_global, uint32_t episode, uint32_t pool_word, uint32_t n_layouts, uint32_t groups,
                                         uint32_t active) {
    return next_layout(env_global, episode, pool_word, n_layouts, groups ? groups : 1u, active);
}

static int create_resources(cz_handle h, int C);
extern "C" int cz_create(const cz_config *cfg, cz_handle *out) {
    if (!cfg || !out) return fail(nullptr, "cz_create: null argument");
    *out = nullptr;
    const int C = cfg->width * cfg->height;
    if (cfg->num_envs < 1) return fail(nullptr, "cz_create: num_envs must be >= 1");
    if (cfg->num_agents < 1 || cfg->num_agents > MAX_AGENTS) return fail(nullptr, "cz_create: num_agents must be 1..4");
    if (cfg->num_recipes < cfg->num_agents || cfg->num_recipes > MAX_AGENTS)
        return fail(nullptr, "cz_create: need num_agents <= num_recipes <= 4 (one recipe per agent, cooking_env.py:329)");
    // (the quotient table holds 2W-1 x-entries from index 0 and 2H-1 y-entries from index 64, below the constants at 126/127)
    if (cfg->width < 1 || cfg->height < 1 || cfg->width > 32 || cfg->height > 32)
        return fail(nullptr, "cz_create: grid %dx%d unsupported (W <= 32, H <= 32)", cfg->width, cfg->height);
    static_assert(2 * 32 - 1 <= LUT_Y0 && LUT_Y0 + 2 * 32 - 1 <= LUT_ZERO, "quotient table layout");
    if (cfg->max_dyn < 1 || cfg->max_dyn > 255) return fail(nullptr, "cz_create: max_dyn must be 1..255 (slot + 1 is an 8-bit field)");
    if (cfg->action_scheme != 1 && cfg->action_scheme != 3)
        return fail(nullptr, "cz_create: action_scheme must be 1 or 3 (scheme2 is unusable in the reference)");
    if (cfg->max_steps < 1 || cfg->feat_len < 1) return fail(nullptr, "cz_create: max_steps and feat_len must be positive");
    {   // the kernels address a handle's records and one-step outputs with 32-bit offsets
        const uint64_t rw = ((uint64_t)(20 + (C + 3) / 4 + 2 * cfg->max_dyn) + 15) / 16 * 16;
        if ((uint64_t)cfg->num_envs * rw * 4 >= (1ull << 32) || (uint64_t)cfg->num_envs * cfg->num_agents * 8 >= (1ull << 32))
            return fail(nullptr, "cz_create: num_envs too large for one handle (records must stay below 4 GiB): use several handles");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, "cz_create: no HIP device available (this library has no CPU fallback)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, "cz_create: device_id %d out of range", cfg->device_id);
    cz_handle h = new cz_handle_s();
    h->cfg = *cfg;
    // from here on a failure must release what was already created, and is reported as cz_create's (there is no handle to ask)
    if (create_resources(h, C)) {
        fail(nullptr, "cz_create: %s", h->err.c_str());
        cz_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}
// what a fresh handle holds: its stream and events, the settings of the environment, the kernel instance, the records, statistics and
// scratch of the batch, the constant tables behind Params::lut
static int create_resources(cz_handle h, int C) {
    const cz_config *const cfg = &h->cfg;
    HIPCHK(h, hipSetDevice(cfg->device_id));
    HIPCHK(h, hipStreamCreateWithFlags(h->own_stream.out(), hipStreamNonBlocking));
    h->stream = h->own_stream;
    HIPCHK(h, hipEventCreate(h->ev0.out()));
    HIPCHK(h, hipEventCreate(h->ev1.out()));
    Params &P = h->P;
    memset(&P, 0, sizeof P);
    P.N = cfg->num_envs; P.A = cfg->num_agents; P.W = cfg->width; P.H = cfg->height; P.D = cfg->max_dyn; P.F = cfg->feat_len;
    const int CW = (C + 3) / 4;
    P.dyn0_off = CELL_WORD0 + CW;   // CELL_WORD0 = 8 header + 4 agents + 8 words of running returns
    P.dyn1_off = P.dyn0_off + P.D;
    P.RW = (P.dyn1_off + P.D + 15) / 16 * 16;
    P.scheme = cfg->action_scheme; P.max_steps = cfg->max_steps; P.end_all = cfg->end_condition_all ? 1 : 0;
    P.R = cfg->num_recipes; P.auto_reset = cfg->auto_reset ? 1 : 0; P.env_id_base = cfg->env_id_base;
    P.recipe_reward = cfg->recipe_reward; P.recipe_penalty = cfg->recipe_penalty; P.node_reward = cfg->recipe_node_reward;
    P.time_penalty_step = cfg->max_time_penalty / (double)cfg->max_steps;       // cooking_env.py:307
    P.T = 1;
    if (const char *s = getenv("CZ_WT")) h->wt_override = atoi(s);
    if (const char *s = getenv("CZ_LEAN")) h->lean_enabled = atoi(s) != 0;
    if (const char *s = getenv("CZ_LEAN_CFG")) h->lean_cfg_enabled = atoi(s) != 0;
    if (const char *s = getenv("CZ_GRAPHS")) h->graphs_enabled = atoi(s) != 0;
    if (const char *s = getenv("CZ_GAE_SHAPE")) {
        int d = 0, w = 0;
        if (sscanf(s, "%dx%d", &d, &w) == 2) h->gae_shape = d * 1000 + w;      // (a shape the library does not carry is refused by the call)
    }
    if (const char *s = getenv("CZ_PPO_TILE")) h->ppo_tile = atoi(s);      // (a tile the library does not carry is refused by the call)
    if (const char *s = getenv("CZ_GRAPH_MIN_RUN")) h->graph_min_run = atoi(s) < 4 ? 4 : (atoi(s) > 256 ? 256 : atoi(s));   // 4..RING_MAX_GRAPH
    if (const char *s = getenv("CZ_RING_PREFIX")) h->ring_prefix = atoi(s) < 0 ? 0 : (atoi(s) > 16 ? 16 : atoi(s));
    if (const char *s = getenv("CZ_ZERO_COPY_BYTES")) h->zero_copy_bytes = (size_t)atoll(s);
    if (const char *s = getenv("CZ_RING_SPLIT")) h->ring_split = atoi(s) == 2 ? 2 : atoi(s) == 0 ? 0 : -1;
    // (read, never set: with fewer than 4 hardware queues the runtime can crash replaying a graph that has parallel branches)
    if (const char *s = getenv("GPU_MAX_HW_QUEUES")) h->few_queues = atoi(s) < 4;
#ifdef CZ_SMALL_ONLY      // diagnostic libraries that carry the small instance only
    if (!(P.D <= 64 && C <= 64)) return fail(h, "this diagnostic library holds the small kernel instance only");
    h->kl = launchers_small();
#else
    h->instance = (P.D <= 64 && C <= 64) ? 0 : (P.D <= 128 && C <= 256) ? 1 : 2;
    h->kl = h->instance == 0 ? launchers_small() : h->instance == 1 ? launchers_large() : launchers_huge();
#endif
    h->huge = P.D > 128 || C > 256;
    {   // the reward of a step on which no recipe node changed: cooking_env.py:304-307 with zero deltas, same op order
        double x = 0.0;
        x += (double)0 * P.node_reward;
        x += 0.0 * P.recipe_reward;
        x += 0.0 * P.recipe_penalty;
        x += P.time_penalty_step;
        P.reward_idle = x;
    }
    const size_t N = (size_t)P.N;
    const size_t state_bytes = N * P.RW * 4;
    HIPCHK(h, hipMalloc(h->d_state.out(), state_bytes));
    HIPCHK(h, hipMemsetAsync(h->d_state, 0, state_bytes, h->stream));
    HIPCHK(h, hipMalloc(h->d_stat_u.out(), N * SU_WORDS * 4));
    HIPCHK(h, hipMalloc(h->d_stat_f.out(), N * SF_WORDS * 8));
    HIPCHK(h, hipMemsetAsync(h->d_stat_u, 0, N * SU_WORDS * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_stat_f, 0, N * SF_WORDS * 8, h->stream));
    HIPCHK(h, hipMalloc(h->d_ep_seen.out(), N * 4));
    HIPCHK(h, hipMemsetAsync(h->d_ep_seen, 0, N * 4, h->stream));
    HIPCHK(h, hipMalloc(h->d_ep_blocks.out(), ((N + EP_BLOCK - 1) / EP_BLOCK) * sizeof(int32_t)));
    HIPCHK(h, hipMalloc(h->d_stats_out.out(), sizeof(cz_stats)));
    HIPCHK(h, hipMalloc(h->d_dump.out(), N * MAX_AGENTS * sizeof(double)));
    HIPCHK(h, hipMalloc(h->d_reset_words.out(), N * 3 * sizeof(int32_t)));
    HIPCHK(h, hipMalloc(h->d_reset_refused.out(), sizeof(unsigned long long)));
    HIPCHK(h, hipMemsetAsync(h->d_reset_refused, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMalloc(h->d_restore_refused.out(), sizeof(unsigned long long)));
    HIPCHK(h, hipMemsetAsync(h->d_restore_refused, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMalloc(h->d_tasks_refused.out(), sizeof(unsigned long long)));
    HIPCHK(h, hipMemsetAsync(h->d_tasks_refused, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMalloc(h->d_stats_part.out(), (size_t)STAT_CHAINS * 16 * sizeof(unsigned long long)));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    P.state = h->d_state; P.stat_u = h->d_stat_u; P.stat_f = h->d_stat_f;
    {   // observation quotients: (x - ax) / W and (y - ay) / H for every possible difference, computed here with the same
        // IEEE-754 double division Python's int / int true division performs (cooking_env.py:364-368)
        double lut[LUT_SIZE];
        for (int i = 0; i < LUT_SIZE; ++i) lut[i] = 0.0;
        for (int i = 0; i < 2 * P.W - 1; ++i) lut[i] = (double)(i - (P.W - 1)) / (double)P.W;
        for (int i = 0; i < 2 * P.H - 1; ++i) lut[LUT_Y0 + i] = (double)(i - (P.H - 1)) / (double)P.H;
        lut[LUT_ZERO] = 0.0; lut[LUT_ONE] = 1.0;
        // flag truth tables (cz_device.h LUT_*): world_objects.py feature vectors of ChopFood / BlenderFood (int(not done()),
        // chop_state, blend_state), Switch / Block (switch_active / int(walkable)), Agent (orientation one-hot)
        for (int st = 0; st < 4; ++st) {
            lut[LUT_NDONE0 + st] = st == 0 ? 1.0 : 0.0;
            lut[LUT_CH0 + st] = (st & 1) ? 1.0 : 0.0;
            lut[LUT_MA0 + st] = (st & 2) ? 1.0 : 0.0;
            lut[LUT_CF0 + st] = st != 0 ? 1.0 : 0.0;
        }
        for (int k = 1; k <= 4; ++k) lut[LUT_OR0 + 8 * (k - 1) + k] = 1.0;
        // ... followed by one word per lane for the observer-relative features (cz_kernels.h observe): lane 16 a + code of the
        // subtrahend table holds observer a's x (mask in the low half), y (high half) or nothing.  Axis codes (soa.py):
        // 1 x, 2 y, 4 + 2 j x unless j == a, 5 + 2 j y unless j == a (an agent's own position is absolute, cooking_env.py:366-368)
        uint32_t submask[64];
        for (int l = 0; l < 64; ++l) {
            const int a = l >> 4, code = l & 15;
            const bool selx = code == 1 || (code >= 4 && !(code & 1) && (code - 4) / 2 != a);
            const bool sely = code == 2 || (code >= 5 && (code & 1) && (code - 5) / 2 != a);
            submask[l] = (selx ? 0x7F8u : 0u) | (sely ? 0x7F8u << 16 : 0u);
        }
        // ... followed by the despawn / respawn parameters (SpawnCfg, cz_set_spawn; all zero: switched off)
        static_assert(SPAWN_CFG_OFFSET == sizeof lut + sizeof submask, "layout of the block behind Params::lut");
        // ... the image words of the cells' coordinates (init_lds: x + W - 1 and 63 + y + H - 1 as byte offsets into this table,
        // one word per cell) and, per lane, which word of which of the env's recipe rows it holds (load_recipe_rows)
        uint32_t coords[1024], rowsel[64];
        const uint32_t c01 = (uint32_t)((P.W - 1) * 8) | ((uint32_t)((LUT_Y0 + P.H - 1) * 8) << 16);
        for (uint32_t c = 0; c < 1024; ++c) {
            const uint32_t y = c / (uint32_t)P.W, x = c - y * (uint32_t)P.W;
            coords[c] = (y < 64u) ? ((x << 3) | (y << 19)) + c01 : 0u;
        }
        for (uint32_t l = 0; l < 64; ++l) {
            const uint32_t lc = l < 9u * (uint32_t)P.R ? l : 9u * (uint32_t)P.R - 1u;       // lanes past the rows repeat the last word
            rowsel[l] = (8u * (lc / 9u)) | ((4u * (lc % 9u)) << 8);
        }
        static_assert(LUT_BLOCK_BYTES == sizeof lut + sizeof submask + sizeof(SpawnCfg) + sizeof coords + sizeof rowsel, "layout of the block behind Params::lut");
        HIPCHK(h, hipMalloc(h->d_lut.out(), LUT_BLOCK_BYTES));
        HIPCHK(h, hipMemset(h->d_lut, 0, LUT_BLOCK_BYTES));
        HIPCHK(h, hipMemcpy((char *)h->d_lut.get() + COORD_TABLE_OFFSET, coords, sizeof coords, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy((char *)h->d_lut.get() + ROWSEL_TABLE_OFFSET, rowsel, sizeof rowsel, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->d_lut, lut, sizeof lut, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy((char *)h->d_lut.get() + sizeof lut, submask, sizeof submask, hipMemcpyHostToDevice));
        P.lut = h->d_lut;
        memcpy(h->obs_table, lut, sizeof lut);
    }
    return 0;
}

extern "C" int cz_destroy(cz_handle h) {
    if (!h) return 0;
    (void)hipSetDevice(h->cfg.device_id);
    (void)hipStreamSynchronize(h->stream);
    for (hipStream_t s : {h->copy_stream.get(), h->rank_stream.get(), h->split_stream.get()})
        if (s) (void)hipStreamSynchronize(s);
    if (h->comm && h->rccl) {
        typedef int (*destroy_t)(void *);
        destroy_t f = (destroy_t)dlsym(h->rccl, "ncclCommDestroy");
        if (f) f(h->comm);
    }
    delete h;
    return 0;
}

// Order this handle's work on a stream of the caller (e.g. the current stream of the framework that produces the
// actions and consumes the observations), so that no host synchronisation is needed in between.  NULL = back to the
// handle's own stream.  Work already queued on the previous stream is waited for first.
extern "C" int cz_set_stream(cz_handle h, void *hip_stream) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    h->tables_version++;
    return 0;
}
// Agent despawn / respawn for every world of the batch, on the device (cooking_world.py:267-290).  rates 0 / 0 switch it off.
// The spawn areas come from the level files (their AGENTS entries, parsing.py:118-151), so they are per LEVEL: level_of_layout
// says which level every layout of the resident pool instantiates (NULL: all of them level 0), spawn_x / spawn_y hold per
// (level, agent) `stride` candidate coordinates of which the first n_x / n_y count.
extern "C" int cz_set_spawn(cz_handle h, double despawn_rate, double respawn_rate, int32_t grace_period, uint64_t seed,
                            int32_t n_levels, const uint8_t *level_of_layout, int32_t stride, const uint8_t *spawn_x, const int32_t *n_x,
                            const uint8_t *spawn_y, const int32_t *n_y) {
    if (!h) return fail(nullptr, "null handle");
    const bool on = despawn_rate > 0.0 || respawn_rate > 0.0;
    if (despawn_rate < 0.0 || respawn_rate < 0.0 || grace_period < 0 || (uint32_t)grace_period > spawn_max_grace(h->P.A))
        return fail(h, "cz_set_spawn: rates must be >= 0 and 0 <= grace_period <= %u for %d agent(s) (20 bits of the record's status word hold the "
                       "countdowns of all agents)", spawn_max_grace(h->P.A), h->P.A);
    SpawnCfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.seed = seed; cfg.despawn_rate = despawn_rate; cfg.respawn_rate = respawn_rate; cfg.grace_period = (uint32_t)grace_period | (spawn_grace_bits((uint32_t)grace_period, h->P.A) << 24);
    std::vector<uint8_t> areas, levels;
    if (on) {
        if (!h->P.lay_init) return fail(h, "cz_set_spawn: load the layout pool first (the spawn areas are looked up by layout)");
        if (!spawn_x || !n_x || !spawn_y || !n_y || n_levels < 1 || n_levels > 255 || stride < 1 || stride > 1024)
            return fail(h, "cz_set_spawn: spawn areas missing, or not 1..255 levels with 1..1024 candidates per list");
        const size_t blk = 4 + 2 * (size_t)stride;
        areas.assign((size_t)n_levels * MAX_AGENTS * blk, 0);
        for (int l = 0; l < n_levels; ++l)
            for (int a = 0; a < h->P.A; ++a) {
                const int nx = n_x[l * h->P.A + a], ny = n_y[l * h->P.A + a];
                if (nx < 1 || nx > stride || ny < 1 || ny > stride)
                    return fail(h, "cz_set_spawn: level %d, agent %d: 1..%d x and y candidates", l, a, stride);
                uint8_t *b = areas.data() + ((size_t)l * MAX_AGENTS + a) * blk;
                b[0] = (uint8_t)(nx & 255); b[1] = (uint8_t)(nx >> 8); b[2] = (uint8_t)(ny & 255); b[3] = (uint8_t)(ny >> 8);
                memcpy(b + 4, spawn_x + ((size_t)l * h->P.A + a) * stride, (size_t)stride);
                memcpy(b + 4 + stride, spawn_y + ((size_t)l * h->P.A + a) * stride, (size_t)stride);
            }
        if (pool_levels(h, level_of_layout, n_levels, "cz_set_spawn: layout %d is of level %d, but only %d level(s) have spawn areas", levels)) return 1;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->d_spawn_tables.reset();
    h->spawn_layouts = 0;
    const uint32_t new_bits = spawn_grace_bits((uint32_t)grace_period, h->P.A);
    if (new_bits != h->spawn_bits) {       // episodes in flight keep their countdowns: re-pack them to the new field width
        hipLaunchKernelGGL(k_repack_grace, dim3((unsigned)((h->P.N + 255) / 256)), dim3(256), 0, h->stream, h->d_state, h->P.RW, (int)h->P.N,
                           h->P.A, h->spawn_bits, new_bits);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->spawn_bits = new_bits;
    }
    if (on) {
        // one allocation: the counter word, the areas, the level of every layout
        const size_t off_areas = 16, off_levels = off_areas + ((areas.size() + 15) & ~(size_t)15);
        HIPCHK(h, hipMalloc(h->d_spawn_tables.out(), off_levels + levels.size() + 16));
        HIPCHK(h, hipMemset(h->d_spawn_tables, 0, off_levels + levels.size() + 16));
        HIPCHK(h, hipMemcpy((char *)h->d_spawn_tables.get() + off_areas, areas.data(), areas.size(), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy((char *)h->d_spawn_tables.get() + off_levels, levels.data(), levels.size(), hipMemcpyHostToDevice));
        cfg.stride = (uint32_t)stride;
        cfg.exhausted = (uint32_t *)h->d_spawn_tables.get();
        cfg.areas = (const uint8_t *)h->d_spawn_tables.get() + off_areas;
        cfg.level_of_layout = (const uint8_t *)h->d_spawn_tables.get() + off_levels;
        h->spawn_layouts = h->n_layouts;
    }
    HIPCHK(h, hipMemcpy((char *)h->d_lut.get() + SPAWN_CFG_OFFSET, &cfg, sizeof cfg, hipMemcpyHostToDevice));
    h->P.auto_reset = (h->P.auto_reset & 1) | (on ? 2 : 0);
    h->tables_version++;
    return 0;
}
// respawns that found no free cell of their spawn area within generate_location's 1001 tries (parsing.py:154-167 raises
// ValueError there; the device leaves the agent where it stood) since cz_set_spawn; -1 on error
extern "C" int64_t cz_spawn_exhausted(cz_handle h) {
    if (!h) return -1;
    if (!h->d_spawn_tables) return 0;
    return read_counter<uint32_t>(h, h->d_spawn_tables, "cz_spawn_exhausted");
}
// the draw the device takes (host mirror, for parity tests): uniform in [0, 1), keyed by (seed, global env id, episode << 32 | t,
// agent, draw index)
extern "C" double cz_spawn_uniform(uint64_t seed, int64_t env_global, uint32_t episode, uint32_t t, int32_t agent, uint32_t draw) {
    return spawn_uniform(seed, (uint64_t)env_global, ((uint64_t)episode << 32) | (uint64_t)t, (uint32_t)agent, draw);
}
extern "C" int32_t cz_record_words(cz_handle h) { return h ? h->P.RW : 0; }
extern "C" int cz_sync(cz_handle h) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// device encoding of one node (layout documented at Ops::recipe_marks in cz_device.h); `children` = 0 for wide rows
static int encode_node(cz_handle h, int recipe, uint32_t j, uint32_t hw, uint32_t children, uint32_t *out) {
    const uint32_t cls = hw & 0xFF, cond = (hw >> 8) & 0xFF, counts = (hw >> 24) & 1;
    uint32_t w = children | (counts << 8);
    if (cls < 16) {
        w |= 0x200u | ((cls <= BLENDER ? cls : 7u) << 10);                  // unknown static class: matches nothing
    } else if (cls < 32) {
        // states: 0 fresh, 1 chopped, 2 mashed, 3 both.  Only Carrot / Banana have a blend_state (the reference
        // raises AttributeError when a blend condition meets another class; here such a node matches nothing)
        const bool blender_food = (cls - 16) == CARROT || (cls - 16) == BANANA;
        uint32_t acc;
        if (cond & 0x10u) acc = cond & 0xFu;                               // explicit accept mask (several conditions)
        else if (cond == COND_NONE) acc = 0xFu;
        else if (cond == COND_CHOPPED) acc = 0xAu;
        else if (cond == COND_NOT_CHOPPED) acc = 0x5u;
        else if (cond == COND_MASHED) acc = blender_food ? 0xCu : 0u;
        else if (cond == COND_NOT_MASHED) acc = blender_food ? 0x3u : 0u;
        else return fail(h, "cz_load_recipes: recipe %d node %u: unknown condition code %u", recipe, j, cond);
        w |= 0x2000u | ((cls - 16) << 16) | (acc << 24);
    }
    // (any other class id, e.g. 255 for a name without objects such as "Agent": neither flag, matches nothing)
    *out = w;
    return 0;
}

extern "C" int cz_load_recipes(cz_handle h, const uint32_t *table, int32_t n, int32_t max_nodes) {
    if (!h || !table || n < 1 || n > 255 || (max_nodes != MAX_NODES && max_nodes != WIDE_NODES)) return fail(h, "cz_load_recipes: bad arguments");
    const bool wide = max_nodes == WIDE_NODES;
    const size_t row_words = wide ? 1 + 2 * WIDE_NODES : 1 + MAX_NODES;
    for (int i = 0; i < n; ++i)
        if (table[(size_t)i * row_words] > (uint32_t)max_nodes) return fail(h, "cz_load_recipes: recipe %d has more than %d nodes", i, max_nodes);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (h->d_recipes) HIPCHK(h, hipStreamSynchronize(h->stream));
    h->d_recipes.reset(); h->P.recipes = nullptr;
    size_t bytes = (size_t)n * row_words * 4;
    HIPCHK(h, hipMalloc(h->d_recipes.out(), bytes));
    // device copy: word 0 = node count; node words are re-encoded for the kernels: conditions become an accept mask over
    // the state index chopped | mashed << 1
    std::vector<uint32_t> dev(table, table + (size_t)n * row_words);
    for (int i = 0; i < n; ++i) {
        uint32_t *row = dev.data() + (size_t)i * row_words;
        const uint32_t nn = row[0];
        for (uint32_t j = 0; j < (uint32_t)max_nodes; ++j) {
            if (wide) {
                if (j >= nn) { row[1 + 2 * j] = row[2 + 2 * j] = 0; continue; }
                if (encode_node(h, i, j, row[1 + 2 * j], 0, &row[1 + 2 * j])) return 1;
                row[2 + 2 * j] &= 0xFFFFu;
            } else {
                if (j >= nn) { row[1 + j] = 0; continue; }
                if (encode_node(h, i, j, row[1 + j], (row[1 + j] >> 16) & 0xFF, &row[1 + j])) return 1;
            }
        }
        row[0] = nn & 0xFFu;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_recipes, dev.data(), bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_recipes = n;
    h->P.recipes = h->d_recipes;
    h->tables_version++;
    h->n_partner = 0;                      // the partner table was built from the book this call replaces: cz_load_partner_table again
    h->n_goal_rows = 0;                    // ... and so was the goal table: cz_load_goal_table again
    // (walk_touches and wide, below, are derived from the WHOLE table, not from the recipes some env plays: every id of the table is
    // valid for every step kernel this handle can select, so cz_set_tasks_device may give any env any of them)
    // Carrying an object from cell to cell changes no co-location (hence no recipe mark) when at most two agents
    // exist (they can never share a cell, cooking_world.py:206-221) and no recipe relates a dynamic-class node to a
    // node of a walkable static class (Floor, Switch, Block) -- the only statics a carried object can be "at".
    int sensitive = h->P.A > 2;
    for (int i = 0; i < n && !sensitive; ++i) {
        const uint32_t *row = table + (size_t)i * row_words;
        auto node = [&](uint32_t j) { return wide ? row[1 + 2 * j] : row[1 + j]; };
        auto kids = [&](uint32_t j) { return wide ? (row[2 + 2 * j] & 0xFFFFu) : ((row[1 + j] >> 16) & 0xFFu); };
        for (uint32_t j = 0; j < row[0] && !sensitive; ++j) {
            uint32_t cls = node(j) & 0xFF, children = kids(j);
            for (uint32_t c = 0; c < row[0]; ++c) {
                if (!((children >> c) & 1)) continue;
                uint32_t ccls = node(c) & 0xFF;
                bool pw = cls == FLOOR || cls == SWITCH || cls == BLOCK, cw = ccls == FLOOR || ccls == SWITCH || ccls == BLOCK;
                bool pd = cls >= 16 && cls < 32, cd = ccls >= 16 && ccls < 32;
                if ((pw && cd) || (pd && cw)) sensitive = 1;
            }
        }
    }
    h->P.walk_touches = sensitive;
    h->P.wide = wide ? 1 : 0;
    return 0;
}

// what the kernels rely on in a layout's tables: descriptors whose halfword indices address a slot / cell / agent of this batch
// and whose axis codes exist; records in which a slot that is not alive carries no container tag (Ops::content_of)
static int validate_layouts(cz_handle h, const char *who, const uint32_t *init_records, const uint32_t *obs_desc, int32_t n) {
    for (size_t i = 0; i < (size_t)n * h->P.F; ++i) {
        uint32_t off = obs_desc[i] & 0xFFFFu, code4 = obs_desc[i] >> 16;
        uint32_t hw = off >> 1, code = code4 >> 2;
        bool ok = !(off & 1u) && !(code4 & 3u) && (code <= 2 || (code >= 4 && code < 4 + 2 * (uint32_t)h->P.A));
        const uint32_t cell0 = h->huge ? Img<16>::CELL0 : Img<1>::CELL0, ag0 = h->huge ? Img<16>::AG0 : Img<1>::AG0;
        const uint32_t zero = h->huge ? Img<16>::ZERO : Img<1>::ZERO;
        if (hw < cell0) ok = ok && (int)(hw / 6) < h->P.D;
        else if (hw < ag0) ok = ok && (int)((hw - cell0) / 4) < h->P.W * h->P.H;
        else if (hw < zero) ok = ok && (int)((hw - ag0) / 8) < h->P.A && ((hw - ag0) & 7u) < 7u;
        else ok = ok && hw == zero;
        if (!ok) return fail(h, "%s: bad observation descriptor %#x at %zu", who, obs_desc[i], i);
    }
    for (int32_t l = 0; l < n; ++l) {
        const uint32_t *r = init_records + (size_t)l * h->P.RW;
        for (int s2 = 0; s2 < h->P.D; ++s2)
            if (slot_dead_but_tagged(r[h->P.dyn0_off + s2], r[h->P.dyn1_off + s2]))
                return fail(h, "%s: layout %d: slot %d is not alive but carries a container tag", who, l, s2);
    }
    return 0;
}

extern "C" int cz_load_layouts(cz_handle h, const uint32_t *init_records, const uint32_t *obs_desc, int32_t n) {
    if (!h || !init_records || !obs_desc || n < 1 || n > 65535) return fail(h, "cz_load_layouts: bad arguments");
    if (validate_layouts(h, "cz_load_layouts", init_records, obs_desc, n)) return 1;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->copy_stream) HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    if (h->n_layouts > 0 && n < h->n_layouts) {
        // a smaller pool: the kernels index lay_desc / lay_init with the layout id and the redraw slice of every resident
        // record, so records that point past the new pool would read out of bounds on the next step / observe / auto-reset
        unsigned long long misfits = 0;
        HIPCHK(h, hipMemsetAsync(h->d_stats_part, 0, sizeof misfits, h->stream));
        hipLaunchKernelGGL(k_layout_misfits, dim3((unsigned)((h->P.N + 255) / 256)), dim3(256), 0, h->stream, h->d_state, h->P.RW, h->P.N,
                           (uint32_t)n, h->d_stats_part);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(&misfits, h->d_stats_part, sizeof misfits, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (misfits)
            return fail(h, "cz_load_layouts: %llu resident env record(s) refer to layouts >= %d of the pool being replaced (%d layouts); "
                           "cz_reset / cz_set_state them into the new range first, or load a pool that is not smaller",
                        misfits, n, h->n_layouts);
    }
    h->d_lay_block.reset(); h->d_lay_init = nullptr; h->P.lay_init = nullptr;
    h->d_lay_desc.reset(); h->P.lay_desc = nullptr;
    if (h->rank_stream) HIPCHK(h, hipStreamSynchronize(h->rank_stream));
    h->d_lay_rank.reset();
    h->h_rank_stage.reset();
    h->h_lay_stage.reset();
    size_t b0 = (size_t)n * h->P.RW * 4, b1 = (size_t)n * h->P.F * 4;
    // the records, behind LAY_CTL_WORDS control words (which part of their pool slices the envs draw from: all of it)
    HIPCHK(h, hipMalloc(h->d_lay_block.out(), LAY_CTL_WORDS * 4 + b0));
    h->d_lay_init = h->d_lay_block + LAY_CTL_WORDS;
    HIPCHK(h, hipMalloc(h->d_lay_desc.out(), b1 + 16));                 // + padding: descriptors are fetched in pairs
    HIPCHK(h, hipMemsetAsync(h->d_lay_block, 0, LAY_CTL_WORDS * 4, h->stream));
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)(h->d_lay_block + LC_GROUPS), 1, 1, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_lay_desc, 0, b1 + 16, h->stream));
    const size_t b2 = (size_t)n * h->P.W * h->P.H * sizeof(uint16_t);
    HIPCHK(h, hipMalloc(h->d_lay_rank.out(), b2));
    HIPCHK(h, hipMemsetAsync(h->d_lay_rank, 0, b2, h->stream));
    h->rank_ok.assign((size_t)n, 0);
    h->rank_missing = n;
    HIPCHK(h, hipMemcpyAsync(h->d_lay_init, init_records, b0, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_lay_desc, obs_desc, b1, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_layouts = n;
    // (the spawn tables map every layout of the pool to its level: a new pool - even one of the same size - needs cz_set_spawn again)
    if (h->P.auto_reset & 2) h->spawn_layouts = -1;
    h->lay_groups = 1; h->lay_active = 0; h->upd_ranges.clear(); h->staged_on_copy.clear(); h->staged_on_main.clear(); h->copy_pending = false;
    h->tables_version++;
    h->P.lay_init = h->d_lay_init; h->P.lay_desc = h->d_lay_desc; h->P.L = n;
    return 0;
}

// the staged slot ranges of cz_update_layouts that still wait for their copy.  force = false: copy them (on the copy stream)
// if the steps that were issued before the update have completed, else leave them for a later call; force = true: they have
// to be in place before what the caller issues next - if those steps are still running, copy in order on the handle's stream.
static int flush_updates(cz_handle h, bool force) {
    if (h->upd_ranges.empty()) return 0;
    const hipError_t q = hipEventQuery(h->ev_steps_issued);
    if (q != hipSuccess) (void)hipGetLastError();
    if (q != hipSuccess && !force) return 0;
    const hipStream_t st = q == hipSuccess ? h->copy_stream : h->stream;
    const size_t RWb = (size_t)h->P.RW * 4, Fb = (size_t)h->P.F * 4, L = (size_t)h->n_layouts;
    for (const auto &r : h->upd_ranges) {
        HIPCHK(h, hipMemcpyAsync(h->d_lay_init + (size_t)r.first * h->P.RW, h->h_lay_stage + (size_t)r.first * RWb, (size_t)r.count * RWb,
                                 hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(h->d_lay_desc + (size_t)r.first * h->P.F, h->h_lay_stage + L * RWb + (size_t)r.first * Fb, (size_t)r.count * Fb,
                                 hipMemcpyHostToDevice, st));
    }
    // (who reads which part of the staging block until when: cz_update_layouts waits before it rewrites the same slots)
    // (the events are re-recorded behind ALL copies issued so far on their stream, so the lists only grow until somebody has
    // waited for the event - cz_update_layouts before it rewrites staged slots - or found it complete)
    if (st == h->copy_stream) {
        if (!h->staged_on_copy.empty() && hipEventQuery(h->ev_copy_done) == hipSuccess) h->staged_on_copy.clear();
        (void)hipGetLastError();
        HIPCHK(h, hipEventRecord(h->ev_copy_done, h->copy_stream));
        h->copy_pending = true;
        h->staged_on_copy.insert(h->staged_on_copy.end(), h->upd_ranges.begin(), h->upd_ranges.end());
    } else {
        if (!h->staged_on_main.empty() && hipEventQuery(h->ev_main_copy_done) == hipSuccess) h->staged_on_main.clear();
        (void)hipGetLastError();
        HIPCHK(h, hipEventRecord(h->ev_main_copy_done, h->stream));
        h->staged_on_main.insert(h->staged_on_main.end(), h->upd_ranges.begin(), h->upd_ranges.end());
    }
    h->upd_ranges.clear();
    return 0;
}

// Fresh layouts UNDER A STEPPING BATCH (the reference instantiates a new level at every reset, cooking_env.py:191-195 /
// parsing.py:21-151; the device redraws from a resident pool): replaces pool slots [first, first + count) without touching
// the handle's stream.  The tables stay where they are (nothing the launches captured changes), the new content goes
// through a pinned staging block of the library (the caller's arrays are free again when this returns) and is copied by a
// stream of its own, AFTER every step issued so far has completed (their envs may still read the old content) and not
// waited for by later steps.  The caller must not replace slots that envs can still draw or are still playing on - that is what
// cz_set_layout_group is for: cut every env's pool slice into groups, let the envs draw from one, refresh another once the
// episodes that started on it are over (at most max_steps + 1 steps after the switch), then switch.  The switch waits for
// the copies (on the device, not on the host), so an env only ever draws a slot whose update has completed.
extern "C" int cz_update_layouts(cz_handle h, int32_t first, int32_t count, const uint32_t *init_records, const uint32_t *obs_desc) {
    if (ready(h)) return 1;
    if (first < 0 || count < 0 || first + count > h->n_layouts || (count > 0 && (!init_records || !obs_desc)))
        return fail(h, "cz_update_layouts: slots [%d, %d) outside the resident pool of %d layouts", first, first + count, h ? h->n_layouts : 0);
    if (count > 0 && validate_layouts(h, "cz_update_layouts", init_records, obs_desc, count)) return 1;
    if (set_device(h)) return 1;
    if (caller_capturing(h)) return fail(h, "cz_update_layouts: not inside a stream capture of the caller (it records an event on the captured stream)");
    const size_t RWb = (size_t)h->P.RW * 4, Fb = (size_t)h->P.F * 4, L = (size_t)h->n_layouts;
    if (!h->copy_stream) {
        HIPCHK(h, hipStreamCreateWithFlags(h->copy_stream.out(), hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(h->ev_copy_done.out(), hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(h->ev_steps_issued.out(), hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(h->ev_main_copy_done.out(), hipEventDisableTiming));
    }
    if (!h->h_lay_stage) HIPCHK(h, hipHostMalloc((void **)h->h_lay_stage.out(), L * (RWb + Fb), hipHostMallocDefault));
    if (count == 0) return 0;               // (count 0: only sets up the copy stream and the staging block, ahead of time)
    // The staging block has a place per slot.  Only an earlier copy of THESE slots that is still running, or not even issued,
    // is in the way (with the rotation of cz_set_layout_group consecutive updates go to different parts of the pool).
    auto overlaps = [&](const std::vector<cz_handle_s::SlotRange> &v) {
        for (const auto &r : v)
            if (r.first < first + count && first < r.first + r.count) return true;
        return false;
    };
    if (overlaps(h->upd_ranges) && flush_updates(h, true)) return 1;
    if (overlaps(h->staged_on_copy)) { HIPCHK(h, hipEventSynchronize(h->ev_copy_done)); h->staged_on_copy.clear(); }
    if (overlaps(h->staged_on_main)) { HIPCHK(h, hipEventSynchronize(h->ev_main_copy_done)); h->staged_on_main.clear(); }
    char *const st_rec = h->h_lay_stage + (size_t)first * RWb, *const st_desc = h->h_lay_stage + L * RWb + (size_t)first * Fb;
    memcpy(st_rec, init_records, (size_t)count * RWb);
    memcpy(st_desc, obs_desc, (size_t)count * Fb);
    // The copy must come after every step issued so far (their envs may still read the old content).  A device-side wait of the
    // copy stream for the handle's stream would do - and slow every step kernel down by a microsecond for as long as it is
    // pending (a second hardware queue with an outstanding barrier: measured in round 3, profiles/r03/rot_probe.txt).  So the copy is issued
    // LATER, by whichever call of this handle first finds that those steps have completed (flush_updates), with nothing to
    // wait for on the device.
    HIPCHK(h, hipEventRecord(h->ev_steps_issued, h->stream));
    mark_ranks(h, first, count, 0);       // (cz_load_layout_ranks follows)
    h->upd_ranges.push_back({first, count});
    h->n_layout_updates += count;
    return flush_updates(h, false);
}

// From the next step on (stream order) every env draws its next episode's layout from part `active` of its pool slice cut
// into `groups` equal parts (1, 0: the whole slice, the default).  Every slice's length must be a multiple of `groups`.
// Waits - on the device - for the cz_update_layouts copies issued so far.
extern "C" int cz_set_layout_group(cz_handle h, int32_t groups, int32_t active) {
    if (ready(h)) return 1;
    if (groups < 1 || groups > h->n_layouts || active < 0 || active >= groups || h->n_layouts % groups)
        return fail(h, "cz_set_layout_group: need 1 <= groups, 0 <= active < groups, and pool slices that are multiples of groups");
    if (set_device(h)) return 1;
    if (caller_capturing(h)) {
        // only the switch between the parts of a cut that is already in place, with no cz_update_layouts copy to order: one launch
        if (groups != h->lay_groups || !h->upd_ranges.empty() || h->copy_pending)
            return fail(h, "cz_set_layout_group: not inside a stream capture of the caller (it orders copies and waits) - unless it only "
                           "switches the active part of the cut in place and no cz_update_layouts is outstanding");
        hipLaunchKernelGGL(k_set_layout_active, dim3(1), dim3(64), 0, h->stream, h->d_lay_block, (uint32_t)active);
        HIPCHK(h, hipGetLastError());
        h->lay_active = active;
        return 0;
    }
    if (flush_updates(h, true)) return 1;
    if (h->copy_pending) { HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_copy_done, 0)); h->copy_pending = false; }
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)(h->d_lay_block + LC_GROUPS), groups, 1, h->stream));
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)(h->d_lay_block + LC_ACTIVE), active, 1, h->stream));
    h->lay_groups = groups; h->lay_active = active;
    return 0;
}
// how many pool slots cz_update_layouts has replaced on this handle so far
extern "C" int64_t cz_layout_updates(cz_handle h) { return h ? h->n_layout_updates : 0; }

// ---- fresh layouts drawn ON THE DEVICE (cz_generate.h): the level programs, one per level of the batch, and the level of every
// pool slot.  Checks everything the kernel relies on when it indexes a program: offsets, class codes, candidate counts.
static int validate_program(cz_handle h, int level, const uint32_t *p, int64_t avail) {
    const auto bad = [&](const char *what) { return fail(h, "cz_load_level_programs: level %d: %s", level, what); };
    if (avail < (int64_t)GEN_HEADER_WORDS || p[GH_MAGIC] != GEN_MAGIC) return bad("not a level program");
    const int64_t words = p[GH_WORDS];
    const int64_t CW = ((int64_t)h->P.W * h->P.H + 3) / 4;
    if (words > avail || words < (int64_t)GEN_HEADER_WORDS + CW) return bad("truncated");
    if ((int)p[GH_W] != h->P.W || (int)p[GH_H] != h->P.H || (int)p[GH_A] != h->P.A || (int)p[GH_F] != h->P.F || (int)p[GH_D] != h->P.D)
        return bad("compiled for another batch geometry (grid, agents, slots or feature length)");
    for (int64_t i = 0; i < CW * 4; ++i)
        if (reinterpret_cast<const uint8_t *>(p + GEN_HEADER_WORDS)[i] > COUNTER) return bad("base grid cells must be Floor or Counter");
    int64_t pos = p[GH_OFF_ENTRIES];
    if (pos != (int64_t)GEN_HEADER_WORDS + CW) return bad("entries do not follow the grid");
    const uint32_t n_sd = p[GH_NSTATIC] + p[GH_NDYN], n_all = n_sd + p[GH_NAGENT];
    if (p[GH_NSTATIC] > 65535u || p[GH_NDYN] > 65535u || p[GH_NAGENT] > 65535u) return bad("too many entries");
    for (uint32_t e = 0; e < n_all; ++e) {
        if (pos + (int64_t)GEN_ENTRY_WORDS > words) return bad("entry table overruns the program");
        const uint32_t *q = p + pos;
        const uint32_t cls = q[GE_CLASS], nx = q[GE_NX], ny = q[GE_NY];
        const bool cls_ok = e < p[GH_NSTATIC] ? (cls > COUNTER && cls <= BLENDER)
                            : e < n_sd        ? (cls >= GEN_CODE_DYN0 && cls <= GEN_CODE_DYN0 + BREAD) : cls == GEN_CODE_AGENT;
        if (!cls_ok) return bad("unknown object class");
        if (nx < 1 || nx > GEN_MAX_CANDIDATES || ny < 1 || ny > GEN_MAX_CANDIDATES || q[GE_COUNT] > 65535u) return bad("1..1024 x and y candidates per entry");
        if (pos + (int64_t)GEN_ENTRY_WORDS + nx + ny > words) return bad("candidate lists overrun the program");
        // parsing.py:34, :92, :131 raise on a drawn position < 0 or > width / height (`>`: the far edge itself only never fits)
        for (uint32_t i = 0; i < nx; ++i) if (q[GEN_ENTRY_WORDS + i] > (uint32_t)h->P.W) return bad("x candidate out of bounds set by the level layout");
        for (uint32_t i = 0; i < ny; ++i) if (q[GEN_ENTRY_WORDS + nx + i] > (uint32_t)h->P.H) return bad("y candidate out of bounds set by the level layout");
        pos += (int64_t)GEN_ENTRY_WORDS + nx + ny;
    }
    if (pos != (int64_t)p[GH_OFF_EXCL] || pos + (int64_t)p[GH_NEXCL] != (int64_t)p[GH_OFF_META] || (int64_t)p[GH_OFF_META] + 2 * (int64_t)p[GH_NMETA] != words)
        return bad("sections do not add up to the program length");
    // the meta table fixes the descriptor: its feature lengths (cooking_env.py:114-117) must add up to F
    static const int flen_static[7] = {0, 3, 3, 4, 4, 3, 3}, flen_dyn[10] = {3, 5, 5, 5, 6, 5, 6, 5, 5, 5};
    int64_t F = 0;
    for (uint32_t i = 0; i < p[GH_NMETA]; ++i) {
        const uint32_t code = p[p[GH_OFF_META] + 2 * i], num = p[p[GH_OFF_META] + 2 * i + 1];
        if (num > 65535u) return bad("meta count");
        if (code <= BLENDER) F += (int64_t)flen_static[code] * num;
        else if (code >= GEN_CODE_DYN0 && code <= GEN_CODE_DYN0 + BREAD) F += (int64_t)flen_dyn[code - GEN_CODE_DYN0] * num;
        else if (code == GEN_CODE_AGENT) F += 7 * (int64_t)num;
        else return bad("unknown class in the meta table");
    }
    if (F != h->P.F) return bad("the meta table's feature lengths do not add up to feat_len");
    return 0;
}

extern "C" int cz_load_level_programs(cz_handle h, const uint32_t *programs, int64_t words, int32_t n_levels, const uint8_t *level_of_slot) {
    if (!h) return fail(nullptr, "null handle");
    if (!h->P.lay_init) return fail(h, "cz_load_level_programs: load the layout pool first (every pool slot is given its level)");
    if (!programs || words < 1 || n_levels < 1 || n_levels > 255) return fail(h, "cz_load_level_programs: need 1..255 level programs");
    std::vector<uint32_t> offs;
    int64_t pos = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (validate_program(h, l, programs + pos, words - pos)) return 1;
        offs.push_back((uint32_t)pos);
        pos += programs[pos + GH_WORDS];
    }
    if (pos != words) return fail(h, "cz_load_level_programs: %lld words given, the %d programs hold %lld", (long long)words, n_levels, (long long)pos);
    std::vector<uint8_t> levels;
    if (pool_levels(h, level_of_slot, n_levels, "cz_load_level_programs: slot %d is of level %d, but only %d program(s) were given", levels)) return 1;
    // the pool slice of a slot = the run of consecutive slots of its level (cooking_zoo_amd keeps one contiguous slice per level)
    h->gen_slices.assign((size_t)h->n_layouts, {0, 0});
    for (int i = 0; i < h->n_layouts;) {
        int j = i;
        while (j < h->n_layouts && levels[(size_t)j] == levels[(size_t)i]) ++j;
        for (int k = i; k < j; ++k) h->gen_slices[(size_t)k] = {i, j - i};
        i = j;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->d_gen_tables.reset();
    h->gen_layouts = 0;
    const size_t off_offs = 16, off_prog = off_offs + (((size_t)n_levels * 4 + 15) & ~(size_t)15), off_levels = off_prog + (((size_t)words * 4 + 15) & ~(size_t)15);
    HIPCHK(h, hipMalloc(h->d_gen_tables.out(), off_levels + levels.size() + 16));
    HIPCHK(h, hipMemset(h->d_gen_tables, 0, off_levels + levels.size() + 16));
    HIPCHK(h, hipMemcpy((char *)h->d_gen_tables.get() + off_offs, offs.data(), offs.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy((char *)h->d_gen_tables.get() + off_prog, programs, (size_t)words * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy((char *)h->d_gen_tables.get() + off_levels, levels.data(), levels.size(), hipMemcpyHostToDevice));
    GenParams &G = h->gen;
    G.failures = (uint32_t *)h->d_gen_tables.get();
    G.prog_off = (const uint32_t *)((char *)h->d_gen_tables.get() + off_offs);
    G.programs = (const uint32_t *)((char *)h->d_gen_tables.get() + off_prog);
    G.level_of_slot = (const uint8_t *)h->d_gen_tables.get() + off_levels;
    G.RW = h->P.RW; G.F = h->P.F; G.W = h->P.W; G.H = h->P.H; G.D = h->P.D; G.A = h->P.A; G.dyn0_off = h->P.dyn0_off;
    // the image offsets of the handle's kernel instance (soa.Dims.img_layout): the huge one keeps a larger image
    G.img_obj0 = h->huge ? Img<16>::OBJ0 : Img<1>::OBJ0; G.img_cell0 = h->huge ? Img<16>::CELL0 : Img<1>::CELL0;
    G.img_ag0 = h->huge ? Img<16>::AG0 : Img<1>::AG0; G.img_zero = h->huge ? Img<16>::ZERO : Img<1>::ZERO;
    h->gen_layouts = h->n_layouts;
    return 0;
}

// Pool slots [first, first + count) drawn anew by ONE launch on the handle's stream (parsing.py:5-151 per slot, then
// layout.py's init_record / obs_descriptor): stream-ordered with the steps before and after it and with cz_set_layout_group,
// nothing allocated, copied or waited for - legal inside a stream capture of the caller.
extern "C" int cz_generate_layouts(cz_handle h, int32_t first, int32_t count, uint64_t seed, uint32_t generation) {
    if (ready(h)) return 1;
    if (!h->d_gen_tables || h->gen_layouts != h->n_layouts)
        return fail(h, "cz_generate_layouts: level programs not loaded for this pool (cz_load_level_programs, again after cz_load_layouts)");
    if (first < 0 || count < 0 || (int64_t)first + count > h->n_layouts)
        return fail(h, "cz_generate_layouts: slots [%d, %d) outside the resident pool of %d layouts", first, first + count, h->n_layouts);
    if (count == 0) return 0;
    if (h->lay_groups > 1)          // the envs draw from part `active` of every slice: that part must stay as it is
        for (int s = first; s < first + count; ++s) {
            const auto &sl = h->gen_slices[(size_t)s];
            const int part = sl.count / h->lay_groups;
            if (part > 0 && (s - sl.first) / part == h->lay_active)
                return fail(h, "cz_generate_layouts: slot %d is in part %d of its pool slice, which the envs draw from (cz_set_layout_group)", s, h->lay_active);
        }
    if (set_device(h)) return 1;
    if (caller_capturing(h)) {
        if (!h->upd_ranges.empty() || h->copy_pending)
            return fail(h, "cz_generate_layouts: a cz_update_layouts copy is outstanding, which a stream capture cannot be ordered behind");
    } else {
        // in order behind every cz_update_layouts issued so far
        if (flush_updates(h, true)) return 1;
        if (h->copy_pending) { HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_copy_done, 0)); h->copy_pending = false; }
    }
    if (h->P.RW > (CELL_WORD0 + 256 + 2 * 255 + 15) / 16 * 16) return fail(h, "cz_generate_layouts: record longer than the generator's staging");
    GenParams G = h->gen;
    G.lay_init = h->d_lay_init; G.lay_desc = h->d_lay_desc; G.lay_rank = h->d_lay_rank;
    G.seed = seed; G.generation = generation; G.first = first;
    hipLaunchKernelGGL(k_generate_layouts, dim3((unsigned)count), dim3(64), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
    h->n_layout_updates += count;
    mark_ranks(h, first, count, 1);       // (a failed draw keeps the slot's row as well)
    return 0;
}
// draws that failed since cz_load_level_programs (the reference raises ValueError there; the slot kept its content); -1 on error
extern "C" int64_t cz_generate_failures(cz_handle h) {
    if (!h) return -1;
    if (!h->d_gen_tables) return 0;
    return read_counter<uint32_t>(h, h->d_gen_tables, "cz_generate_failures");
}

// The tail of a call that answers into a host buffer: behind the launch (`rc`: what it returned) the copy of the staged bytes (none
// when `dst` is null), then the wait - also when the launch failed, since host memory the stream may still read must outlive the
// call - and the launch's or the copy's error is reported before the wait's.
static int copy_back_and_wait(cz_handle h, hipError_t rc, void *dst, const void *src, size_t bytes) {
    if (rc == hipSuccess && dst) rc = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t rs = hipStreamSynchronize(h->stream);
    HIPCHK(h, rc);
    HIPCHK(h, rs);
    return 0;
}

// pool slots [first, first + count) have (ok = 1) / have lost (0) the rank rows of their layouts
static void mark_ranks(cz_handle h, int32_t first, int32_t count, int ok) {
    for (int32_t l = first; l < first + count; ++l) {
        h->rank_missing += (int)h->rank_ok[(size_t)l] - ok;
        h->rank_ok[(size_t)l] = (uint8_t)ok;
    }
}
static int check_range(cz_handle h, int64_t b, int64_t c) {
    if (!h) return fail(nullptr, "null handle");
    if (b < 0 || c < 0 || b + c > h->P.N) return fail(h, "env range [%lld, %lld) outside [0, %d)", (long long)b, (long long)(b + c), h->P.N);
    return 0;
}

extern "C" int cz_set_state(cz_handle h, int64_t b, int64_t c, const uint32_t *records) {
    if (check_range(h, b, c)) return 1;
    if (c == 0) return 0;
    if (!records) return fail(h, "cz_set_state: null buffer");
    // the words the kernels use as table indices must be in range (everything else lives in registers / LDS)
    for (int64_t i = 0; i < c; ++i) {
        const uint32_t *r = records + (size_t)i * h->P.RW;
        // (the rules k_restore_where applies on the device, cz_device.h; a rule waits while its table is not loaded)
        uint32_t faults = record_header_faults(r[W_LAYOUT], r[W_RECIPES], r[W_POOL], (uint32_t)h->n_layouts, h->P.R, (uint32_t)h->n_recipes);
        if (h->n_layouts == 0) faults &= ~(HDR_LAYOUT | HDR_POOL);
        if (h->n_recipes == 0) faults &= ~HDR_RECIPE;
        if (faults & HDR_LAYOUT) return fail(h, "cz_set_state: record %lld: layout id %u out of range", (long long)i, r[W_LAYOUT]);
        if (faults & HDR_RECIPE) {
            uint32_t shift = 0;                                      // the first id that is out of range
            while (((r[W_RECIPES] >> shift) & 0xFFu) < (uint32_t)h->n_recipes) shift += 8;
            return fail(h, "cz_set_state: record %lld: recipe id %u out of range", (long long)i, (r[W_RECIPES] >> shift) & 0xFFu);
        }
        if (faults & HDR_POOL) return fail(h, "cz_set_state: record %lld: layout pool slice out of range", (long long)i);
        for (int s2 = 0; s2 < h->P.D; ++s2)
            if (slot_dead_but_tagged(r[h->P.dyn0_off + s2], r[h->P.dyn1_off + s2]))
                return fail(h, "cz_set_state: record %lld: slot %d is not alive but carries a container tag", (long long)i, s2);
    }
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipMemcpyAsync(h->d_state + (size_t)b * h->P.RW, records, (size_t)c * h->P.RW * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int cz_get_state(cz_handle h, int64_t b, int64_t c, uint32_t *records) {
    if (check_range(h, b, c)) return 1;
    if (c == 0) return 0;
    if (!records) return fail(h, "cz_get_state: null buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipMemcpyAsync(records, h->d_state + (size_t)b * h->P.RW, (size_t)c * h->P.RW * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

static int ready(cz_handle h) {
    if (!h) return fail(nullptr, "null handle");
    if (!h->P.recipes) return fail(h, "recipes not loaded (cz_load_recipes)");
    if (!h->P.lay_init) return fail(h, "layouts not loaded (cz_load_layouts)");
    return 0;
}

// What one call asks of a launch: its five buffers, the outputs it names beyond them and, for a fused launch, its span.  Nothing
// call-specific travels through the handle: resolve_step below merges this with the handle's durable settings.
struct StepCall {
    const int32_t *actions; double *obs, *rewards; uint8_t *term, *trunc;
    uint8_t *codes = nullptr;      // the compact observation (cz_step_device_compact, cz_step_compact, cz_rollout_compact)
    float *obs32 = nullptr;        // float32 rows (cz_step_device_f32) or, fused, the float32 trajectory (cz_rollout_f32, cz_rollout_actions_f32)
    uint32_t *marks = nullptr;     // every env's recipe marks (the host step)
    bool fused = false;            // T steps in one launch (the rollouts, fused ring runs); seed and step0 are theirs as well
    int32_t T = 1; uint64_t seed = 0; uint32_t step0 = 0;
    // cz_rollout_policy, cz_rollout_policy_value (fused, float32 only): what the policy adds to the launch (cz_policy.h) - `actions`
    // above stays null, the launch plays no actions of the caller
    const PolicyLaunch *policy = nullptr;
};
// the fused call of a rollout: T steps, the stream's seed and step0, the three outputs every rollout has; the entry point adds its own
static StepCall fused_call(int32_t T, uint64_t seed, uint32_t step0, double *rewards, uint8_t *term, uint8_t *trunc) {
    StepCall c{nullptr, nullptr, rewards, term, trunc};
    c.fused = true; c.T = T; c.seed = seed; c.step0 = step0;
    return c;
}
enum ObsForm { OBS_F64, OBS_CODES, OBS_F32 };      // what a launch writes its observation as (OBS_CODES: float64 rows beside the codes if P.obs)

// The outputs of one launch, in the Params its kernel gets: what the call named, and - one-step launches only - the handle's durable
// setting (cz_set_compact_output, cz_set_f32_output) where the call names no output of that kind (a fused launch writes what its call
// names and nothing of the handle's settings).  The one place that refuses mixed
// outputs (returns the message; nullptr = fine), and the one place that knows the float32 pointer travels in the slot Params::codes shares.
static const char *resolve_step(cz_handle h, const StepCall &c, Params &P, ObsForm &form) {
    uint8_t *const codes = c.fused || c.codes ? c.codes : h->codes;
    float *const obs32 = c.fused || c.obs32 ? c.obs32 : h->obs32;
    if (obs32) {        // the float32 rows stand in for the float64 ones and exclude the compact form (the float32 kernels write nothing else)
        if (codes) return "a float32 output (cz_set_f32_output / cz_step_device_f32) and a compact output (cz_set_compact_output / "
                          "cz_step_device_compact) are both set: switch one of them off";
        if (c.obs) return "float32 observation rows are switched on (cz_set_f32_output): pass d_obs = NULL, or switch them off "
                          "with cz_set_f32_output(h, NULL) to get float64 rows";
    }
    form = obs32 ? OBS_F32 : codes ? OBS_CODES : OBS_F64;
    P = h->P;
    P.actions = c.actions; P.obs = c.obs; P.rewards = c.rewards; P.term = c.term; P.trunc = c.trunc; P.marks_out = c.marks;
    P.T = c.T; P.seed = c.seed; P.step0 = c.step0;
    if (obs32) P.obs32 = obs32; else P.codes = codes;
    return nullptr;
}

// Which kernel a launch gets (the same table is in DESIGN.md section 4).  `form` is resolve_step's; P.wt is decided by then.
//   fused, OBS_F32, a policy call with values -> ROLLOUT_POLICY_VALUE (cz_rollout_policy_value)
//   fused, OBS_F32, a policy call     -> ROLLOUT_POLICY       (cz_rollout_policy)
//   fused, OBS_F32 and P.actions      -> ROLLOUT_ACTIONS_F32  (cz_rollout_actions_f32)
//   fused, OBS_F32                    -> ROLLOUT_F32          (cz_rollout_f32)
//   fused, P.actions                  -> ROLLOUT_ACTIONS      (cz_rollout_actions, fused rings)
//   fused, OBS_CODES without P.obs    -> ROLLOUT_CODES_ONLY   (cz_rollout_compact)
//   fused, OBS_CODES and P.obs        -> ROLLOUT_CODES        (cz_rollout_compact)
//   fused, neither                    -> ROLLOUT              (cz_rollout)
//   one step, OBS_F32                 -> STEP_F32             (cz_step_device_f32, cz_set_f32_output; resolve_step has refused P.obs or codes beside it)
//   one step, OBS_CODES               -> STEP_CODES           (cz_step_device_compact, cz_set_compact_output)
//   one step otherwise                -> STEP, and of that the lean kernel when the handle allows it (CZ_LEAN), the instance has one and
//                                        every setting it fixes at compile time holds: float64 rows of at most 128 * OBS_PAIRS features with
//                                        write-through stores, no marks buffer, narrow recipe tables, no despawn / respawn
//   one step without P.actions        -> hipErrorInvalidValue
static hipError_t choose_step(cz_handle h, const Params &P, const StepCall &call, ObsForm form, StepChoice &c) {
    const bool fused = call.fused;
    c.lean = false;
    c.cfg = -1;
    if (call.policy) {
        c.mode = call.policy->values ? ROLLOUT_POLICY_VALUE : ROLLOUT_POLICY;
        return fused && form == OBS_F32 ? hipSuccess : hipErrorInvalidValue;
    }
    if (fused && form == OBS_F32) c.mode = P.actions ? ROLLOUT_ACTIONS_F32 : ROLLOUT_F32;
    else if (fused) c.mode = P.actions ? ROLLOUT_ACTIONS : form != OBS_CODES ? ROLLOUT : P.obs ? ROLLOUT_CODES : ROLLOUT_CODES_ONLY;
    else c.mode = form == OBS_F32 ? STEP_F32 : form == OBS_CODES ? STEP_CODES : STEP;
    if (c.mode == STEP)
        c.lean = h->lean_enabled && h->kl.has_lean && P.obs && !P.marks_out && !P.wide && !(P.auto_reset & 2) && P.F <= 128 * OBS_PAIRS && P.wt == 1;
    // ... and of the lean kernels the one with the handle's recipe count, end condition and walk_touches fixed, where one exists
    if (c.lean && h->lean_cfg_enabled) c.cfg = lean_cfg_of(P);
    return !fused && !P.actions ? hipErrorInvalidValue : hipSuccess;
}

// The Params of envs [begin, begin + count) of a resolved one-step launch: N = count, the global env ids start `begin` later, and
// every array a one-step kernel indexes by env - records, actions, the outputs in the launch's `form`, marks, statistics - starts
// `begin` rows of its own row size later (a null pointer stays null).  Everything decided on the whole call's N - P.wt, the kernel
// (choose_step) - is decided before this.  `begin` may be any env index: a part's last workgroup may be partial, as a launch's may.
static Params sub_range(const Params &P, ObsForm form, int32_t begin, int32_t count) {
    Params Q = P;
    const size_t b = (size_t)begin, row = (size_t)P.A * (size_t)P.F;
    Q.N = count;
    Q.env_id_base = P.env_id_base + begin;
    Q.state = P.state + b * (size_t)P.RW;
    if (P.actions) Q.actions = P.actions + b * (size_t)P.A;
    if (P.obs) Q.obs = P.obs + b * row;
    if (P.rewards) Q.rewards = P.rewards + b * (size_t)P.A;
    if (P.term) Q.term = P.term + b * (size_t)P.A;
    if (P.trunc) Q.trunc = P.trunc + b * (size_t)P.A;
    if (P.marks_out) Q.marks_out = P.marks_out + b * 2;
    if (form == OBS_F32) Q.obs32 = P.obs32 + b * row;
    else if (P.codes) Q.codes = P.codes + b * (size_t)P.A * (size_t)codes_pitch(P.F);
    Q.stat_u = P.stat_u + b * SU_WORDS;
    Q.stat_f = P.stat_f + b * SF_WORDS;
#ifdef CZ_PROFILE
    if (P.stamps) Q.stamps = P.stamps + b * 16;
#endif
#ifdef CZ_TIMELINE
    if (P.timeline) Q.timeline = P.timeline + b * 2;
#endif
    return Q;
}

// A run of one-step launches as two launch chains (cz_set_ring_split): where part 1 begins and the stream its launches go to.
// launch_step with a RunSplit issues the step's two launches, part 0 on the handle's stream; the run's fork and join are the caller's.
struct RunSplit { int32_t begin1; hipStream_t side; int only = -1; };   // only: 0 / 1 - that part's launch alone (its graph's capture)

static int launch_step(cz_handle h, const StepCall &call, const RunSplit *split = nullptr) {
    if ((h->P.auto_reset & 2) && h->spawn_layouts != h->n_layouts)
        return fail(h, "despawn / respawn is on, but the layout pool was reloaded since cz_set_spawn (now %d layouts): call cz_set_spawn "
                       "again (it maps every layout to the level whose spawn areas it uses)", h->n_layouts);
    const hipStream_t stream = h->stream;
    const bool fused = call.fused;
    Params P;                 // built here, once, from the call and the handle: nothing of an earlier launch can be left in it
    ObsForm form;
    if (const char *refused = resolve_step(h, call, P, form)) return fail(h, "%s", refused);
    const bool f32 = form == OBS_F32;
    // write-through observation stores pay when the launch is short enough for the end-of-kernel L2 write-back to be
    // exposed: one step of a batch of up to ~10 000 envs, whatever its rows weigh (round 6, profiles/r06/wt_sizes.txt: the 2.2 KB
    // rows of the 7x7 levels cross over between 10 240 and 12 288 envs - 43 / 52 MiB -, the 6.7 KB rows of large_16x16 are still
    // ahead at 8192 envs = 210 MiB; until round 5 the rule was "up to 128 MiB", which cost the 7x7 levels 5-9 % from 12 288 to
    // 24 576 envs and large_16x16 2-7 % from 6144 to 8192); streaming stores when one launch's observations do not fit the
    // memory-side cache (256 MiB) any more.  (CZ_WT=0/1/2 overrides, for experiments.)
    // Float32 rows (STEP_F32) take the same rule with 4 bytes per feature.  Its crossover points were measured for float64 rows only:
    // for float32 rows the rule is UNMEASURED (profiles/r10/README.md; tools/f32_sizes.py has the CZ_WT sweep that would settle it).
    const size_t obs_bytes = (size_t)P.N * P.A * P.F * (f32 ? 4 : 8);
    if (!fused) P.wt = obs_bytes > ((size_t)224 << 20) ? 2 : P.N <= 10240 ? 1 : 0;
    // (fused: streaming stores only when an agent's row fills whole DRAM pages - 4 KiB and more, config 5: +8 %; with the
    // 2.2 KB rows of the 7x7 levels they lose 15 % against the cache's own write-back order, profiles/r03/wt_ab2.txt)
    // A float32 trajectory (ROLLOUT_F32, ROLLOUT_ACTIONS_F32) takes the same rule with the row's real bytes, 4 F >= 4096.  Both
    // figures were measured for float64 rows only: for float32 rows the fused rule is UNMEASURED as well.
    else P.wt = (obs_bytes > ((size_t)224 << 20) && (size_t)P.F * (f32 ? 4 : 8) >= 4096) ? 2 : 0;
    if (h->wt_override >= 0) P.wt = h->wt_override;
    if (!fused) {             // the one-step kernels store rewards and flags unconditionally
        if (!P.rewards) P.rewards = (double *)h->d_dump.get();
        if (!P.term) P.term = (uint8_t *)h->d_dump.get();
        if (!P.trunc) P.trunc = (uint8_t *)h->d_dump.get();
    }
#ifdef CZ_TIMELINE
    P.timeline = (h->tl_base && h->tl_cap > 0) ? h->tl_base + (size_t)(h->tl_count++ % h->tl_cap) * (size_t)P.N * 2 : nullptr;
#endif
    // a policy rollout: its borrowed slots of P, and the kernel's block beside it - a copy of P, which nothing writes behind this point
    Params policy_block;
    if (call.policy && !policy_encode(*call.policy, P, policy_block)) return fail(h, "a policy rollout: a pointer that carries a tag (policy_encode) is a device address above 2^48");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (h->ktime && caller_capturing(h)) return fail(h, "kernel timing (cz_kernel_time_reset) cannot run inside a stream capture of the caller");
    if (h->ktime) {
        while (h->kev.size() < h->kev_used + 2) {
            hipEvent_t e;
            HIPCHK(h, hipEventCreate(&e));
            h->kev.emplace_back(e);
        }
        e0 = h->kev[h->kev_used]; e1 = h->kev[h->kev_used + 1];
        h->kev_used += 2;
        HIPCHK(h, hipEventRecord(e0, stream));
    }
    StepChoice choice;
    const hipError_t chosen = choose_step(h, P, call, form, choice);
    h->last_step_lean = choice.lean ? 1 : 0;
    h->last_step_mode = choice.mode;
    h->last_step_variant = !choice.lean ? -1 : choice.cfg < 0 ? 0 : (0x100 | P.R | (P.end_all << 4) | (P.walk_touches << 5));
    HIPCHK(h, chosen);
    if (split && !fused) {
        if (split->only != 1) HIPCHK(h, h->kl.step(sub_range(P, form, 0, split->begin1), stream, choice, nullptr));
        if (split->only != 0) HIPCHK(h, h->kl.step(sub_range(P, form, split->begin1, P.N - split->begin1), split->side, choice, nullptr));
    } else HIPCHK(h, h->kl.step(P, stream, choice, call.policy ? &policy_block : nullptr));
    if (h->ktime) HIPCHK(h, hipEventRecord(e1, stream));
    return 0;
}
extern "C" int cz_reset(cz_handle h, int64_t b, int64_t c, const int32_t *layout_ids, const uint8_t *recipe_ids,
                        const uint32_t *pool_words, double *obs) {
    if (ready(h) || check_range(h, b, c)) return 1;
    if (c == 0) return 0;
    if (!layout_ids || !recipe_ids) return fail(h, "cz_reset: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    std::vector<uint32_t> pools((size_t)c, 0u);
    for (int64_t i = 0; i < c; ++i) {
        if (layout_ids[i] < 0 || layout_ids[i] >= h->n_layouts) return fail(h, "cz_reset: layout id %d out of range", layout_ids[i]);
        for (int r = 0; r < h->P.R; ++r)
            if (recipe_ids[i * 4 + r] >= h->n_recipes) return fail(h, "cz_reset: recipe id %d out of range", recipe_ids[i * 4 + r]);
        if (pool_words) {
            uint32_t base = pool_words[i] & 0xFFFFu, count = pool_words[i] >> 16;
            if (count && (int)(base + count) > h->n_layouts) return fail(h, "cz_reset: layout pool slice [%u,%u) out of range", base, base + count);
            pools[(size_t)i] = pool_words[i];
        }
    }
    // persistent scratch of the handle (cz_create: three words per env; the observation staging is shared with cz_step / cz_observe)
    int32_t *const d_lay = h->d_reset_words;
    uint32_t *const d_rec = (uint32_t *)h->d_reset_words.get() + h->P.N, *const d_pool = (uint32_t *)h->d_reset_words.get() + 2 * (size_t)h->P.N;
    HIPCHK(h, hipMemcpyAsync(d_lay, layout_ids, (size_t)c * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_rec, recipe_ids, (size_t)c * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_pool, pools.data(), (size_t)c * 4, hipMemcpyHostToDevice, h->stream));
    size_t ob = (size_t)c * h->P.A * h->P.F * 8;
    if (obs && !h->d_obs) HIPCHK(h, hipMalloc(h->d_obs.out(), (size_t)h->P.N * h->P.A * h->P.F * 8));
    Params P = h->P;
    hipLaunchKernelGGL(k_count_aborted, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, h->stream, h->d_stat_u, h->d_state, h->P.RW,
                       (long long)b, (int)c);
    const hipError_t rc = h->kl.reset(P, h->stream, b, (int)c, d_lay, d_rec, d_pool, obs ? h->d_obs.get() : nullptr);
    return copy_back_and_wait(h, rc, obs, h->d_obs, ob);            // (pools, a host vector, must outlive its copy)
}

// observe() of the current state (after cz_set_state), host buffer [count][A][F]
extern "C" int cz_observe(cz_handle h, int64_t b, int64_t c, double *obs) {
    if (ready(h) || check_range(h, b, c)) return 1;
    if (c == 0) return 0;
    if (!obs) return fail(h, "cz_observe: null buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    size_t ob = (size_t)c * h->P.A * h->P.F * 8;
    if (!h->d_obs) HIPCHK(h, hipMalloc(h->d_obs.out(), (size_t)h->P.N * h->P.A * h->P.F * 8));
    Params P = h->P;
    return copy_back_and_wait(h, h->kl.observe(P, h->stream, b, (int)c, h->d_obs, nullptr), obs, h->d_obs, ob);
}

// observe() of the current state into DEVICE buffers, float64 rows and / or the compact form (either may be NULL): what a consumer
// that stays on the device needs after cz_reset / cz_set_state, before the first step has written anything.  Stream-ordered,
// no synchronisation (legal inside a stream capture of the caller).
extern "C" int cz_observe_device(cz_handle h, int64_t b, int64_t c, double *d_obs, uint8_t *d_codes) {
    if (begin_ranged_call(h, b, c)) return 1;
    if (c == 0) return 0;
    if (!d_obs && !d_codes) return fail(h, "cz_observe_device: both output pointers are null");
    if (set_device(h)) return 1;
    Params P = h->P;
    P.wt = 0;
    HIPCHK(h, h->kl.observe(P, h->stream, b, (int)c, d_obs, d_codes));
    return 0;
}
// ... the compact form into a host buffer: codes uint8 [count][A][cz_codes_pitch] (cz_obs_table()[code] is the float64 feature)
extern "C" int cz_observe_compact(cz_handle h, int64_t b, int64_t c, uint8_t *codes) {
    if (ready(h) || check_range(h, b, c)) return 1;
    if (c == 0) return 0;
    if (!codes) return fail(h, "cz_observe_compact: null buffer");
    if (set_device(h)) return 1;
    const size_t row = (size_t)h->P.A * codes_pitch(h->P.F);
    if (!h->d_codes_stage) HIPCHK(h, hipMalloc(h->d_codes_stage.out(), (size_t)h->P.N * row));
    Params P = h->P;
    P.wt = 0;
    return copy_back_and_wait(h, h->kl.observe(P, h->stream, b, (int)c, nullptr, (uint8_t *)h->d_codes_stage.get()), codes, h->d_codes_stage, (size_t)c * row);
}

static int set_device(cz_handle h) {
    // hipSetDevice is not free, hipGetDevice is: switch only when the calling thread is on another GPU (the caller, or
    // another handle, may have changed the thread's current device since the last call)
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != h->cfg.device_id) HIPCHK(h, hipSetDevice(h->cfg.device_id));
    return 0;
}

// the archive arguments of cz_save_device / cz_restore_device (`who`), in front of everything that needs the device
static int check_archive(cz_handle h, const char *who, const int32_t *d_slot, const uint32_t *d_records, int64_t capacity) {
    if (!h) return fail(nullptr, "null handle");
    if (!d_records || capacity < 0) return fail(h, "%s: the archive pointer is null or the capacity negative", who);
    if (!d_slot && capacity < h->P.N) return fail(h, "%s: without slots the archive needs a row per env (capacity %lld < %d envs)", who, (long long)capacity, h->P.N);
    return 0;
}
// Begins a call that works on device pointers: the handle is ready, the entry point's own arguments are good (`bad_args`: its message
// otherwise), a fused rollout (`rollout`: the entry point's name) stays inside the span the kernel addresses, the handle's device is
// current, and a staged layout update whose time may have come is flushed - unless the caller is capturing.
static int begin_device_call(cz_handle h, bool args_ok, const char *bad_args, const char *rollout = nullptr, int32_t T = 0) {
    if (ready(h)) return 1;
    if (!args_ok) return fail(h, "%s", bad_args);
    // (the fused kernel addresses rewards / flags / actions with 32-bit offsets from the array base)
    if (rollout && (uint64_t)T * (uint64_t)h->P.N * (uint64_t)h->P.A * 8ull > 0xFFFFFFFFull)
        return fail(h, "%s: T * num_envs * num_agents * 8 must stay below 4 GiB (T <= %llu here): split the rollout", rollout,
                    (unsigned long long)(0xFFFFFFFFull / ((uint64_t)h->P.N * h->P.A * 8ull)));
    if (set_device(h)) return 1;
    if (!h->upd_ranges.empty() && !caller_capturing(h) && flush_updates(h, false)) return 1;
    return 0;
}
// Begins a device-pointer call on the envs [b, b + c): the handle is ready and the range lies inside the batch.  The call's own checks
// follow in its own order, then set_device.
static int begin_ranged_call(cz_handle h, int64_t b, int64_t c) { return ready(h) || check_range(h, b, c); }

// reset() of cooking_env.py:178-210 for chosen envs, decided and carried out on the device: one launch of k_reset_where over the whole
// batch on the handle's stream - no copy, no query, no wait, so it is legal inside a capture of the caller; outside one a staged layout
// update is flushed as by every device-pointer call.  The handle's cz_set_compact_output / cz_set_f32_output settings play no part:
// the call writes the forms it names, rows of the restarted envs only (cooking_env.py:271,352-373), with plain stores.
extern "C" int cz_reset_device(cz_handle h, const uint8_t *d_mask, const int32_t *d_layout_ids, double *d_obs, float *d_obs32,
                               uint8_t *d_codes) {
    if (begin_device_call(h, true, "")) return 1;
    Params P = h->P;
    P.wt = 0;
    HIPCHK(h, h->kl.reset_where(P, h->stream, d_mask, d_layout_ids, d_obs, d_obs32, d_codes, h->d_reset_refused));
    return 0;
}
// envs that cz_reset_device left alone since cz_create because their explicit layout id was >= the pool size (waits for the stream); -1 on error
extern "C" int64_t cz_reset_device_refused(cz_handle h) {
    return h ? read_counter<unsigned long long>(h, h->d_reset_refused, "cz_reset_device_refused") : -1;
}

// An archive of records in device memory, owned by the caller: uint32 [capacity][RW].  cz_save_device gathers records out of the batch
// (k_save_where), cz_restore_device scatters rows back in - many envs may take one row, the fork - and writes the restored envs' first
// observation (k_restore_where).  Each is one launch on the handle's stream: no copy, no query, no wait, legal inside a capture of the
// caller, and no step.  Without a slot array env e and row e belong together, and the archive must hold N rows: checked here, in front
// of everything that needs the device.
extern "C" int cz_save_device(cz_handle h, const int32_t *d_slot, uint32_t *d_records, int64_t capacity) {
    if (check_archive(h, "cz_save_device", d_slot, d_records, capacity) || begin_device_call(h, true, "")) return 1;
    hipLaunchKernelGGL(k_save_where, dim3((unsigned)h->P.N), dim3(64), 0, h->stream, (const uint32_t *)h->d_state, h->P.RW, d_slot, d_records, capacity);
    HIPCHK(h, hipGetLastError());
    return 0;
}
// The handle's cz_set_compact_output / cz_set_f32_output settings play no part: the call writes the forms it names, rows of the
// restored envs only (cooking_env.py:271,352-373), with plain stores.
extern "C" int cz_restore_device(cz_handle h, const int32_t *d_slot, const uint32_t *d_records, int64_t capacity, double *d_obs,
                                 float *d_obs32, uint8_t *d_codes) {
    if (check_archive(h, "cz_restore_device", d_slot, d_records, capacity) || begin_device_call(h, true, "")) return 1;
    Params P = h->P;
    P.wt = 0;
    HIPCHK(h, h->kl.restore_where(P, h->stream, d_slot, d_records, capacity, (uint32_t)h->n_recipes, d_obs, d_obs32, d_codes, h->d_restore_refused));
    return 0;
}
// envs that cz_restore_device left alone since cz_create because their slot was >= capacity or their row failed cz_set_state's checks (waits for the stream); -1 on error
extern "C" int64_t cz_restore_device_refused(cz_handle h) {
    return h ? read_counter<unsigned long long>(h, h->d_restore_refused, "cz_restore_device_refused") : -1;
}

extern "C" int cz_step_device(cz_handle h, const int32_t *d_actions, double *d_obs, double *d_rewards, uint8_t *d_term,
                              uint8_t *d_trunc) {
    if (begin_device_call(h, d_actions, "cz_step_device: actions pointer is null")) return 1;
    return launch_step(h, StepCall{d_actions, d_obs, d_rewards, d_term, d_trunc});
}

// The step with the observation as one byte per feature (and, optionally, the float64 one beside it): see observe() in cz_kernels.h.
extern "C" int cz_step_device_compact(cz_handle h, const int32_t *d_actions, uint8_t *d_codes, double *d_obs, double *d_rewards,
                                      uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, d_actions && d_codes, "cz_step_device_compact: actions and codes pointers must not be null")) return 1;
    StepCall c{d_actions, d_obs, d_rewards, d_term, d_trunc};
    c.codes = d_codes;
    return launch_step(h, c);
}
// From now on EVERY one-step launch of the handle (cz_step_device, _many, _ring, cz_step) also writes the compact observation
// to d_codes (uint8 [N][A][pitch]); NULL switches it off.  With d_obs = NULL in those calls the launches write codes only.
extern "C" int cz_set_compact_output(cz_handle h, uint8_t *d_codes) {
    if (!h) return fail(nullptr, "null handle");
    if (d_codes && h->obs32) return fail(h, "cz_set_compact_output: a float32 output is set (cz_set_f32_output): switch it off first");
    h->codes = d_codes;
    h->tables_version++;                  // (graphs captured for the ring carry the pointer)
    return 0;
}
extern "C" int32_t cz_codes_pitch(cz_handle h) { return h ? codes_pitch(h->P.F) : 0; }

// The step with the observation as FLOAT32 rows (cooking_env.py:271,352-373 in the dtype a policy network takes): d_obs32 float
// [N][A][F], dense, every value np.float32 of the reference's float64 feature (round to nearest even) - a gather from the
// 256-entry table rounded once (cz_obs_table_f32), no arithmetic on values.  Half the observation bytes and no second pass.
extern "C" int cz_step_device_f32(cz_handle h, const int32_t *d_actions, float *d_obs32, double *d_rewards, uint8_t *d_term,
                                  uint8_t *d_trunc) {
    if (begin_device_call(h, d_actions && d_obs32, "cz_step_device_f32: actions and float32 observation pointers must not be null")) return 1;
    StepCall c{d_actions, nullptr, d_rewards, d_term, d_trunc};
    c.obs32 = d_obs32;
    return launch_step(h, c);
}
// From now on EVERY one-step launch of the handle (cz_step_device, _many, _ring, cz_step) called with d_obs = NULL writes the
// float32 rows to d_obs32; NULL switches it off.  Excludes a compact output and a float64 buffer in those calls (resolve_step says so).
extern "C" int cz_set_f32_output(cz_handle h, float *d_obs32) {
    if (!h) return fail(nullptr, "null handle");
    if (d_obs32 && h->codes) return fail(h, "cz_set_f32_output: a compact output is set (cz_set_compact_output): switch it off first");
    h->obs32 = d_obs32;
    h->tables_version++;                  // (graphs captured for the ring carry the pointer)
    return 0;
}
// observe() of the current state as float32 rows [env_count][A][F] into a DEVICE buffer: the first observation of a float32
// consumer after cz_reset / cz_set_state.  Stream-ordered, nothing is synchronised (legal inside a stream capture of the caller).
extern "C" int cz_observe_device_f32(cz_handle h, int64_t b, int64_t c, float *d_obs32) {
    if (begin_ranged_call(h, b, c)) return 1;
    if (c == 0) return 0;
    if (!d_obs32) return fail(h, "cz_observe_device_f32: the output pointer is null");
    if (set_device(h)) return 1;
    Params P = h->P;
    P.wt = 0;
    HIPCHK(h, h->kl.observe_f32(P, h->stream, b, (int)c, d_obs32));
    return 0;
}
// The grid observation of the current state into DEVICE buffers (k_observe_grid, cz_query.h; definition: cooking_zoo_amd/grid.py): any
// of the three forms of the (W, H, C) tensor and the agents' locations, laid out for env_count envs.  Stream-ordered, nothing is copied,
// waited for or queried (legal inside a stream capture of the caller).
extern "C" int32_t cz_grid_channels(int32_t extended) { return extended == 0 ? 32 : extended == 1 ? 48 : -1; }
extern "C" int cz_observe_grid_device(cz_handle h, int64_t b, int64_t c, int32_t extended, uint32_t *d_bits, uint8_t *d_grid8, float *d_grid32,
                                      int32_t *d_agent_xy) {
    if (begin_ranged_call(h, b, c)) return 1;
    if (cz_grid_channels(extended) < 0) return fail(h, "cz_observe_grid_device: extended is %d, not 0 or 1", extended);
    if (c == 0) return 0;
    if (!d_bits && !d_grid8 && !d_grid32 && !d_agent_xy) return fail(h, "cz_observe_grid_device: all four output pointers are null");
    if (((uintptr_t)d_grid8 | (uintptr_t)d_grid32) & 15u || (uintptr_t)d_bits & 7u || (uintptr_t)d_agent_xy & 3u)
        return fail(h, "cz_observe_grid_device: d_grid8 and d_grid32 must be 16-byte aligned, d_bits 8-byte, d_agent_xy 4-byte");
    if (set_device(h)) return 1;
    HIPCHK(h, h->kl.observe_grid(h->P, h->stream, b, (int)c, extended, d_bits, d_grid8, d_grid32, d_agent_xy));
    return 0;
}
// Frames of the current state into DEVICE buffers (k_render, cz_query.h; definition: cooking_zoo_amd/render.py).  cz_load_sprites
// takes the sheet uint8 [cz_render_sprites()][M][M][4] RGBA from HOST memory, uploads it with the table v * (1 / 255) and replaces an earlier
// sheet; it allocates, copies and waits for the stream (not capturable).  cz_render_device is one launch on the env's stream: nothing
// is copied, waited for, queried or allocated (legal inside a stream capture of the caller); the records are only read.
extern "C" int32_t cz_render_sprites(void) { return RENDER_SPRITES; }
extern "C" int cz_load_sprites(cz_handle h, const uint8_t *rgba, int32_t n_sprites, int32_t M) {
    if (ready(h)) return 1;
    if (!rgba) return fail(h, "cz_load_sprites: the sheet pointer is null");
    if (n_sprites != RENDER_SPRITES) return fail(h, "cz_load_sprites: %d sprites, the sheet has %d (cz_render_sprites)", n_sprites, RENDER_SPRITES);
    if (M < 1 || M > RENDER_M_MAX) return fail(h, "cz_load_sprites: M = %d is outside [1, %d]", M, RENDER_M_MAX);
    if (set_device(h)) return 1;
    HIPCHK(h, hipStreamSynchronize(h->stream));                        // (a launch in flight may still read the old sheet)
    h->d_sprites.reset(); h->sprites_M = 0;
    const size_t bytes = (size_t)RENDER_SPRITES * M * M * 4;
    float ftab[256];
    const volatile float inv = 1.0f / 255.0f;                          // render.py: v * (1 / 255) in float32, torch's `x / 255` on the device
    for (int v = 0; v < 256; ++v) ftab[v] = (float)v * inv;
    HIPCHK(h, hipMalloc(h->d_sprites.out(), sizeof ftab + bytes));
    HIPCHK(h, hipMemcpy(h->d_sprites, ftab, sizeof ftab, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy((char *)h->d_sprites.get() + sizeof ftab, rgba, bytes, hipMemcpyHostToDevice));
    h->sprites_M = M;
    return 0;
}
extern "C" int cz_render_device(cz_handle h, int64_t b, int64_t c, int32_t P, uint32_t vis, uint8_t *d_rgb8, float *d_chw32) {
    if (begin_ranged_call(h, b, c)) return 1;
    if (P < RENDER_P_MIN || P > RENDER_P_MAX) return fail(h, "cz_render_device: P = %d is outside [%d, %d]", P, RENDER_P_MIN, RENDER_P_MAX);
    if (!h->sprites_M) return fail(h, "cz_render_device: no sprite sheet is loaded (cz_load_sprites)");
    if (c == 0) return 0;
    if (!d_rgb8 && !d_chw32) return fail(h, "cz_render_device: both output pointers are null");
    if ((uintptr_t)d_rgb8 & 3u || (uintptr_t)d_chw32 & 15u) return fail(h, "cz_render_device: d_rgb8 must be 4-byte aligned, d_chw32 16-byte");
    if (set_device(h)) return 1;
    RenderArgs G{};
    G.env_begin = b;
    G.ftab = (const float *)h->d_sprites.get();
    G.sheet = (const uint32_t *)((const char *)h->d_sprites.get() + 256 * sizeof(float));
    G.rgb8 = d_rgb8; G.chw32 = d_chw32;
    G.P = (uint32_t)P; G.M = (uint32_t)h->sprites_M; G.vis = vis;
    // the reference's own float expressions in its own order (graphic_pipeline.py:46-55, 197-220; render.geometry), every product
    // rounded to double before the next (volatile: nothing is folded or fused)
    const volatile double tile = (double)P, hs = 0.5, cs = 0.7;
    volatile double v;
    v = tile * hs; G.holding = (uint32_t)(int)v;
    v = tile * cs; G.container = (uint32_t)(int)v;
    v = tile * cs; v = v * hs; G.holding_container = (uint32_t)(int)v;
    G.arrow = (uint32_t)P / 4u;
    volatile double one_h = 1.0 - hs, one_c = 1.0 - cs;
    v = tile * one_h; G.holding_off = (uint32_t)(int)v;
    v = tile * one_c; v = v / 2.0; G.container_off = (uint32_t)(int)v;
    volatile double f = one_c / 2.0; f = f * hs; f = one_h + f;
    v = tile * f; G.holding_container_off = (uint32_t)(int)v;
    const uint32_t WP = (uint32_t)h->P.W * (uint32_t)P, per_row = (WP & 3u) ? WP : WP >> 2;
    G.mul_p = (1u << 20) / (uint32_t)P + 1u;
    G.mul_row = (1u << RENDER_ROW_SHIFT) / per_row + 1u;
    HIPCHK(h, h->kl.render(h->P, h->stream, (int)c, G));
    return 0;
}
// Shortest-path navigation on the current state into DEVICE buffers (k_navigate, cz_query.h; definition: cooking_zoo_amd/nav.py):
// first move, path length and / or the whole distance field for every agent and T candidate goals each.  Stream-ordered, nothing is
// copied, waited for or queried (legal inside a stream capture of the caller); the records are only read.
extern "C" int32_t cz_nav_max_targets(void) { return NAV_MAX_TARGETS; }
extern "C" int cz_navigate_device(cz_handle h, int64_t b, int64_t c, int32_t T, uint32_t flags, const int32_t *d_target, int32_t *d_action,
                                  int32_t *d_steps, uint16_t *d_field) {
    if (begin_ranged_call(h, b, c)) return 1;
    if (T < 1 || T > NAV_MAX_TARGETS) return fail(h, "cz_navigate_device: T is %d, not in 1..%d targets per agent", T, NAV_MAX_TARGETS);
    if (flags & ~NAV_KNOWN_FLAGS) return fail(h, "cz_navigate_device: unknown flags bits 0x%x", flags & ~NAV_KNOWN_FLAGS);
    if (c == 0) return 0;
    if (!d_target) return fail(h, "cz_navigate_device: d_target is null");
    if (!d_action && !d_steps && !d_field) return fail(h, "cz_navigate_device: all three output pointers are null");
    if (((uintptr_t)d_target | (uintptr_t)d_action | (uintptr_t)d_steps) & 3u || (uintptr_t)d_field & 1u)
        return fail(h, "cz_navigate_device: d_target, d_action and d_steps must be 4-byte aligned, d_field 2-byte");
    if (set_device(h)) return 1;
    HIPCHK(h, h->kl.navigate(h->P, h->stream, b, (int)c, T, flags, d_target, d_action, d_steps, d_field));
    return 0;
}
// The rank rows of pool slots [first, first + count): uint16 [count][W * H], the position of every cell's static object in
// world_objects[class] (Layout.static_lists) - the list order the scripted partner breaks ties by, which the records do not hold.
// The caller's array is free again when this returns; in place before anything issued later on the handle's stream runs.  Like
// cz_update_layouts only for slots that no env plays on, and not inside a stream capture.
extern "C" int cz_load_layout_ranks(cz_handle h, int32_t first, int32_t count, const uint16_t *ranks) {
    if (ready(h)) return 1;
    if (first < 0 || count < 0 || (int64_t)first + count > h->n_layouts || (count > 0 && !ranks))
        return fail(h, "cz_load_layout_ranks: slots [%d, %d) outside the resident pool of %d layouts", first, first + count, h->n_layouts);
    if (count == 0) return 0;
    const size_t C = (size_t)h->P.W * h->P.H;
    for (size_t k = 0; k < (size_t)count * C; ++k)
        if (ranks[k] >= C) return fail(h, "cz_load_layout_ranks: rank %u at %zu is not below the %zu cells", (unsigned)ranks[k], k, C);
    if (set_device(h)) return 1;
    if (caller_capturing(h)) return fail(h, "cz_load_layout_ranks: not inside a stream capture of the caller (it copies from the host)");
    // through a pinned staging block of the library, on a stream of its own: the caller's thread does not wait for the steps it has
    // issued (a refill under a stepping batch), and what it issues next on the handle's stream waits for the copy on the device
    if (!h->rank_stream) {
        HIPCHK(h, hipStreamCreateWithFlags(h->rank_stream.out(), hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(h->ev_rank_done.out(), hipEventDisableTiming));
    }
    if (!h->h_rank_stage) HIPCHK(h, hipHostMalloc((void **)h->h_rank_stage.out(), (size_t)h->n_layouts * C * sizeof(uint16_t), hipHostMallocDefault));
    else HIPCHK(h, hipEventSynchronize(h->ev_rank_done));             // (the last copy out of the staging block: over long ago)
    uint16_t *const stage = h->h_rank_stage + (size_t)first * C;
    memcpy(stage, ranks, (size_t)count * C * sizeof(uint16_t));
    HIPCHK(h, hipMemcpyAsync(h->d_lay_rank + (size_t)first * C, stage, (size_t)count * C * sizeof(uint16_t), hipMemcpyHostToDevice, h->rank_stream));
    HIPCHK(h, hipEventRecord(h->ev_rank_done, h->rank_stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_rank_done, 0));
    mark_ranks(h, first, count, 1);
    return 0;
}
// The partner table: one row of PARTNER_ROW_WORDS words per recipe of the loaded recipe table, built by the host from the same
// graphs (cooking_zoo_amd/partner.py partner_rows) - the node words the step kernels use keep an accept mask, which loses the
// ORDER of a node's conditions.  Checks everything k_partner relies on.
extern "C" int32_t cz_partner_row_words(void) { return PARTNER_ROW_WORDS; }
extern "C" int cz_load_partner_table(cz_handle h, const uint32_t *rows, int32_t n) {
    if (!h || !rows) return fail(h, "cz_load_partner_table: bad arguments");
    if (n != h->n_recipes) return fail(h, "cz_load_partner_table: %d rows for the %d recipes of the loaded table (cz_load_recipes first)", n, h->n_recipes);
    for (int i = 0; i < n; ++i) {
        const uint32_t *row = rows + (size_t)i * PARTNER_ROW_WORDS, nn = row[0];
        if (nn < 1 || nn > (uint32_t)WIDE_NODES) return fail(h, "cz_load_partner_table: recipe %d has %u nodes, not 1..%d", i, nn, WIDE_NODES);
        for (uint32_t j = 0; j < nn; ++j) {
            const uint32_t a = row[1 + 2 * j], nc = (a >> 8) & 0xFFu, kids = a >> 16;
            if (nc > (uint32_t)PARTNER_MAX_CONDS) return fail(h, "cz_load_partner_table: recipe %d node %u has %u conditions, more than %d", i, j, nc, PARTNER_MAX_CONDS);
            if (kids >> nn || (kids >> j) & 1u) return fail(h, "cz_load_partner_table: recipe %d node %u: bad child mask %#x", i, j, kids);
            for (uint32_t q = 0; q < nc; ++q) {
                const uint32_t cond = (row[2 + 2 * j] >> (4 * q)) & 0xFu, attr = cond & 1u, value = (cond >> 1) & 3u;
                if ((cond >> 3) || value > (attr ? 2u : 1u)) return fail(h, "cz_load_partner_table: recipe %d node %u: bad condition %#x", i, j, cond);
            }
        }
    }
    if (set_device(h)) return 1;
    if (caller_capturing(h)) return fail(h, "cz_load_partner_table: not inside a stream capture of the caller (it allocates and copies)");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->d_partner.reset(); h->n_partner = h->partner_rows_alloc = 0;
    const size_t bytes = (size_t)n * PARTNER_ROW_WORDS * 4, counter = (bytes + 7) / 8 * 8;
    HIPCHK(h, hipMalloc(h->d_partner.out(), counter + 8));
    HIPCHK(h, hipMemsetAsync(h->d_partner, 0, counter + 8, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_partner, rows, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_partner = h->partner_rows_alloc = n;
    return 0;
}
static unsigned long long *partner_counter(cz_handle h) {
    return reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(h->d_partner.get()) + ((size_t)h->partner_rows_alloc * PARTNER_ROW_WORDS * 4 + 7) / 8 * 8);
}
// The scripted partner on the current state into DEVICE buffers (k_partner, cz_query.h; definition: cooking_zoo_amd/partner.py): the
// action the reference's CookingAgent would return for every chosen agent of every env.  Stream-ordered, nothing is copied, waited
// for, queried or allocated (legal inside a stream capture of the caller); the records are only read.
extern "C" int cz_partner_device(cz_handle h, int64_t b, int64_t c, uint32_t agents, uint32_t flags, const int32_t *d_recipe, int32_t *d_action,
                                 int32_t *d_target, uint8_t *d_status) {
    if (begin_ranged_call(h, b, c)) return 1;
    if (agents == 0 || agents >> h->P.A) return fail(h, "cz_partner_device: agents is 0x%x, not a non-empty set of the %d agents", agents, h->P.A);
    if (flags) return fail(h, "cz_partner_device: unknown flags bits 0x%x", flags);
    if (!h->d_partner || h->n_partner == 0 || h->n_partner != h->n_recipes) return fail(h, "cz_partner_device: no partner table for the loaded recipes (cz_load_partner_table)");
    if (h->rank_missing)
        return fail(h, "cz_partner_device: %d pool slot(s) have no rank row (cz_load_layout_ranks after cz_load_layouts / cz_update_layouts)", h->rank_missing);
    if (c == 0) return 0;
    if (!d_action && !d_target && !d_status) return fail(h, "cz_partner_device: all three output pointers are null");
    if (((uintptr_t)d_recipe | (uintptr_t)d_action | (uintptr_t)d_target) & 3u)
        return fail(h, "cz_partner_device: d_recipe, d_action and d_target must be 4-byte aligned");
    if (set_device(h)) return 1;
    PartnerArgs G{b, agents, h->n_partner, d_recipe, h->d_partner, h->d_lay_rank, partner_counter(h), d_action, d_target, d_status};
    HIPCHK(h, h->kl.partner(h->P, h->stream, (int)c, G));
    return 0;
}
// The goal table: the goal id (RecipeNode.id_num, recipe.py:16) of every node of every recipe of the loaded table, 0xFF past a
// recipe's last node, and the length of a goal vector (cooking_env.py:100-105 num_goals).  Checks everything k_infos relies on.
extern "C" int cz_load_goal_table(cz_handle h, const uint8_t *goal_ids, int32_t n, int32_t num_goals) {
    if (!h || !goal_ids) return fail(h, "cz_load_goal_table: bad arguments");
    if (n != h->n_recipes || !h->d_recipes) return fail(h, "cz_load_goal_table: %d rows for the %d recipes of the loaded table (cz_load_recipes first)", n, h->n_recipes);
    if (num_goals < 1 || num_goals > 255) return fail(h, "cz_load_goal_table: num_goals is %d, not in 1..255", num_goals);
    if (set_device(h)) return 1;
    if (caller_capturing(h)) return fail(h, "cz_load_goal_table: not inside a stream capture of the caller (it allocates and copies)");
    // the node counts are the recipe table's (cz_load_recipes keeps them in word 0 of every row)
    const size_t row_words = h->P.wide ? 1 + 2 * WIDE_NODES : 1 + MAX_NODES;
    std::vector<uint32_t> rows((size_t)n * row_words);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(rows.data(), h->d_recipes, rows.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        const uint32_t nn = rows[(size_t)i * row_words] & 0xFFu;
        for (uint32_t j = 0; j < (uint32_t)GOAL_ROW_NODES; ++j) {
            const uint32_t id = goal_ids[(size_t)i * GOAL_ROW_NODES + j];
            if (j < nn ? id >= (uint32_t)num_goals : id != 0xFFu)
                return fail(h, "cz_load_goal_table: recipe %d node %u: goal id %u (a node of the recipe: below num_goals = %d; past its %u nodes: 0xFF)", i, j, id, num_goals, nn);
        }
    }
    h->d_goal.reset(); h->n_goal_rows = 0;
    const size_t bytes = (size_t)n * GOAL_ROW_NODES;
    HIPCHK(h, hipMalloc(h->d_goal.out(), bytes));
    HIPCHK(h, hipMemcpyAsync(h->d_goal, goal_ids, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_goal_rows = n;
    h->num_goals = num_goals;
    return 0;
}
extern "C" int32_t cz_num_goals(cz_handle h) { return h && h->n_goal_rows ? h->num_goals : -1; }
// New recipes for chosen envs, decided and carried out on the device (k_set_tasks, cz_offstep.h; definition: cooking_zoo_amd/tasks.py
// host_set_tasks): one launch over the whole batch on the handle's stream - no copy, no query, no wait, no allocation, so it is legal
// inside a capture of the caller; outside one a staged layout update is flushed as by every device-pointer call.  Not a step and not
// a reset: t, status, episode, statistics and the last-episode row stay.
extern "C" int cz_set_tasks_device(cz_handle h, const uint8_t *d_mask, const uint8_t *d_recipe_ids, const uint8_t *d_task_list, int32_t K,
                                   uint64_t seed) {
    if (ready(h)) return 1;
    if (!d_recipe_ids && !d_task_list) return fail(h, "cz_set_tasks_device: neither recipe ids nor a task list");
    if (!d_recipe_ids && K < 1) return fail(h, "cz_set_tasks_device: a task list of %d rows", K);
    // (rows are read as words; a list beside an id array is ignored, whatever its address)
    if ((uintptr_t)(d_recipe_ids ? d_recipe_ids : d_task_list) & 3u) return fail(h, "cz_set_tasks_device: the source of the ids must be 4-byte aligned");
    if (begin_device_call(h, true, "")) return 1;
    HIPCHK(h, h->kl.set_tasks(h->P, h->stream, d_mask, reinterpret_cast<const uint32_t *>(d_recipe_ids),
                              d_recipe_ids ? nullptr : reinterpret_cast<const uint32_t *>(d_task_list), (uint32_t)(K > 0 ? K : 1), seed,
                              (uint32_t)h->n_recipes, h->d_tasks_refused));
    return 0;
}
// envs that cz_set_tasks_device left alone since cz_create because a new recipe id of a used slot was >= the table's size (waits for the stream); -1 on error
extern "C" int64_t cz_set_tasks_refused(cz_handle h) {
    return h ? read_counter<unsigned long long>(h, h->d_tasks_refused, "cz_set_tasks_refused") : -1;
}
// The task state on the current records into DEVICE buffers (k_infos, cz_query.h; definition: cooking_zoo_amd/tasks.py host_infos).
// Stream-ordered, nothing is copied, waited for, queried or allocated (legal inside a stream capture of the caller); the records are
// only read.
extern "C" int cz_infos_device(cz_handle h, int64_t b, int64_t c, uint8_t *d_goal8, float *d_goal32, uint8_t *d_recipe_done, int32_t *d_task,
                               int32_t *d_t) {
    if (begin_ranged_call(h, b, c)) return 1;
    if (!h->d_goal || h->n_goal_rows == 0 || h->n_goal_rows != h->n_recipes) return fail(h, "cz_infos_device: no goal table for the loaded recipes (cz_load_goal_table)");
    if (!d_goal8 && !d_goal32 && !d_recipe_done && !d_task && !d_t) return fail(h, "cz_infos_device: all five output pointers are null");
    if (((uintptr_t)d_goal32 | (uintptr_t)d_task | (uintptr_t)d_t) & 3u) return fail(h, "cz_infos_device: d_goal32, d_task and d_t must be 4-byte aligned");
    if (c == 0) return 0;
    if (set_device(h)) return 1;
    const InfosArgs G{h->d_state, h->d_recipes, h->d_goal, b, (int32_t)c, h->P.RW, h->P.A, h->num_goals, h->n_recipes,
                      d_goal8, d_goal32, d_recipe_done, d_task, d_t};
    const dim3 grid((unsigned)((c + INFOS_WAVES - 1) / INFOS_WAVES)), block(64 * INFOS_WAVES);
    if (h->P.wide) hipLaunchKernelGGL(k_infos<true>, grid, block, 0, h->stream, G);
    else hipLaunchKernelGGL(k_infos<false>, grid, block, 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
    return 0;
}
// agents that were asked for a recipe index outside the table (they got IDLE) since cz_load_partner_table; -1 on error.  Waits.
extern "C" int64_t cz_partner_bad_recipes(cz_handle h) {
    if (!h || !h->d_partner) return h ? 0 : -1;
    return read_counter<unsigned long long>(h, partner_counter(h), "cz_partner_bad_recipes");
}
// Action effects and masks on the current state into DEVICE buffers (k_action_effects, cz_query.h; definition:
// cooking_zoo_amd/effects.py): for every chosen agent of every env and every action code, what the action would change if the agent
// played it alone.  Stream-ordered, nothing is copied, waited for, queried or allocated (legal inside a stream capture of the caller);
// the records are only read; not a step: counts nothing.
extern "C" int32_t cz_num_actions(cz_handle h) { return h ? (h->P.scheme == 3 ? 5 : 8) : -1; }   // actions.py:17,50
extern "C" int cz_action_effects_device(cz_handle h, int64_t b, int64_t c, uint32_t agents, uint32_t ignore, uint8_t *d_mask, uint8_t *d_effects) {
    if (begin_ranged_call(h, b, c)) return 1;
    if (agents == 0 || agents >> h->P.A) return fail(h, "cz_action_effects_device: agents is 0x%x, not a non-empty set of the %d agents", agents, h->P.A);
    if (ignore & ~FX_ALL) return fail(h, "cz_action_effects_device: unknown ignore bits 0x%x", ignore & ~FX_ALL);
    if (!d_mask && !d_effects) return fail(h, "cz_action_effects_device: both output pointers are null");
    if (c == 0) return 0;
    if (set_device(h)) return 1;
    HIPCHK(h, h->kl.action_effects(h->P, h->stream, (int)c, EffectsArgs{b, agents, ignore, d_mask, d_effects}));
    return 0;
}
// host mirror of the table the float32 rows are gathered from: what the kernels make of the float64 table while they stage it
// (v_cvt_f32_f64, round to nearest even) is what this conversion makes of the host copy
extern "C" int cz_obs_table_f32(cz_handle h, float *table) {
    if (!h || !table) return fail(h, "cz_obs_table_f32: null argument");
    for (int i = 0; i < LUT_SIZE; ++i) table[i] = (float)h->obs_table[i];
    return 0;
}
// diagnostic, not part of cookingzoo.h (tests/test_gpu_lean_step.py): 1 if the most recent step launch issued or captured by the
// handle was the lean one-step kernel, 0 if another kernel, -1 before the first
extern "C" int32_t cz_diag_last_step_lean(cz_handle h) { return h ? h->last_step_lean : -1; }
// diagnostic, not part of cookingzoo.h (tests/test_gpu_kernel_matrix.py): the StepMode (cz_kernels.h) of that launch, -1 before the first
extern "C" int32_t cz_diag_last_step_mode(cz_handle h) { return h ? h->last_step_mode : -1; }
// ... and which lean kernel: -1 none (or no launch yet), 0 k_step_lean, 0x100 | R | end_all << 4 | walk_touches << 5 the k_step_lean_cfg
// with those settings fixed at compile time
extern "C" int32_t cz_diag_last_step_variant(cz_handle h) { return h ? h->last_step_variant : -1; }
// diagnostic, not part of cookingzoo.h (tests/test_gpu_instance_edges.py): the kernel instance the handle's launches use,
// 0 small (Inst<1,1>), 1 large (Inst<2,4>), 2 huge (Inst<4,16>); -1 for a null handle
extern "C" int32_t cz_diag_instance(cz_handle h) { return h ? h->instance : -1; }
// diagnostic, not part of cookingzoo.h (tests/test_gpu_layout_generate_matrix.py): rows [first, first + count) of the resident layout
// pool as the device holds them - init records into `records` [count][record words], observation descriptors into `desc`
// [count][feat_len] (either may be null) - after everything issued on the handle's stream so far.  Reads only.
extern "C" int cz_diag_read_layout_pool(cz_handle h, int32_t first, int32_t count, uint32_t *records, uint32_t *desc) {
    if (ready(h)) return 1;
    if (!h->d_lay_init || !h->d_lay_desc) return fail(h, "cz_diag_read_layout_pool: no layout pool loaded");
    if (first < 0 || count < 0 || (int64_t)first + count > h->n_layouts)
        return fail(h, "cz_diag_read_layout_pool: slots [%d, %d) outside the resident pool of %d layouts", first, first + count, h->n_layouts);
    if (count == 0) return 0;
    if (set_device(h)) return 1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (records)
        HIPCHK(h, hipMemcpy(records, h->d_lay_init + (size_t)first * h->P.RW, (size_t)count * h->P.RW * 4, hipMemcpyDeviceToHost));
    if (desc)
        HIPCHK(h, hipMemcpy(desc, h->d_lay_desc + (size_t)first * h->P.F, (size_t)count * h->P.F * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int cz_obs_table(cz_handle h, double *table) {
    if (!h || !table) return fail(h, "cz_obs_table: null argument");
    memcpy(table, h->obs_table, sizeof h->obs_table);
    return 0;
}
extern "C" const void *cz_obs_table_device(cz_handle h) { return h ? (const void *)h->d_lut.get() : nullptr; }

static bool ring_fusable(cz_handle h, const StepCall &c, int32_t K, int64_t stride);
static int launch_ring_fused(cz_handle h, const StepCall &c, int32_t K, const int32_t *d_ring, int64_t stride, int32_t period, int32_t first_slot);

// SPLIT RUNS (cz_set_ring_split).  A run of one-step launches - cz_step_device_ring, cz_step_device_many - goes out as two launch
// chains over the two halves of the batch, part 0 on the handle's stream and part 1 on a second stream of the handle's: one half
// computes while the other is in its kernel boundary, its ramp or its first round trip to the records.  Envs never interact and every
// array a step touches is indexed by env, so each part is an ordinary launch over its envs (sub_range) and the results are those of
// the whole launches.  The chains are ordered by their streams alone: the second stream waits for an event of the first in front of
// the run (fork) and the first for an event of the second behind it (join) - one fork and join per graph replay or directly launched
// piece, none per step; no wave waits on memory another launch writes.
// A replayed piece is TWO linear graphs, one per chain and stream, between a fork and a join issued with the replay - not one graph
// with two branches: this runtime replays a graph that forks inside at 6.2-7.5 us per step of 4096 envs, against 5.2-5.3 us for the
// unsplit graph and for the two linear ones (profiles/r28/README.md).
// Automatic mode splits the batch sizes at which the split cleared the project's rule - its slowest run faster than the unsplit run's
// fastest, alternated in fresh processes - in the size sweep of profiles/r28/README.md: 4096 to 32768 envs; 1024 and 2048 lose 6 %, and
// nothing above 32768 was measured.  Small instance only: no other was measured.
constexpr int32_t RING_SPLIT_MIN_N = 4096, RING_SPLIT_MAX_N = 32768;
// Which pieces of a run go out as two chains now.  Never split: a run inside a stream capture of the caller (`capturing`), with kernel
// timing on, as fused launches (those never get here), of fewer than two envs, or in a process whose environment holds the runtime
// to fewer than 4 hardware queues.  Mode 2 splits the replayed and the directly launched pieces.  Automatic mode splits the replayed
// ones only: launched directly the host issues two launches per step, and a 20-step region of 4096 envs took 7.0-10.2 us per step
// against 6.1-6.4 us unsplit (8192 envs: 10.3-22.2 against 10.3-10.8, profiles/r28/README.md).
enum : int { SPLIT_GRAPHS = 1, SPLIT_DIRECT = 2 };
static int run_split(cz_handle h, bool capturing) {
    if (h->ring_split == 0 || capturing || h->ktime || h->few_queues || h->P.N < 2) return 0;
    if (h->ring_split == 2) return SPLIT_GRAPHS | SPLIT_DIRECT;
    return h->instance == 0 && h->P.N >= RING_SPLIT_MIN_N && h->P.N <= RING_SPLIT_MAX_N ? SPLIT_GRAPHS : 0;
}
// Part 1 begins at ceil(N / 2), rounded up to whole workgroups where that leaves it an env.  Makes the second stream on first use.
static int split_begin(cz_handle h, RunSplit &s) {
    const int32_t N = h->P.N, epw = h->instance == 2 ? envs_per_wg<16>() : envs_per_wg<1>(), half = (N + 1) / 2;
    const int32_t whole = (half + epw - 1) / epw * epw;
    s.begin1 = whole < N ? whole : half;
    if (!h->split_stream) {
        HIPCHK(h, hipStreamCreateWithFlags(h->split_stream.out(), hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(h->ev_fork.out(), hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(h->ev_join.out(), hipEventDisableTiming));
    }
    s.side = h->split_stream;
    return 0;
}
static int split_fork(cz_handle h) {
    HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->split_stream, h->ev_fork, 0));
    return 0;
}
static int split_join(cz_handle h) {
    HIPCHK(h, hipEventRecord(h->ev_join, h->split_stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
    return 0;
}
// The phase offset of a replayed split run: the first node of the second chain's graph, one wave that sleeps a fixed time and touches
// no memory.  Chains of equal period that start together stay in phase - both halves idle and compute at the same moments -, and how
// far apart they start decides how their live windows interleave for the whole replay: 12 sleeps took 4096 envs from 5.16-5.24 to
// 5.10-5.16 us per step and 6144 envs from 6.42-6.59 to 6.19-6.27, and left 8192 where it was; 20 to 80 sleeps gave the gain back
// (profiles/r28/README.md).
#ifndef CZ_RING_DELAY_SLEEPS
#define CZ_RING_DELAY_SLEEPS 12
#endif
__global__ __launch_bounds__(64) void k_ring_delay() {
#pragma unroll
    for (int i = 0; i < CZ_RING_DELAY_SLEEPS; ++i) __builtin_amdgcn_s_sleep(16);
}
// launches `count` steps over slots [slot, slot + count) directly, as one chain or as two between a fork and a join
static int launch_slots(cz_handle h, StepCall &c, const int32_t *d_ring, int64_t stride, int32_t slot, int32_t count, const RunSplit *split) {
    if (count < 1) return 0;
    if (split && split_fork(h)) return 1;
    int bad = 0;
    for (int32_t j = 0; j < count && !bad; ++j) {
        c.actions = d_ring + (int64_t)(slot + j) * stride;
        bad = launch_step(h, c, split);
    }
    if (split && split_join(h)) return 1;        // (also behind a failed launch: what did go to the second stream is joined)
    return bad;
}
// K consecutive steps, one launch each, issued from C: step k reads actions d_actions + k * action_stride (int32 units,
// wrapping every `action_period` steps) and overwrites the same output buffers.  Same work as K cz_step_device calls
// without K trips through the host language.
extern "C" int cz_step_device_many(cz_handle h, int32_t K, const int32_t *d_actions, int64_t action_stride, int32_t action_period,
                                   double *d_obs, double *d_rewards, uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, d_actions && K >= 1 && action_period >= 1, "cz_step_device_many: bad arguments")) return 1;
    StepCall c{d_actions, d_obs, d_rewards, d_term, d_trunc};
    if (ring_fusable(h, c, K, action_stride)) return launch_ring_fused(h, c, K, d_actions, action_stride, action_period, 0);   // cz_set_ring_fused
    RunSplit split;
    const bool two = (run_split(h, caller_capturing(h)) & SPLIT_DIRECT) != 0;
    if (two && (split_begin(h, split) || split_fork(h))) return 1;
    int bad = 0;
    for (int32_t k = 0; k < K && !bad; ++k) {
        c.actions = d_actions + (int64_t)(k % action_period) * action_stride;
        bad = launch_step(h, c, two ? &split : nullptr);
    }
    if (two && split_join(h)) return 1;
    return bad;
}

// The same K launches for callers that keep their actions in a ring of `period` slots (slot s at d_ring + s * stride):
// step k reads slot (first_slot + k) % period.  A run of consecutive slots is captured once into a HIP graph, keyed by
// (first slot, length), and replayed afterwards: that takes the host out of the loop (0.02 us instead of ~2.5 us of CPU
// per launch) and the kernels read their arguments from memory that is not rewritten before every launch.  A run is cut
// where the ring wraps and at RING_MAX_GRAPH launches; pieces shorter than the handle's graph_min_run (48; CZ_GRAPH_MIN_RUN, clamped to
// 4..RING_MAX_GRAPH) are launched directly.  At
// most RING_CACHE graphs are kept (least recently used goes first), so a caller that keeps asking for new (slot, length)
// pairs pays a capture each time -- keep the runs of a loop aligned.  Results are identical to cz_step_device_many.
constexpr int RING_MAX_GRAPH = 256, RING_CACHE = 64;   // (rocprofv3 --kernel-trace aborts on replays of ~1000 kernel nodes: malformed AQL packet)
// captures the launches of slots [slot, slot + len) on stream `on` (nothing executes) and instantiates them: the whole launches
// (part < 0), or one chain of a split run - part 0 on the handle's stream, part 1 on the second stream, behind the phase offset
static int ring_capture(cz_handle h, StepCall &c, const int32_t *d_ring, int64_t stride, int32_t slot, int32_t len, hipStream_t on,
                        const RunSplit *split, int part, OwnedGraphExec &ge) {
    RunSplit one;
    if (split) { one = *split; one.only = part; }
    OwnedGraph g;
    HIPCHK(h, hipStreamBeginCapture(on, hipStreamCaptureModeThreadLocal));
    if (part == 1 && CZ_RING_DELAY_SLEEPS > 0) hipLaunchKernelGGL(k_ring_delay, dim3(1), dim3(64), 0, on);
    int bad = 0;
    for (int s = 0; s < len && !bad; ++s) {
        c.actions = d_ring + (int64_t)(slot + s) * stride;
        bad = launch_step(h, c, split ? &one : nullptr);
    }
    const hipError_t ec = hipStreamEndCapture(on, g.out());
    if (bad) return 1;
    HIPCHK(h, ec);
    const hipError_t ei = hipGraphInstantiate(ge.out(), g, nullptr, nullptr, 0);
    if (ei != hipSuccess) { (void)ge.release(); HIPCHK(h, ei); }
    return 0;
}
// drops every cached graph (waits for the ones still executing: a split replay ends joined onto the handle's stream)
static void ring_drop(cz_handle h) {
    if (!h->ring_graphs.empty()) (void)hipStreamSynchronize(h->stream);
    h->ring_graphs.clear();
}
static bool ring_select(cz_handle h, const int32_t *d_ring, int64_t stride, int32_t period, double *d_obs, double *d_rewards,
                        uint8_t *d_term, uint8_t *d_trunc, int32_t parts) {
    if (h->ktime || !h->graphs_enabled) return false;
    cz_handle_s::RingKey key;
    key.ring = d_ring; key.stride = stride; key.period = period; key.obs = d_obs; key.rew = d_rewards; key.term = d_term;
    key.trunc = d_trunc; key.stream = h->stream; key.version = h->tables_version; key.parts = parts;
    if (!(key == h->ring_key)) {                   // another ring, other output buffers, new tables or another split: every graph is stale
        ring_drop(h);
        h->ring_key = key;
    }
    return true;
}
// the graph of run [slot, slot + len) - of a split run: the graphs of its two chains -, captured on first use
static int ring_graph(cz_handle h, StepCall &c, const int32_t *d_ring, int64_t stride, int32_t slot, int32_t len, const RunSplit *split,
                      hipGraphExec_t &out, hipGraphExec_t &out2) {
    h->ring_clock++;
    for (auto &r : h->ring_graphs)
        if (r.slot == slot && r.len == len) { r.used = h->ring_clock; out = r.ge; out2 = r.ge2; return 0; }
    if ((int)h->ring_graphs.size() >= RING_CACHE) {
        size_t victim = 0;
        for (size_t i = 1; i < h->ring_graphs.size(); ++i)
            if (h->ring_graphs[i].used < h->ring_graphs[victim].used) victim = i;
        HIPCHK(h, hipStreamSynchronize(h->stream));            // it may still be executing
        h->ring_graphs.erase(h->ring_graphs.begin() + (long)victim);
    }
    cz_handle_s::RunGraph r{slot, len, {}, {}, h->ring_clock};
    if (ring_capture(h, c, d_ring, stride, slot, len, h->stream, split, split ? 0 : -1, r.ge)) return 1;
    if (split && ring_capture(h, c, d_ring, stride, slot, len, split->side, split, 1, r.ge2)) return 1;
    out = r.ge; out2 = r.ge2;
    h->ring_graphs.push_back(std::move(r));
    return 0;
}
// cz_set_ring_fused: the run as fused launches over the ring's own action rows (cz_rollout_actions' kernel, every step's outputs
// written in place), one launch per stretch of consecutive slots.  Needs densely packed slots (stride = num_envs * num_agents).
// (and a run whose one-step launches would write float64 rows or none: the fused kernel has neither codes nor float32 rows in place)
static bool ring_fusable(cz_handle h, const StepCall &c, int32_t K, int64_t stride) {
    Params P;
    ObsForm form;
    return h->ring_fused && K >= 2 && !h->ktime && !resolve_step(h, c, P, form) && form == OBS_F64 && stride == (int64_t)h->P.N * h->P.A;
}
static int launch_ring_fused(cz_handle h, const StepCall &c, int32_t K, const int32_t *d_ring, int64_t stride, int32_t period, int32_t first_slot) {
    // (the kernel addresses the action rows with 32-bit byte offsets from the first row of the launch)
    const Params &P = h->P;
    const int64_t max_T = (int64_t)(0xFFFFFFFFull / ((uint64_t)P.N * (uint64_t)P.A * 4ull));
    if (max_T < 1) return fail(h, "fused ring run: one action row of %d envs x %d agents exceeds the 4 GiB the kernel addresses", P.N, P.A);
    int32_t k = 0;
    while (k < K) {
        const int32_t slot = (int32_t)(((int64_t)first_slot + k) % period);
        int64_t run = K - k;
        if (run > period - slot) run = period - slot;
        if (run > max_T) run = max_T;
        StepCall q = c;
        q.actions = d_ring + (int64_t)slot * stride;
        q.fused = true; q.T = (int32_t)run; q.seed = 0; q.step0 = 1u;          // bit 0: outputs in place
        if (launch_step(h, q)) return 1;
        k += (int32_t)run;
    }
    h->n_ring_fused_steps += K;
    return 0;
}
// walks the run [first_slot, first_slot + K) piece by piece; launch = false only builds the graphs
static int ring_walk(cz_handle h, int32_t K, const int32_t *d_ring, int64_t stride, int32_t period, int32_t first_slot, double *d_obs,
                     double *d_rewards, uint8_t *d_term, uint8_t *d_trunc, bool launch) {
    StepCall c{d_ring, d_obs, d_rewards, d_term, d_trunc};
    if (ring_fusable(h, c, K, stride)) return launch ? launch_ring_fused(h, c, K, d_ring, stride, period, first_slot) : 0;
    // (inside a capture of the caller: plain launches - a capture of the library's own cannot nest in it)
    const bool capturing = caller_capturing(h);
    RunSplit two;
    const int parts = run_split(h, capturing);
    const RunSplit *const split = parts & SPLIT_GRAPHS ? &two : nullptr, *const split_direct = parts & SPLIT_DIRECT ? &two : nullptr;
    if (parts && split_begin(h, two)) return 1;
    const bool graphs = !capturing && ring_select(h, d_ring, stride, period, d_obs, d_rewards, d_term, d_trunc, split ? 2 : 1);
    int32_t k = 0;
    while (k < K) {
        const int32_t slot = (int32_t)(((int64_t)first_slot + k) % period);
        int32_t run = K - k;
        if (run > period - slot) run = period - slot;
        if (run > RING_MAX_GRAPH) run = RING_MAX_GRAPH;
        // Short pieces go out as plain launches: a graph's first kernel starts ~10-16 us after hipGraphLaunch, a directly launched one
        // after ~3-5 us, and the host enqueues a launch (2.8 us) faster than the device runs it - a 20-step region takes 6.7 us per step
        // launched directly against 6.85 us replayed (profiles/r05/k20_modes.txt); long runs are replayed (no host work per launch).
        // Replaying a graph costs the host ~10-16 us before its first kernel starts; a directly launched kernel starts
        // after ~3-5 us.  So the first `ring_prefix` steps of a call's first piece go out as plain launches and keep the GPU busy
        // while the host submits the graph of the rest behind them.
        const int32_t pre = k == 0 ? h->ring_prefix : 0;
        if (graphs && run >= h->graph_min_run + pre) {
            hipGraphExec_t ge = nullptr, ge2 = nullptr;
            if (ring_graph(h, c, d_ring, stride, slot + pre, run - pre, split, ge, ge2)) return 1;
            if (launch) {
                if (launch_slots(h, c, d_ring, stride, slot, pre, split_direct)) return 1;
                if (ge2 && split_fork(h)) return 1;
                HIPCHK(h, hipGraphLaunch(ge, h->stream));
                if (ge2) {
                    HIPCHK(h, hipGraphLaunch(ge2, h->split_stream));
                    if (split_join(h)) return 1;
                }
                h->n_graph_kernels += run - pre;
                h->n_direct_kernels += pre;
            }
        } else if (launch) {
            if (launch_slots(h, c, d_ring, stride, slot, run, split_direct)) return 1;
            h->n_direct_kernels += run;
        }
        k += run;
    }
    return 0;
}
// Builds every graph cz_step_device_ring(K, ..., first_slot, ...) would build lazily, without stepping anything (so that a
// measurement does not pay the one-off capture inside its timed region).
extern "C" int cz_ring_prepare(cz_handle h, int32_t K, const int32_t *d_ring, int64_t stride, int32_t period, int32_t first_slot,
                               double *d_obs, double *d_rewards, uint8_t *d_term, uint8_t *d_trunc) {
    if (ready(h)) return 1;
    if (!d_ring || K < 1 || period < 1 || first_slot < 0 || first_slot >= period) return fail(h, "cz_ring_prepare: bad arguments");
    if (set_device(h)) return 1;
    return ring_walk(h, K, d_ring, stride, period, first_slot, d_obs, d_rewards, d_term, d_trunc, false);
}
extern "C" int cz_step_device_ring(cz_handle h, int32_t K, const int32_t *d_ring, int64_t stride, int32_t period, int32_t first_slot,
                                   double *d_obs, double *d_rewards, uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, d_ring && K >= 1 && period >= 1 && first_slot >= 0 && first_slot < period, "cz_step_device_ring: bad arguments")) return 1;
    return ring_walk(h, K, d_ring, stride, period, first_slot, d_obs, d_rewards, d_term, d_trunc, true);
}
// Runs of cz_step_device_ring / cz_step_device_many as FUSED launches (opt-in): the K steps of a run whose action slots are densely
// packed go out as one launch per stretch of consecutive slots, the env state staying in registers across the steps and every
// step's outputs written to the caller's [N][A] buffers in place - the same final state, outputs and statistics as K launches,
// without launch boundaries.  Returns the previous setting.
extern "C" int cz_set_ring_fused(cz_handle h, int32_t enabled) {
    if (!h) { fail(nullptr, "null handle"); return -1; }
    const int was = h->ring_fused ? 1 : 0;
    h->ring_fused = enabled != 0;
    return was;
}
// Split runs (see run_split): -1 automatic (the default), 0 off, 2 two launch chains; anything else is refused.  Drops the cached ring
// graphs.  Returns the previous mode, -2 on error.
extern "C" int cz_set_ring_split(cz_handle h, int32_t mode) {
    if (!h) { fail(nullptr, "null handle"); return -2; }
    if (mode != -1 && mode != 0 && mode != 2) { fail(h, "cz_set_ring_split: mode %d is none of -1 (automatic), 0 (off), 2 (two parts)", mode); return -2; }
    const int was = h->ring_split;
    if (mode != was && !caller_capturing(h)) {
        if (hipSetDevice(h->cfg.device_id) != hipSuccess) { fail(h, "cz_set_ring_split: hipSetDevice failed"); return -2; }
        ring_drop(h);
    }
    h->ring_split = mode;
    h->tables_version++;
    return was;
}
// in how many launch chains the replayed pieces of a run of this handle go out as things stand (1 or 2; a run inside a capture of the
// caller: always 1)
extern "C" int32_t cz_ring_split_parts(cz_handle h) { return h ? (run_split(h, false) ? 2 : 1) : 0; }
// how many ring graphs the handle holds (tests: what a setting dropped)
extern "C" int32_t cz_diag_ring_graphs(cz_handle h) { return h ? (int32_t)h->ring_graphs.size() : 0; }
extern "C" int64_t cz_ring_fused_steps(cz_handle h, int32_t reset) {
    if (!h) return 0;
    const int64_t n = h->n_ring_fused_steps;
    if (reset) h->n_ring_fused_steps = 0;
    return n;
}
// how many step kernels of this handle were replayed from graphs / launched directly (cz_step_device_ring only);
// reset != 0 zeroes the counters after reading
extern "C" int cz_launch_counts(cz_handle h, int64_t *graph_kernels, int64_t *direct_kernels, int32_t reset) {
    if (!h) return fail(nullptr, "null handle");
    if (graph_kernels) *graph_kernels = h->n_graph_kernels;
    if (direct_kernels) *direct_kernels = h->n_direct_kernels;
    if (reset) h->n_graph_kernels = h->n_direct_kernels = 0;
    return 0;
}

extern "C" int cz_rollout(cz_handle h, int32_t T, uint64_t seed, uint32_t step0, double *d_obs, double *d_rewards,
                          uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, T >= 1, "cz_rollout: T must be >= 1", "cz_rollout", T)) return 1;
    StepCall c = fused_call(T, seed, step0, d_rewards, d_term, d_trunc);
    c.obs = d_obs;
    return launch_step(h, c);
}

// ... with a COMPACT trajectory: d_codes uint8 [T][N][A][cz_codes_pitch] (one byte per feature, see cz_step_device_compact) instead
// of - or, with d_obs, next to - the float64 one: an eighth of the bytes a learner has to read back
extern "C" int cz_rollout_compact(cz_handle h, int32_t T, uint64_t seed, uint32_t step0, uint8_t *d_codes, double *d_obs, double *d_rewards,
                                  uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, T >= 1 && d_codes, "cz_rollout_compact: T must be >= 1 and the codes pointer non-null", "cz_rollout_compact", T)) return 1;
    StepCall c = fused_call(T, seed, step0, d_rewards, d_term, d_trunc);
    c.obs = d_obs; c.codes = d_codes;
    return launch_step(h, c);
}

// The same fused launch over actions of the caller: d_actions int32 [T][N][A], step t of env e reads row t.  What replay and
// open-loop search use instead of T one-step launches: the record stays in registers, every step's outputs land in the
// trajectory buffers, and nothing has to be ordered between launches .
extern "C" int cz_rollout_actions(cz_handle h, int32_t T, const int32_t *d_actions, double *d_obs, double *d_rewards,
                                  uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, T >= 1 && d_actions, "cz_rollout_actions: T must be >= 1 and the actions pointer non-null", "cz_rollout_actions", T)) return 1;
    StepCall c = fused_call(T, 0, 0, d_rewards, d_term, d_trunc);
    c.actions = d_actions; c.obs = d_obs;
    return launch_step(h, c);
}

// The fused launch with the trajectory as FLOAT32 rows (cooking_env.py:243-269 T times, the observation of :352-373 in the dtype a
// policy network takes): d_obs32 float [T][N][A][F], dense, every element np.float32 of the float64 feature as in cz_step_device_f32 -
// k_step<..., ROLLOUT_F32>, which writes no other form of the observation.  State, statistics, rewards and flags are those cz_rollout
// leaves from the same start; the handle's cz_set_compact_output / cz_set_f32_output settings are ignored, as by every rollout.
extern "C" int cz_rollout_f32(cz_handle h, int32_t T, uint64_t seed, uint32_t step0, float *d_obs32, double *d_rewards,
                              uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, T >= 1 && d_obs32, "cz_rollout_f32: T must be >= 1 and the float32 trajectory pointer non-null (without one: "
                                                "cz_rollout with d_obs = NULL)", "cz_rollout_f32", T)) return 1;
    StepCall c = fused_call(T, seed, step0, d_rewards, d_term, d_trunc);
    c.obs32 = d_obs32;
    return launch_step(h, c);
}
// ... over actions of the caller (cooking_env.py:243-269 T times, :352-373): d_actions int32 [T][N][A] as for cz_rollout_actions, every
// step's rows in row t of the trajectory (k_step<..., ROLLOUT_ACTIONS_F32>: there is no in-place form)
extern "C" int cz_rollout_actions_f32(cz_handle h, int32_t T, const int32_t *d_actions, float *d_obs32, double *d_rewards,
                                      uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, T >= 1 && d_actions && d_obs32, "cz_rollout_actions_f32: T must be >= 1 and the actions and float32 trajectory "
                                                             "pointers non-null (without a trajectory: cz_rollout_actions with d_obs = NULL)",
                          "cz_rollout_actions_f32", T)) return 1;
    StepCall c = fused_call(T, 0, 0, d_rewards, d_term, d_trunc);
    c.actions = d_actions; c.obs32 = d_obs32;
    return launch_step(h, c);
}

// ---- the MLP policy (definition: cooking_zoo_amd/policy.py; device code: cz_policy.h, k_policy / k_policy_pack in cz_query.h)
// Loads n_sets weight sets from DEVICE memory in torch.nn.Linear's layouts - W1 float32 [n][64][F], b1 [n][64], W2 [n][C][64], b2 [n][C],
// F the handle's row length and C = cz_num_actions - with one repack launch on the handle's stream.  The table (room for 4 sets) is
// allocated by the handle's first call and never again: every later call is stream-ordered work only and legal inside a capture.
// F and C are fixed by cz_create, so neither cz_load_layouts nor cz_load_recipes drops the table.
extern "C" int cz_load_policy_device(cz_handle h, int32_t n_sets, const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2) {
    if (!h) return fail(nullptr, "null handle");
    if (n_sets < 1 || n_sets > POLICY_MAX_SETS) return fail(h, "cz_load_policy_device: n_sets is %d, not 1..%d", n_sets, POLICY_MAX_SETS);
    if (!d_w1 || !d_b1 || !d_w2 || !d_b2) return fail(h, "cz_load_policy_device: a weight pointer is null");
    if (set_device(h)) return 1;
    const size_t per_set = policy_set_floats(h->P.F);
    if (!h->d_policy) {
        if (caller_capturing(h)) return fail(h, "cz_load_policy_device: the handle's first load allocates the table: call it once outside the capture");
        // (room for the value heads behind the sets: cz_load_value_device; zeroed, so that no launch reads what nobody wrote)
        HIPCHK(h, hipMalloc(h->d_policy.out(), (size_t)policy_table_floats(h->P.F) * sizeof(float)));
        if (!policy_taggable(h->d_policy)) {            // (no device address is: policy_encode would refuse every launch)
            h->d_policy.reset();
            return fail(h, "cz_load_policy_device: device address above 2^48");
        }
        HIPCHK(h, hipMemsetAsync(h->d_policy + policy_value_offset(h->P.F), 0, POLICY_VALUE_FLOATS * sizeof(float), h->stream));
    }
    const uint32_t total = (uint32_t)(per_set * (size_t)n_sets);
    hipLaunchKernelGGL((k_policy_pack<0>), dim3((total + 255u) / 256u), dim3(256), 0, h->stream, h->d_policy, n_sets, h->P.F, cz_num_actions(h),
                       d_w1, d_b1, d_w2, d_b2);
    HIPCHK(h, hipGetLastError());
    h->n_policy_sets = n_sets;
    return 0;
}
extern "C" int32_t cz_policy_sets(cz_handle h) { return h ? h->n_policy_sets : -1; }
// Loads the value heads of sets 0 .. n_sets-1 from DEVICE memory in torch.nn.Linear(64, 1)'s layouts - wv float32 [n][64], bv [n][1] -
// with one repack launch on the handle's stream (legal inside a capture).  The heads live in the policy table's allocation, which
// cz_load_policy_device owns: refused before the first such call.  Heads past n_sets are zeroed.
extern "C" int cz_load_value_device(cz_handle h, int32_t n_sets, const float *d_wv, const float *d_bv) {
    if (!h) return fail(nullptr, "null handle");
    if (n_sets < 1 || n_sets > POLICY_MAX_SETS) return fail(h, "cz_load_value_device: n_sets is %d, not 1..%d", n_sets, POLICY_MAX_SETS);
    if (!d_wv || !d_bv) return fail(h, "cz_load_value_device: a weight pointer is null");
    if (!h->d_policy) return fail(h, "cz_load_value_device: no weight table yet: cz_load_policy_device allocates it");
    if (set_device(h)) return 1;
    hipLaunchKernelGGL((k_value_pack<0>), dim3(1), dim3(320), 0, h->stream, h->d_policy + policy_value_offset(h->P.F), n_sets, d_wv, d_bv);
    HIPCHK(h, hipGetLastError());
    h->n_value_sets = n_sets;
    return 0;
}
extern "C" int32_t cz_value_sets(cz_handle h) { return h ? h->n_value_sets : -1; }
// The agents' bytes of a policy or value call (agent a's set in byte a, 0xFF none): how many agents have a set, or -1 after
// refuse(agent, set) - the caller's fail() - when one asks for a set past the `usable` ones
template <class Refuse>
static int count_sets(cz_handle h, uint32_t bytes, int32_t usable, Refuse &&refuse) {
    int with_set = 0;
    for (int a = 0; a < h->P.A; ++a) {
        const uint32_t s = (bytes >> (8 * a)) & 0xFFu;
        if (s == POLICY_NONE) continue;
        if (s >= (uint32_t)usable) { refuse(a, s); return -1; }
        ++with_set;
    }
    return with_set;
}
// `vsets` of a value call, checked: the packed form, or -1 after fail()
static int64_t check_value_call(cz_handle h, const char *who, uint32_t vsets, int *with_set) {
    if (!h->d_policy || h->n_policy_sets == 0) { fail(h, "%s: no weight table loaded (cz_load_policy_device)", who); return -1; }
    *with_set = count_sets(h, vsets, h->n_policy_sets < h->n_value_sets ? h->n_policy_sets : h->n_value_sets, [&](int a, uint32_t s) {
        fail(h, "%s: agent %d asks for the value head of set %u, but %d sets and %d value heads are loaded", who, a, s, h->n_policy_sets, h->n_value_sets);
    });
    return *with_set < 0 ? -1 : (int64_t)policy_pack_vsets(vsets, h->P.A);
}
// `sets` and `mode` of a policy call, checked: the packed form, or -1 after fail()
static int64_t check_policy_call(cz_handle h, const char *who, uint32_t sets, int32_t mode, bool need_one) {
    if (!h->d_policy || h->n_policy_sets == 0) { fail(h, "%s: no weight table loaded (cz_load_policy_device)", who); return -1; }
    if (mode != (int32_t)POLICY_GREEDY && mode != (int32_t)POLICY_SAMPLE) { fail(h, "%s: mode is %d, not CZ_POLICY_GREEDY (0) or CZ_POLICY_SAMPLE (1)", who, mode); return -1; }
    const int with_set = count_sets(h, sets, h->n_policy_sets, [&](int a, uint32_t s) {
        fail(h, "%s: agent %d asks for weight set %u, but %d are loaded", who, a, s, h->n_policy_sets);
    });
    if (with_set < 0) return -1;
    if (need_one && with_set == 0) { fail(h, "%s: every agent's set is 0xFF (that is cz_rollout_f32)", who); return -1; }
    return (int64_t)policy_pack_sets(sets, (uint32_t)mode, h->P.A);
}
// The policy on rows of the caller: d_obs32 float32 [env_count][A][F] -> d_actions int32 [env_count][A] and / or d_logits float32
// [env_count][A][C].  `sets`: agent a's weight set in byte a, 0xFF = none - that agent's entries are left untouched in both outputs.
// `step` keys the draw of CZ_POLICY_SAMPLE, spawn_uniform(seed, global env id, step, 0x300 + a, 0).  One launch of k_policy on the
// handle's stream: nothing is copied, waited for or allocated (legal inside a stream capture of the caller); no record is touched.
extern "C" int cz_policy_device(cz_handle h, int64_t b, int64_t c, const float *d_obs32, uint32_t sets, int32_t mode, uint64_t seed, uint32_t step,
                                int32_t *d_actions, float *d_logits) {
    if (begin_ranged_call(h, b, c)) return 1;
    const int64_t packed = check_policy_call(h, "cz_policy_device", sets, mode, false);
    if (packed < 0) return 1;
    if (c == 0) return 0;
    if (!d_obs32) return fail(h, "cz_policy_device: the rows pointer is null");
    if (!d_actions && !d_logits) return fail(h, "cz_policy_device: both output pointers are null");
    if (set_device(h)) return 1;
    const int A = h->P.A, F = h->P.F;
    const size_t rows = (size_t)A * (size_t)policy_quads(F) * 16u;
    PolicyArgs G{h->P.env_id_base + b, d_obs32, h->d_policy, F, cz_num_actions(h), (uint32_t)packed, step, seed, d_actions, d_logits};
    HIPCHK(h, with_agents(A, [&](auto na) {
        hipLaunchKernelGGL((k_policy<decltype(na)::value>), dim3((unsigned)c), dim3(64), rows, h->stream, G);
        return hipGetLastError();
    }));
    return 0;
}
// The value heads on rows of the caller (policy.host_value): d_obs32 float32 [rows][A][F] -> d_values float32 [rows][A]; `rows` counts
// [A][F]-rows as in cz_logprob_device and is not tied to the batch.  `vsets`: agent a's value set in byte a, 0xFF = none - that agent's
// entries are left untouched.  One launch of k_value on the handle's stream (legal inside a capture); no record is read.
extern "C" int cz_value_device(cz_handle h, int64_t rows, const float *d_obs32, uint32_t vsets, float *d_values) {
    if (ready(h)) return 1;
    if (rows < 1 || rows > (int64_t)0x7FFFFFFF) return fail(h, "cz_value_device: rows is %lld, not 1..%lld", (long long)rows, (long long)0x7FFFFFFF);
    if (!d_obs32 || !d_values) return fail(h, "cz_value_device: the rows or values pointer is null");
    int with_set = 0;
    const int64_t vpacked = check_value_call(h, "cz_value_device", vsets, &with_set);
    if (vpacked < 0) return 1;
    if (!with_set) return fail(h, "cz_value_device: every agent's byte of vsets is 0xFF");
    if (set_device(h)) return 1;
    const int A = h->P.A, F = h->P.F;
    const size_t lds = (size_t)A * (size_t)policy_quads(F) * 16u;
    const ValueArgs G{d_obs32, h->d_policy, F, (uint32_t)vpacked, d_values};
    HIPCHK(h, with_agents(A, [&](auto na) {
        hipLaunchKernelGGL((k_value<decltype(na)::value>), dim3((unsigned)rows), dim3(64), lds, h->stream, G);
        return hipGetLastError();
    }));
    return 0;
}
// cz_rollout_f32 with the policy in front of every fused step (k_step<..., ROLLOUT_POLICY>): agent a's action at step t is the policy's on
// the env's float32 row before that step - for t = 0 what cz_observe_device_f32 would write at launch, later row t - 1 of the trajectory,
// the row of a reset pass included - with the draw keyed by step0 + t; agents whose byte of `sets` is 0xFF play cz_rollout's stream,
// cz_action(seed, env, a, step0 + t).  d_obs32 float32 [T][N][A][F] is required; d_actions int32 [T][N][A] (every agent's action as
// played) and d_logits float32 [T][N][A][C] (policy agents only) are optional; the rest is cz_rollout_actions_f32 over those actions.
extern "C" int cz_rollout_policy(cz_handle h, int32_t T, uint32_t sets, int32_t mode, uint64_t seed, uint32_t step0, float *d_obs32, int32_t *d_actions,
                                 float *d_logits, double *d_rewards, uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, T >= 1 && d_obs32, "cz_rollout_policy: T must be >= 1 and the float32 trajectory pointer non-null", "cz_rollout_policy", T)) return 1;
    const int64_t packed = check_policy_call(h, "cz_rollout_policy", sets, mode, true);
    if (packed < 0) return 1;
    const PolicyLaunch L{d_actions, d_logits, h->d_policy, (uint32_t)packed};
    StepCall c = fused_call(T, seed, step0, d_rewards, d_term, d_trunc);
    c.obs32 = d_obs32; c.policy = &L;
    return launch_step(h, c);
}
// cz_rollout_policy plus the value heads (k_step<..., ROLLOUT_POLICY_VALUE>): d_values float32 [T + 1][N][A], required.  Row t holds the
// value of agent a's set in byte a of `vsets` (0xFF: none, entries untouched) on the row the policy reads in front of step t, row T the
// value on the row step T - 1 staged - the row a following launch's step 0 reads - so d_values goes into cz_gae_device as it is.
// `vsets` is independent of `sets`; every agent may be at 0xFF in `sets` (values under the action stream) as long as one has a value
// set.  Everything else is what cz_rollout_policy leaves for the same arguments.
extern "C" int cz_rollout_policy_value(cz_handle h, int32_t T, uint32_t sets, uint32_t vsets, int32_t mode, uint64_t seed, uint32_t step0, float *d_obs32,
                                       int32_t *d_actions, float *d_logits, float *d_values, double *d_rewards, uint8_t *d_term, uint8_t *d_trunc) {
    if (begin_device_call(h, T >= 1 && d_obs32 && d_values, "cz_rollout_policy_value: T must be >= 1 and the float32 trajectory and values pointers non-null",
                          "cz_rollout_policy_value", T)) return 1;
    if (!policy_taggable(d_values)) return fail(h, "cz_rollout_policy_value: the values pointer is a device address above 2^48");
    const int64_t packed = check_policy_call(h, "cz_rollout_policy_value", sets, mode, false);
    if (packed < 0) return 1;
    int with_value = 0;
    const int64_t vpacked = check_value_call(h, "cz_rollout_policy_value", vsets, &with_value);
    if (vpacked < 0) return 1;
    if (!with_value && ((uint32_t)packed & 0xFFFu) == 0xFFFu) return fail(h, "cz_rollout_policy_value: every agent is at 0xFF in both sets and vsets (that is cz_rollout_f32)");
    const PolicyLaunch L{d_actions, d_logits, h->d_policy, (uint32_t)packed, d_values, (uint32_t)vpacked};
    StepCall c = fused_call(T, seed, step0, d_rewards, d_term, d_trunc);
    c.obs32 = d_obs32; c.policy = &L;
    return launch_step(h, c);
}

// ---- what a learner trains on (definition: cooking_zoo_amd/targets.py; k_gae / k_logprob in cz_query.h).  Both calls work on dense
// arrays of the caller whose extents the caller names - a shard or a slice passes its own - and are one launch on the handle's stream:
// nothing is copied, waited for or allocated (legal inside a stream capture of the caller); no record is read.
template <int D, int WG>
static hipError_t launch_gae(hipStream_t stream, const GaeArgs &G) {
    hipLaunchKernelGGL((k_gae<D, WG>), dim3((unsigned)((G.n + WG - 1) / WG)), dim3(WG), 0, stream, G);
    return hipGetLastError();
}
// Generalised advantage estimation over [T][env_count][A] series, t descending, in float64 (targets.host_gae): d_values float32
// [T + 1][env_count][A] holds the critic on the state before step t in row t and the bootstrap in row T; a termination or truncation
// at t cuts both the bootstrap and the carry.  Series of agents outside `agents` are neither read nor written.
extern "C" int cz_gae_device(cz_handle h, int32_t T, int64_t env_count, const double *d_rewards, const uint8_t *d_term, const uint8_t *d_trunc,
                             const float *d_values, double gamma, double lambda, uint32_t agents, float *d_adv, float *d_ret) {
    if (ready(h)) return 1;
    const int A = h->P.A;
    if (T < 1) return fail(h, "cz_gae_device: T is %d, not >= 1", T);
    if (env_count < 1 || env_count > (int64_t)0x7FFFFFFF * 64 / A) return fail(h, "cz_gae_device: env_count is %lld, not 1..%lld", (long long)env_count, (long long)((int64_t)0x7FFFFFFF * 64 / A));
    if (!d_rewards || !d_term || !d_values) return fail(h, "cz_gae_device: the rewards, terminations or values pointer is null");
    if (!d_adv && !d_ret) return fail(h, "cz_gae_device: both output pointers are null");
    if (!(agents & ((1u << A) - 1u))) return fail(h, "cz_gae_device: agents is 0x%x: none of the %d agents", agents, A);
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(h, "cz_gae_device: gamma is %g, not in [0, 1]", gamma);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(h, "cz_gae_device: lambda is %g, not in [0, 1]", lambda);
    if (set_device(h)) return 1;
    const GaeArgs G{env_count * A, T, A, agents, d_rewards, d_term, d_trunc, d_values, gamma, gamma * lambda, d_adv, d_ret};
    hipError_t e = hipErrorInvalidValue;
    switch (h->gae_shape) {
    case 2064: e = launch_gae<2, 64>(h->stream, G); break;
    case 4064: e = launch_gae<4, 64>(h->stream, G); break;
    case 8064: e = launch_gae<8, 64>(h->stream, G); break;
    case 16064: e = launch_gae<16, 64>(h->stream, G); break;
    case 2256: e = launch_gae<2, 256>(h->stream, G); break;
    case 4256: e = launch_gae<4, 256>(h->stream, G); break;
    case 8256: e = launch_gae<8, 256>(h->stream, G); break;
    case 16256: e = launch_gae<16, 256>(h->stream, G); break;
    default: return fail(h, "cz_gae_device: CZ_GAE_SHAPE names %d rows ahead x %d threads; the library carries 2, 4, 8, 16 x 64, 256", h->gae_shape / 1000, h->gae_shape % 1000);
    }
    HIPCHK(h, e);
    return 0;
}
// Log-probability of the action played and entropy of the softmax CZ_POLICY_SAMPLE draws from (targets.host_logprob): d_logits float32
// [rows][A][C], d_actions int32 [rows][A] -> d_logp and / or d_entropy float32 [rows][A]; an action outside 0 .. C-1 gets 0.0.  Agents
// whose byte of `sets` is 0xFF are left untouched in both outputs (cz_policy_device's convention: their logits were never written).
extern "C" int cz_logprob_device(cz_handle h, int64_t rows, const float *d_logits, const int32_t *d_actions, uint32_t sets, float *d_logp,
                                 float *d_entropy) {
    if (ready(h)) return 1;
    const int A = h->P.A;
    if (rows < 1 || rows > (int64_t)0x7FFFFFFF * 256 / A) return fail(h, "cz_logprob_device: rows is %lld, not 1..%lld", (long long)rows, (long long)((int64_t)0x7FFFFFFF * 256 / A));
    if (!d_logits || !d_actions) return fail(h, "cz_logprob_device: the logits or actions pointer is null");
    if (!d_logp && !d_entropy) return fail(h, "cz_logprob_device: both output pointers are null");
    int chosen = 0;
    for (int a = 0; a < A; ++a) chosen += ((sets >> (8 * a)) & 0xFFu) != POLICY_NONE;
    if (!chosen) return fail(h, "cz_logprob_device: every agent's byte of sets is 0xFF");
    if (set_device(h)) return 1;
    const LogprobArgs G{rows * A, A, sets, d_logits, d_actions, d_logp, d_entropy};
    const dim3 grid((unsigned)((G.total + 255) / 256));
    if (cz_num_actions(h) == 5) hipLaunchKernelGGL((k_logprob<5>), grid, dim3(256), 0, h->stream, G);
    else hipLaunchKernelGGL((k_logprob<8>), grid, dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---- PPO's gradients (definition: cooking_zoo_amd/ppo.py; k_ppo_forward / k_ppo_outer / k_ppo_reduce in cz_query.h)
// The workspace of a call over `positions` positions and `n_sets` loaded sets, carved from `base` into G -> its size in bytes
static size_t ppo_carve(unsigned char *base, int64_t positions, int A, int F, int n_sets, PpoArgs &G) {
    const size_t pairs = (size_t)positions * (size_t)A, slots = pairs * 2u, chunks = (size_t)((positions + PPO_CHUNK - 1) / PPO_CHUNK);
    size_t at = 0;
    const auto take = [&](auto *&field, size_t count) {
        using T = std::remove_reference_t<decltype(*field)>;
        field = reinterpret_cast<T *>(base + at);
        at += (count * sizeof(T) + 255u) & ~(size_t)255u;
    };
    take(G.terms, pairs * PPO_TERMS);
    take(G.chunk_stats, chunks * PPO_TERMS);
    take(G.hid, slots * POLICY_HIDDEN);
    take(G.da, slots * POLICY_HIDDEN);
    take(G.small, slots * PPO_SMALL);
    take(G.partial, chunks * (size_t)n_sets * ppo_set_floats(F));
    return at;
}
// the most positions a call may name: (position, agent) pairs and their rows stay within 31 bits
static int64_t ppo_max_positions(cz_handle h) { return (int64_t)0x3FFFFFFF / h->P.A; }
// Allocates the workspace of cz_ppo_grad_device for minibatches of up to max_positions positions over the sets loaded now: per (position,
// agent) two pass slots (hidden vector, da, the scalars) and the statistics' terms, per (chunk of 64 positions, loaded set) one partial
// gradient.  Outside a capture; a call that asks for no more than is reserved does nothing (and is legal anywhere).
extern "C" int cz_ppo_reserve(cz_handle h, int64_t max_positions) {
    if (ready(h)) return 1;
    if (!h->d_policy || h->n_policy_sets == 0) return fail(h, "cz_ppo_reserve: no weight table loaded (cz_load_policy_device): the workspace is sized by the loaded sets");
    if (max_positions < 1 || max_positions > ppo_max_positions(h)) return fail(h, "cz_ppo_reserve: max_positions is %lld, not 1..%lld", (long long)max_positions, (long long)ppo_max_positions(h));
    if (max_positions <= h->ppo_positions && h->n_policy_sets <= h->ppo_sets) return 0;
    if (caller_capturing(h)) return fail(h, "cz_ppo_reserve: %lld positions over %d sets need an allocation: call it outside the capture", (long long)max_positions, h->n_policy_sets);
    if (set_device(h)) return 1;
    const int64_t positions = max_positions > h->ppo_positions ? max_positions : h->ppo_positions;
    const int32_t n_sets = h->n_policy_sets > h->ppo_sets ? h->n_policy_sets : h->ppo_sets;
    PpoArgs G{};
    const size_t bytes = ppo_carve(nullptr, positions, h->P.A, h->P.F, n_sets, G);
    HIPCHK(h, hipStreamSynchronize(h->stream));        // (a call issued earlier may still be using the old workspace)
    h->ppo_positions = 0;
    h->ppo_sets = 0;
    HIPCHK(h, hipMalloc(h->d_ppo.out(), bytes));
    h->ppo_positions = positions;
    h->ppo_sets = n_sets;
    return 0;
}
extern "C" int64_t cz_ppo_reserved(cz_handle h) { return h ? h->ppo_positions : -1; }
extern "C" int32_t cz_ppo_chunk(void) { return PPO_CHUNK; }
// The gradient of PPO's clipped-surrogate loss with value and entropy terms over a minibatch of a trajectory in device memory
// (ppo.host_ppo_grad): d_obs32 float32 [rows][A][F], d_actions int32 [rows][A], d_logp_old / d_adv / d_ret float32 [rows][A]; d_index int32
// [positions] names the minibatch's rows (NULL: positions == rows, row m), an index outside 0 .. rows-1 contributes nothing and is
// counted in d_stats[7].  `sets` / `vsets` as in cz_rollout_policy_value.  The gradients come in torch.nn.Linear's layouts behind a
// leading axis of cz_policy_sets(h): d_gw1 [n][64][F], d_gb1 [n][64], d_gw2 [n][C][64], d_gb2 [n][C], d_gwv [n][64], d_gbv [n][1]; sets no
// agent uses get zeros.  d_stats float64 [8] (may be NULL).  Three launches on the handle's stream: nothing is copied, waited for or
// allocated (legal inside a stream capture of the caller); no record is read.
extern "C" int cz_ppo_grad_device(cz_handle h, int64_t rows, int64_t positions, const int32_t *d_index, const float *d_obs32, const int32_t *d_actions,
                                  const float *d_logp_old, const float *d_adv, const float *d_ret, uint32_t sets, uint32_t vsets, double clip,
                                  double c_value, double c_entropy, float *d_gw1, float *d_gb1, float *d_gw2, float *d_gb2, float *d_gwv, float *d_gbv,
                                  double *d_stats) {
    if (ready(h)) return 1;
    const int A = h->P.A, F = h->P.F;
    const int64_t packed = check_policy_call(h, "cz_ppo_grad_device", sets, (int32_t)POLICY_GREEDY, false);
    if (packed < 0) return 1;
    int with_value = 0;
    int64_t vpacked = (int64_t)policy_pack_vsets(0xFFFFFFFFu, A);
    bool any_value = false;
    for (int a = 0; a < A; ++a) any_value |= ((vsets >> (8 * a)) & 0xFFu) != POLICY_NONE;
    if (any_value) {                  // (without a critic no value head need be loaded)
        vpacked = check_value_call(h, "cz_ppo_grad_device", vsets, &with_value);
        if (vpacked < 0) return 1;
    }
    int with_policy = 0;
    uint32_t used = 0;
    for (int a = 0; a < A; ++a) {
        const uint32_t s = (sets >> (8 * a)) & 0xFFu, vs = (vsets >> (8 * a)) & 0xFFu;
        if (s != POLICY_NONE) { ++with_policy; used |= 1u << s; }
        if (vs != POLICY_NONE) used |= 1u << vs;
    }
    if (!with_policy && !with_value) return fail(h, "cz_ppo_grad_device: every agent is at 0xFF in both sets and vsets");
    if (rows < 1 || rows > ppo_max_positions(h)) return fail(h, "cz_ppo_grad_device: rows is %lld, not 1..%lld", (long long)rows, (long long)ppo_max_positions(h));
    if (positions < 1) return fail(h, "cz_ppo_grad_device: positions is %lld, not >= 1", (long long)positions);
    if (positions > h->ppo_positions) return fail(h, "cz_ppo_grad_device: %lld positions, but the workspace holds %lld (cz_ppo_reserve)", (long long)positions, (long long)h->ppo_positions);
    if (h->n_policy_sets > h->ppo_sets) return fail(h, "cz_ppo_grad_device: %d sets are loaded, but the workspace was reserved for %d (cz_ppo_reserve again)", h->n_policy_sets, h->ppo_sets);
    if (!d_index && positions != rows) return fail(h, "cz_ppo_grad_device: without an index positions (%lld) must equal rows (%lld)", (long long)positions, (long long)rows);
    if (!d_obs32 || !d_actions || !d_logp_old || !d_adv || !d_ret) return fail(h, "cz_ppo_grad_device: the rows, actions, logp_old, advantages or returns pointer is null");
    if (!d_gw1 || !d_gb1 || !d_gw2 || !d_gb2) return fail(h, "cz_ppo_grad_device: a gradient pointer of the policy's four tensors is null");
    if (with_value && (!d_gwv || !d_gbv)) return fail(h, "cz_ppo_grad_device: a value set is named, but a value-gradient pointer is null");
    if (!(clip >= 0.0)) return fail(h, "cz_ppo_grad_device: clip is %g, not >= 0", clip);
    if (!(c_value >= 0.0)) return fail(h, "cz_ppo_grad_device: c_value is %g, not >= 0", c_value);
    if (!(c_entropy >= 0.0)) return fail(h, "cz_ppo_grad_device: c_entropy is %g, not >= 0", c_entropy);
    if (h->ppo_tile != 16 && h->ppo_tile != 32 && h->ppo_tile != 64) return fail(h, "cz_ppo_grad_device: CZ_PPO_TILE names %d features; the library carries 16, 32 and 64", h->ppo_tile);
    if (set_device(h)) return 1;
    PpoArgs G{};
    G.rows = rows; G.positions = (int32_t)positions; G.A = A; G.F = F; G.C = cz_num_actions(h); G.n_sets = h->n_policy_sets;
    G.packed = (uint32_t)packed; G.vpacked = (uint32_t)vpacked; G.used = used;
    G.index = d_index; G.obs32 = d_obs32; G.actions = d_actions; G.logp_old = d_logp_old; G.adv = d_adv; G.ret = d_ret;
    G.table = h->d_policy;
    G.K.inv_p = with_policy ? 1.0 / (double)(positions * with_policy) : 0.0;
    G.K.inv_v = with_value ? 1.0 / (double)(positions * with_value) : 0.0;
    G.K.lo = 1.0 - clip; G.K.hi = 1.0 + clip; G.K.c_value = c_value; G.K.c_entropy = c_entropy;
    (void)ppo_carve(h->d_ppo.get(), positions, A, F, G.n_sets, G);
    G.gw1 = d_gw1; G.gb1 = d_gb1; G.gw2 = d_gw2; G.gb2 = d_gb2; G.gwv = d_gwv; G.gbv = d_gbv; G.stats = d_stats;
    const unsigned pairs = (unsigned)(positions * A), chunks = (unsigned)((positions + PPO_CHUNK - 1) / PPO_CHUNK);
    const size_t lds = (size_t)policy_quads(F) * 16u;
    if (G.C == 5) hipLaunchKernelGGL((k_ppo_forward<5>), dim3(pairs), dim3(64), lds, h->stream, G);
    else hipLaunchKernelGGL((k_ppo_forward<8>), dim3(pairs), dim3(64), lds, h->stream, G);
    HIPCHK(h, hipGetLastError());
    const dim3 outer(chunks, (unsigned)((F + h->ppo_tile - 1) / h->ppo_tile), (unsigned)G.n_sets);
    if (h->ppo_tile == 16) hipLaunchKernelGGL((k_ppo_outer<16>), outer, dim3(64), 0, h->stream, G);
    else if (h->ppo_tile == 32) hipLaunchKernelGGL((k_ppo_outer<32>), outer, dim3(64), 0, h->stream, G);
    else hipLaunchKernelGGL((k_ppo_outer<64>), outer, dim3(64), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
    const unsigned elements = ppo_set_floats(F) * (unsigned)G.n_sets + PPO_TERMS;
    hipLaunchKernelGGL((k_ppo_reduce<0>), dim3((elements + 255u) / 256u), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---- the optimiser (definition: cooking_zoo_amd/adam.py; k_adam_norm / k_adam_finish / k_adam_update in cz_adam.h)
extern "C" int32_t cz_sizeof_params(void) { return (int32_t)sizeof(cz_params); }
extern "C" int32_t cz_adam_chunk(void) { return ADAM_CHUNK; }
// Allocates what cz_adam_step_device needs beside the caller's arrays: one float64 per chunk of POLICY_MAX_SETS sets' tensors and the
// control words behind them.  F and C are fixed by cz_create, so one allocation serves the handle's life: outside a capture the first
// time, nothing afterwards.
extern "C" int cz_adam_reserve(cz_handle h) {
    if (!h) return fail(nullptr, "null handle");
    if (h->d_adam) return 0;
    if (caller_capturing(h)) return fail(h, "cz_adam_reserve: the first call allocates the partials: call it outside the capture");
    if (set_device(h)) return 1;
    const size_t words = (size_t)adam_partial_stride(h->P.F, cz_num_actions(h)) * POLICY_MAX_SETS + ADAM_CTL_WORDS;
    HIPCHK(h, hipMalloc(h->d_adam.out(), words * sizeof(double)));
    return 0;
}
static_assert(sizeof(cz_params) == sizeof(AdamGroup), "cz_params is the six pointers of an AdamGroup, in its order");
// One optimiser step on the caller's arrays (adam.host_adam_step): global-norm clipping over the masked sets' gradients, then Adam /
// AdamW on parameters, first and second moments - float32 in torch.nn.Linear's layouts behind a leading axis of cz_policy_sets(h), the
// four structs host memory read during the call - with the state float64 [8] in device memory.  Unless CZ_ADAM_KEEP_TABLE is set the
// new parameters of the masked sets are written into the weight table by the same launch, the value heads too when the value tensors
// are given.  Three launches on the handle's stream: nothing is copied, waited for or allocated (legal inside a capture of the caller).
extern "C" int cz_adam_step_device(cz_handle h, uint32_t set_mask, const cz_params *params, const cz_params *grads, const cz_params *exp_avg,
                                   const cz_params *exp_avg_sq, double *d_state, double lr, const double *d_lr, double beta1, double beta2,
                                   double eps, double weight_decay, double max_norm, uint32_t flags) {
    if (!h) return fail(nullptr, "null handle");
    if (!h->d_policy || h->n_policy_sets == 0) return fail(h, "cz_adam_step_device: no weight table loaded (cz_load_policy_device)");
    if (!h->d_adam) return fail(h, "cz_adam_step_device: no partials reserved (cz_adam_reserve)");
    if (flags & ~(uint32_t)CZ_ADAM_KEEP_TABLE) return fail(h, "cz_adam_step_device: unknown flag bits 0x%x", flags & ~(uint32_t)CZ_ADAM_KEEP_TABLE);
    if (set_mask == 0u) return fail(h, "cz_adam_step_device: set_mask is empty");
    if (set_mask >> h->n_policy_sets) return fail(h, "cz_adam_step_device: set_mask 0x%x names a set past the %d loaded", set_mask, h->n_policy_sets);
    if (!params || !grads || !exp_avg || !exp_avg_sq || !d_state) return fail(h, "cz_adam_step_device: a group or the state pointer is null");
    const cz_params *const groups[4] = {params, grads, exp_avg, exp_avg_sq};
    int value_pointers = 0;
    for (const cz_params *g : groups) {
        if (!g->w1 || !g->b1 || !g->w2 || !g->b2) return fail(h, "cz_adam_step_device: a pointer of the policy's four tensors is null");
        value_pointers += (g->wv != nullptr) + (g->bv != nullptr);
    }
    if (value_pointers != 0 && value_pointers != 8) return fail(h, "cz_adam_step_device: the value tensors (wv, bv) are present in all four groups or in none; %d of 8 pointers are given", value_pointers);
    const bool keep = (flags & CZ_ADAM_KEEP_TABLE) != 0u;
    if (value_pointers && !keep && (set_mask >> h->n_value_sets)) return fail(h, "cz_adam_step_device: value tensors are given, but set_mask 0x%x names a set past the %d value heads loaded (cz_load_value_device, or CZ_ADAM_KEEP_TABLE)", set_mask, h->n_value_sets);
    if (!(lr >= 0.0)) return fail(h, "cz_adam_step_device: lr is %g, not >= 0", lr);
    if (!(weight_decay >= 0.0)) return fail(h, "cz_adam_step_device: weight_decay is %g, not >= 0", weight_decay);
    if (!(max_norm >= 0.0)) return fail(h, "cz_adam_step_device: max_norm is %g, not >= 0", max_norm);
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(h, "cz_adam_step_device: beta1 is %g, not in [0, 1)", beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(h, "cz_adam_step_device: beta2 is %g, not in [0, 1)", beta2);
    if (!(eps > 0.0)) return fail(h, "cz_adam_step_device: eps is %g, not > 0", eps);
    if (set_device(h)) return 1;
    AdamArgs A{};
    A.F = h->P.F; A.C = cz_num_actions(h); A.n_sets = h->n_policy_sets; A.with_value = value_pointers ? 1 : 0; A.set_mask = set_mask;
    const auto group = [](const cz_params &g) { return AdamGroup{{g.w1, g.b1, g.w2, g.b2, g.wv, g.bv}}; };
    A.P = group(*params); A.G = group(*grads); A.M = group(*exp_avg); A.V = group(*exp_avg_sq);
    A.table = keep ? nullptr : h->d_policy.get();
    A.state = d_state; A.d_lr = d_lr; A.lr = lr; A.beta1 = beta1; A.beta2 = beta2; A.omb1 = 1.0 - beta1; A.omb2 = 1.0 - beta2;
    A.eps = eps; A.wd = weight_decay; A.max_norm = max_norm; A.partials = h->d_adam.get();
    const unsigned sets = (unsigned)A.n_sets, stride = adam_partial_stride(A.F, A.C);
    hipLaunchKernelGGL((k_adam_norm<0>), dim3(adam_set_chunks(A.F, A.C, A.with_value), sets), dim3(ADAM_LANES), 0, h->stream, A);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_adam_finish<0>), dim3(1), dim3(ADAM_LANES), (size_t)stride * POLICY_MAX_SETS * sizeof(double), h->stream, A);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_adam_update<0>), dim3((adam_set_elements(A.F, A.C, A.with_value) + ADAM_LANES - 1u) / ADAM_LANES, sets), dim3(ADAM_LANES), 0, h->stream, A);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the device address of pinned, device-mapped host memory (cz_host_alloc, hipHostMalloc, hipHostRegister); nullptr for
// pageable memory
static void *mapped_device_pointer(const void *host) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, host) != hipSuccess) {
        (void)hipGetLastError();                      // pageable memory: "invalid value", not an error of ours
        return nullptr;
    }
    return attr.type == hipMemoryTypeHost ? attr.devicePointer : nullptr;
}

// The host-pointer step: cz_step, and cz_step_compact with d_codes, the device's view of where the codes go.
static int host_step(cz_handle h, const int32_t *actions, double *obs, uint8_t *d_codes, double *rewards, uint8_t *term, uint8_t *trunc) {
    if (ready(h)) return 1;
    if (!actions || !rewards || !term || !trunc) return fail(h, "cz_step: null buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const size_t NA = (size_t)h->P.N * h->P.A, marks_words = 2 * (size_t)h->P.N;
    {   // host actions are checked here (the device-pointer entry points cannot look: their kernel reads action & 7)
        const int32_t n_actions = h->P.scheme == 3 ? 5 : 8;              // actions.py:17,50
        for (size_t i = 0; i < NA; ++i)
            if (actions[i] >= n_actions)
                return fail(h, "cz_step: action %d of env %zu, agent %zu is outside [0, %d) (negative = despawned)", actions[i],
                            i / (size_t)h->P.A, i % (size_t)h->P.A, n_actions);
    }
    const size_t ob = NA * h->P.F * 8;
    // What the three transports below share.  Each says where its five buffers and its marks live; then: the launch (as cz_step_device
    // begins and issues it, with the marks buffer), the staged transport's copies back (`staged` bytes of its device block), one
    // synchronisation, the small outputs out of `small` - the CPU's view of the block they landed in, nullptr where the kernel wrote the
    // caller's arrays - and the marks.
    const auto run = [&](StepCall c, size_t staged, const char *small, size_t o_rew, size_t o_term, size_t o_trunc, const void *marks) -> int {
        c.codes = d_codes;
        if (begin_device_call(h, true, "") || launch_step(h, c)) return 1;
        if (staged) {
            HIPCHK(h, hipMemcpyAsync(h->h_small, h->d_small, staged, hipMemcpyDeviceToHost, h->stream));
            if (obs) HIPCHK(h, hipMemcpyAsync(obs, h->d_obs, ob, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (small) {
            memcpy(rewards, small + o_rew, NA * 8);
            memcpy(term, small + o_term, NA);
            memcpy(trunc, small + o_trunc, NA);
        }
        h->last_marks.assign((const uint32_t *)marks, (const uint32_t *)marks + marks_words);
        return 0;
    };
    // Small batches (the single-env facade): the step is pure latency, so the kernel reads the actions from and writes
    // its outputs to one pinned, device-mapped host block -- one launch and one synchronisation, no copy commands.
    const size_t o_act = 0, o_rew = (NA * 4 + 15) & ~(size_t)15, o_term = o_rew + NA * 8, o_trunc = o_term + ((NA + 15) & ~(size_t)15),
                 o_marks = o_trunc + ((NA + 15) & ~(size_t)15), o_obs = o_marks + (((size_t)h->P.N * 8 + 15) & ~(size_t)15),
                 total = o_obs + ob;
    if (total <= h->zero_copy_bytes) {
        if (!h->h_stage) {
            HIPCHK(h, hipHostMalloc((void **)h->h_stage.out(), total, hipHostMallocMapped));
            HIPCHK(h, hipHostGetDevicePointer((void **)&h->d_stage, h->h_stage, 0));
        }
        memcpy(h->h_stage + o_act, actions, NA * 4);
        StepCall c{(const int32_t *)(h->d_stage + o_act), obs ? (double *)(h->d_stage + o_obs) : nullptr, (double *)(h->d_stage + o_rew),
                   (uint8_t *)(h->d_stage + o_term), (uint8_t *)(h->d_stage + o_trunc)};
        c.marks = (uint32_t *)(h->d_stage + o_marks);
        if (run(c, 0, h->h_stage, o_rew, o_term, o_trunc, h->h_stage + o_marks)) return 1;
        if (obs) memcpy(obs, h->h_stage + o_obs, ob);
        return 0;
    }
    // Buffers from cz_host_alloc (or any pinned, device-mapped host memory): the kernel reads the actions from and writes
    // every output to them directly -- the observation bytes cross PCIe while the launch is still computing, and no copy
    // command is queued at all.
    {
        void *d_act = mapped_device_pointer(actions), *d_rew = mapped_device_pointer(rewards), *d_term = mapped_device_pointer(term),
             *d_trunc = mapped_device_pointer(trunc), *d_obs = obs ? mapped_device_pointer(obs) : nullptr;
        if (d_act && d_rew && d_term && d_trunc && (!obs || d_obs)) {
            if (!h->h_marks) {
                HIPCHK(h, hipHostMalloc((void **)h->h_marks.out(), (size_t)h->P.N * 8, hipHostMallocMapped));
                HIPCHK(h, hipHostGetDevicePointer((void **)&h->d_marks_mapped, h->h_marks, 0));
            }
            StepCall c{(const int32_t *)d_act, (double *)d_obs, (double *)d_rew, (uint8_t *)d_term, (uint8_t *)d_trunc};
            c.marks = h->d_marks_mapped;
            return run(c, 0, nullptr, 0, 0, 0, h->h_marks);
        }
    }
    // Pageable buffers: staged copies.  The small outputs (rewards, flags, marks) live in one device block and come back
    // with one copy command through one pinned block; the observation goes straight into the caller's array.
    const size_t s_rew = 0, s_term = NA * 8, s_trunc = s_term + ((NA + 15) & ~(size_t)15), s_marks = s_trunc + ((NA + 15) & ~(size_t)15),
                 s_total = s_marks + (size_t)h->P.N * 8;
    if (!h->d_actions) {
        HIPCHK(h, hipMalloc(h->d_actions.out(), NA * 4));
        HIPCHK(h, hipMalloc(h->d_small.out(), s_total));
        HIPCHK(h, hipHostMalloc((void **)h->h_small.out(), s_total, hipHostMallocDefault));
    }
    if (obs && !h->d_obs) HIPCHK(h, hipMalloc(h->d_obs.out(), ob));
    HIPCHK(h, hipMemcpyAsync(h->d_actions, actions, NA * 4, hipMemcpyHostToDevice, h->stream));
    StepCall c{h->d_actions, obs ? h->d_obs.get() : nullptr, (double *)(h->d_small + s_rew), (uint8_t *)(h->d_small + s_term), (uint8_t *)(h->d_small + s_trunc)};
    c.marks = (uint32_t *)(h->d_small + s_marks);
    return run(c, s_total, h->h_small, s_rew, s_term, s_trunc, h->h_small + s_marks);
}
extern "C" int cz_step(cz_handle h, const int32_t *actions, double *obs, double *rewards, uint8_t *term, uint8_t *trunc) {
    return host_step(h, actions, obs, nullptr, rewards, term, trunc);
}

// The host-pointer step with the COMPACT observation instead of the float64 rows: codes uint8 [N][A][cz_codes_pitch] (see
// cz_step_device_compact) - 1/8 of the bytes that have to cross PCIe, which is what a host-array step of thousands of envs
// spends its time on.  Buffers from cz_host_alloc are written by the kernel directly; others through a device staging block.
extern "C" int cz_step_compact(cz_handle h, const int32_t *actions, uint8_t *codes, double *rewards, uint8_t *term, uint8_t *trunc) {
    if (ready(h)) return 1;
    if (!codes) return fail(h, "cz_step_compact: null codes buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const size_t bytes = (size_t)h->P.N * h->P.A * (size_t)codes_pitch(h->P.F);
    void *direct = mapped_device_pointer(codes);
    if (!direct && !h->d_codes_stage) HIPCHK(h, hipMalloc(h->d_codes_stage.out(), bytes));
    if (host_step(h, actions, nullptr, direct ? (uint8_t *)direct : (uint8_t *)h->d_codes_stage.get(), rewards, term, trunc)) return 1;
    if (!direct) {
        HIPCHK(h, hipMemcpyAsync(codes, h->d_codes_stage, bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

extern "C" int cz_last_marks(cz_handle h, uint32_t *out) {
    if (ready(h)) return 1;
    if (!out) return fail(h, "cz_last_marks: null buffer");
    if (h->last_marks.size() != 2 * (size_t)h->P.N) return fail(h, "cz_last_marks: no cz_step has run on this handle yet");
    memcpy(out, h->last_marks.data(), (size_t)h->P.N * 8);
    return 0;
}

// Measurement aid for bench.py: `reps` back-to-back launches of a kernel with the step kernel's grid shape that only
// writes `bytes` (<= 2 GiB) to d_dst; returns the average launch duration.  d_dst is overwritten with zeros.
extern "C" int cz_probe_output_only(cz_handle h, void *d_dst, size_t bytes, int32_t reps, float *us_per_launch) {
    if (ready(h)) return 1;
    if (!d_dst || !us_per_launch || reps < 1 || bytes < 16 || bytes > ((size_t)1 << 31)) return fail(h, "cz_probe_output_only: bad arguments");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const dim3 grid((unsigned)((h->P.N + ENVS_PER_WG - 1) / ENVS_PER_WG)), block(64 * ENVS_PER_WG);
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k_probe_fill, grid, block, 0, h->stream, d_dst, (uint32_t)bytes);
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_probe_fill, grid, block, 0, h->stream, d_dst, (uint32_t)bytes);
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *us_per_launch = ms * 1e3f / (float)reps;
    return 0;
}

// the closed loop of the two probes below: K x [one step, the policy's launch] captured into one HIP graph, which is replayed `reps` times
// behind a warm-up replay; the average time per step (step + policy)
template <class Policy>
static int probe_closed_loop(cz_handle h, const StepCall &c, int32_t K, int32_t reps, float *us_per_step, Policy &&policy) {
    const bool was_timing = h->ktime;
    h->ktime = false;
    OwnedGraph g;
    OwnedGraphExec ge;
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    int bad = 0;
    for (int k = 0; k < K && !bad; ++k) {
        bad = launch_step(h, c);
        if (!bad && !getenv("CZ_PROBE_NO_POLICY")) policy();
    }
    const hipError_t ec = hipStreamEndCapture(h->stream, g.out());
    h->ktime = was_timing;
    if (bad) return 1;
    HIPCHK(h, ec);
    const hipError_t ei = hipGraphInstantiate(ge.out(), g, nullptr, nullptr, 0);
    HIPCHK(h, ei);
    hipError_t rc = hipGraphLaunch(ge, h->stream);                         // warm
    if (rc == hipSuccess) rc = hipEventRecord(h->ev0, h->stream);
    for (int r = 0; r < reps && rc == hipSuccess; ++r) rc = hipGraphLaunch(ge, h->stream);
    if (rc == hipSuccess) rc = hipEventRecord(h->ev1, h->stream);
    if (rc == hipSuccess) rc = hipEventSynchronize(h->ev1);
    float ms = 0.f;
    if (rc == hipSuccess) rc = hipEventElapsedTime(&ms, h->ev0, h->ev1);
    HIPCHK(h, rc);
    *us_per_step = ms * 1e3f / (float)((int64_t)reps * K);
    return 0;
}

// Measurement aid for bench.py: a CLOSED loop of K steps - cz_step_device, then a policy kernel that derives every agent's
// next action from the observation it has just been given, on the same stream - captured into one HIP graph and replayed
// `reps` times; returns the average time per step (step + policy).  d_actions (int32 [N][A]) is read and rewritten in place.
extern "C" int cz_probe_closed_loop(cz_handle h, int32_t K, int32_t reps, int32_t *d_actions, double *d_obs, double *d_rewards,
                                    uint8_t *d_term, uint8_t *d_trunc, float *us_per_step) {
    if (ready(h)) return 1;
    if (K < 1 || K > 1024 || reps < 1 || !d_actions || !d_obs || !us_per_step) return fail(h, "cz_probe_closed_loop: bad arguments");
    if (set_device(h)) return 1;
    const StepCall c{d_actions, d_obs, d_rewards, d_term, d_trunc};
    const int rows = h->P.N * h->P.A;
    const uint32_t n_actions = h->P.scheme == 3 ? 5u : 8u;
    return probe_closed_loop(h, c, K, reps, us_per_step, [&] {
        hipLaunchKernelGGL(k_probe_policy, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, h->stream, d_obs, d_actions, rows, h->P.F, n_actions);
    });
}

// Test / measurement aid: ONE launch of that stand-in policy on the handle's stream - d_actions[env][agent] = hash of four features of
// the observation in d_obs (float64 rows) or, with d_obs NULL, in d_codes (compact rows; same actions).  What a caller's policy
// kernel is in tests/test_gpu_capture.py: [cz_probe_policy, cz_step_device] captured into a graph of the CALLER.
extern "C" int cz_probe_policy(cz_handle h, const double *d_obs, const uint8_t *d_codes, int32_t *d_actions) {
    if (ready(h)) return 1;
    if (!d_actions || (!d_obs && !d_codes)) return fail(h, "cz_probe_policy: bad arguments");
    if (set_device(h)) return 1;
    const int rows = h->P.N * h->P.A;
    const uint32_t n_actions = h->P.scheme == 3 ? 5u : 8u;
    if (d_obs) hipLaunchKernelGGL(k_probe_policy, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, h->stream, d_obs, d_actions, rows, h->P.F, n_actions);
    else hipLaunchKernelGGL(k_probe_policy_codes, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, h->stream, d_codes, h->d_lut, d_actions, rows,
                            h->P.F, codes_pitch(h->P.F), n_actions);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ... the same closed loop for a consumer of the compact observation: cz_step_device_compact (codes only, no float64 rows), then
// the policy kernel that reads the codes
extern "C" int cz_probe_closed_loop_compact(cz_handle h, int32_t K, int32_t reps, int32_t *d_actions, uint8_t *d_codes, double *d_rewards,
                                            uint8_t *d_term, uint8_t *d_trunc, float *us_per_step) {
    if (ready(h)) return 1;
    if (K < 1 || K > 1024 || reps < 1 || !d_actions || !d_codes || !us_per_step) return fail(h, "cz_probe_closed_loop_compact: bad arguments");
    if (set_device(h)) return 1;
    StepCall c{d_actions, nullptr, d_rewards, d_term, d_trunc};
    c.codes = d_codes;
    const int rows = h->P.N * h->P.A;
    const uint32_t n_actions = h->P.scheme == 3 ? 5u : 8u;
    return probe_closed_loop(h, c, K, reps, us_per_step, [&] {
        hipLaunchKernelGGL(k_probe_policy_codes, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, h->stream, d_codes, h->d_lut, d_actions, rows,
                           h->P.F, codes_pitch(h->P.F), n_actions);
    });
}

// ---- device memory + timing helpers --------------------------------------------------------------------
extern "C" void *cz_dev_alloc(cz_handle h, size_t bytes) {
    if (!h) return nullptr;
    void *p = nullptr;
    if (hipSetDevice(h->cfg.device_id) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) {
        fail(h, "cz_dev_alloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}
extern "C" int cz_dev_free(cz_handle h, void *p) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipFree(p));
    return 0;
}
// Pinned (page-locked) host memory: buffers handed to cz_step / cz_reset / cz_observe from here are reached by the copy
// engines directly, without the runtime pinning or staging pageable pages on every call.
extern "C" void *cz_host_alloc(cz_handle h, size_t bytes) {
    if (!h) return nullptr;
    void *p = nullptr;
    if (hipSetDevice(h->cfg.device_id) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        fail(h, "cz_host_alloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}
extern "C" int cz_host_free(cz_handle h, void *p) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipHostFree(p));
    return 0;
}
extern "C" int cz_memcpy_h2d(cz_handle h, void *d, const void *s, size_t n) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" int cz_memcpy_d2h(cz_handle h, void *d, const void *s, size_t n) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" int cz_timer_start(cz_handle h) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    return 0;
}
extern "C" int cz_timer_stop(cz_handle h, float *ms) {
    if (!h || !ms) return fail(h, "cz_timer_stop: null argument");
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return 0;
}
extern "C" int cz_kernel_time_reset(cz_handle h, int32_t enable) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->ktime = enable != 0;
    h->kev_used = 0;
    h->ktime_ms = 0.0;
    h->klaunches = 0;
    return 0;
}
extern "C" int cz_kernel_time_read(cz_handle h, double *total_ms, int64_t *launches) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i + 1 < h->kev_used; i += 2) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->kev[i], h->kev[i + 1]));
        h->ktime_ms += ms;
        h->klaunches += 1;
    }
    h->kev_used = 0;
    if (total_ms) *total_ms = h->ktime_ms;
    if (launches) *launches = h->klaunches;
    return 0;
}

// ---- statistics + RCCL ----------------------------------------------------------------------------------
static int stats_reduce(cz_handle h) {
    hipLaunchKernelGGL(k_stats_chains, dim3(STAT_CHAINS / 4), dim3(64), 0, h->stream, h->d_stat_u, h->d_stat_f, h->d_state, h->P.RW, h->P.N,
                       h->d_stats_part);
    hipLaunchKernelGGL(k_stats_tree, dim3(1), dim3(256), 0, h->stream, h->d_stats_part, h->d_stats_out);
    HIPCHK(h, hipGetLastError());
    return 0;
}
extern "C" int cz_get_stats(cz_handle h, cz_stats *out) {
    if (!h || !out) return fail(h, "cz_get_stats: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (stats_reduce(h)) return 1;
    HIPCHK(h, hipMemcpyAsync(out, h->d_stats_out, sizeof(cz_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" int cz_reset_stats(cz_handle h) {
    if (!h) return fail(nullptr, "null handle");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    hipLaunchKernelGGL(k_stats_clear, dim3((h->P.N + 255) / 256), dim3(256), 0, h->stream, h->d_stat_u, h->d_stat_f, h->d_ep_seen,
                       h->d_state, h->P.RW, h->P.N);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// The per-env episode records (cookingzoo.h; cooking_env.py:248,264,329): one launch, two when the packed list or the count is asked
// for, on the handle's stream - no copy, no query, no wait, so the call is legal inside a capture of the caller.
extern "C" int32_t cz_sizeof_episode(void) { return (int32_t)sizeof(cz_episode); }
extern "C" int cz_episodes_collect(cz_handle h, uint8_t *d_mask, double *d_return, int32_t *d_length, uint32_t *d_flags,
                                   cz_episode *d_list, int32_t capacity, int32_t *d_count) {
    if (begin_device_call(h, capacity >= 0, "cz_episodes_collect: capacity is negative")) return 1;
    const int N = h->P.N;
    const dim3 grid((unsigned)((N + EP_BLOCK - 1) / EP_BLOCK)), block(EP_BLOCK);
    const bool ranked = d_list || d_count;
    if (ranked) hipLaunchKernelGGL(k_episodes_count, grid, block, 0, h->stream, h->d_stat_u, h->d_ep_seen, N, h->d_ep_blocks);
    hipLaunchKernelGGL(k_episodes_collect, grid, block, 0, h->stream, h->d_stat_u, h->d_stat_f, h->d_ep_seen, N, h->P.A, h->P.env_id_base,
                       ranked ? h->d_ep_blocks.get() : nullptr, d_mask, d_return, d_length, d_flags, d_list, capacity, d_count);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// RCCL is loaded lazily so that the library also loads on machines without it (CPU build check)
typedef struct { char internal[128]; } cz_nccl_id;
static void *rccl_lib(cz_handle h) {
    // One process holds one RCCL.  A copy that is already loaded (e.g. the librccl.so.1 a PyTorch wheel bundles, loaded
    // together with the HIP runtime that copy was built against) must be the one that is used: glibc matches loaded
    // objects by SONAME, so ask for the SONAME first and without loading anything (RTLD_NOLOAD), then load by SONAME,
    // then by the development name.
    static void *lib = nullptr;
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) fail(h, "cannot load librccl.so.1 / librccl.so: %s", dlerror());
    return lib;
}
// which files serve this process: the RCCL the communicator binds and the HIP runtime the library runs on (diagnostics
// for mixed-stack problems; bench.py prints both)
extern "C" int cz_runtime_paths(char *rccl_path, char *hip_path, size_t cap) {
    if (rccl_path && cap) {
        rccl_path[0] = 0;
        if (void *lib = rccl_lib(nullptr)) {
            Dl_info info;
            void *sym = dlsym(lib, "ncclGetUniqueId");
            if (sym && dladdr(sym, &info) && info.dli_fname) snprintf(rccl_path, cap, "%s", info.dli_fname);
        }
    }
    if (hip_path && cap) {
        hip_path[0] = 0;
        Dl_info info;
        if (dladdr((void *)&hipGetDeviceCount, &info) && info.dli_fname) snprintf(hip_path, cap, "%s", info.dli_fname);
    }
    return 0;
}
extern "C" int cz_comm_unique_id(uint8_t id[128]) {
    void *lib = rccl_lib(nullptr);
    if (!lib) return 1;
    typedef int (*fn_t)(cz_nccl_id *);
    fn_t f = (fn_t)dlsym(lib, "ncclGetUniqueId");
    if (!f) return fail(nullptr, "ncclGetUniqueId not found");
    cz_nccl_id u;
    int r = f(&u);
    if (r) return fail(nullptr, "ncclGetUniqueId failed: %d", r);
    memcpy(id, u.internal, 128);
    return 0;
}
extern "C" int cz_comm_init(cz_handle h, int32_t n_ranks, int32_t rank, const uint8_t id[128]) {
    if (!h) return fail(nullptr, "null handle");
    if (!id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(h, "cz_comm_init: bad arguments");
    if (h->comm) return fail(h, "cz_comm_init: this handle already has a communicator");
    h->rccl = rccl_lib(h);                       // (process-wide handle, never unloaded)
    if (!h->rccl) return 1;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    typedef int (*fn_t)(void **, int, cz_nccl_id, int);
    fn_t f = (fn_t)dlsym(h->rccl, "ncclCommInitRank");
    if (!f) return fail(h, "ncclCommInitRank not found");
    cz_nccl_id u;
    memcpy(u.internal, id, 128);
    int r = f(&h->comm, n_ranks, u, rank);
    if (r) return fail(h, "ncclCommInitRank failed: %d", r);
    h->n_ranks = n_ranks; h->rank = rank;
    HIPCHK(h, hipMalloc(h->d_gather.out(), sizeof(cz_stats) * (size_t)n_ranks));
    return 0;
}
extern "C" int cz_stats_allgather(cz_handle h, cz_stats *out) {
    if (!h || !out) return fail(h, "cz_stats_allgather: null argument");
    if (!h->comm) return fail(h, "cz_stats_allgather: communicator not initialised (cz_comm_init)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (stats_reduce(h)) return 1;
    typedef int (*fn_t)(const void *, void *, size_t, int, void *, hipStream_t);
    fn_t f = (fn_t)dlsym(h->rccl, "ncclAllGather");
    if (!f) return fail(h, "ncclAllGather not found");
    int r = f(h->d_stats_out, h->d_gather, sizeof(cz_stats), /*ncclInt8*/ 0, h->comm, h->stream);
    if (r) return fail(h, "ncclAllGather failed: %d", r);
    HIPCHK(h, hipMemcpyAsync(out, h->d_gather, sizeof(cz_stats) * (size_t)h->n_ranks, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// Barrier over the communicator: a 4-byte RCCL all-reduce on the handle's stream, then a stream synchronisation.  Every
// rank returns only after every rank's earlier work on its handle stream has finished (bench.py brackets its timed
// region with it).
extern "C" int cz_comm_barrier(cz_handle h) {
    if (!h) return fail(nullptr, "null handle");
    if (!h->comm) return fail(h, "cz_comm_barrier: communicator not initialised (cz_comm_init)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    typedef int (*fn_t)(const void *, void *, size_t, int, int, void *, hipStream_t);
    fn_t f = (fn_t)dlsym(h->rccl, "ncclAllReduce");
    if (!f) return fail(h, "ncclAllReduce not found");
    // d_gather holds n_ranks cz_stats: its first word doubles as the barrier token (overwritten by the next all-gather)
    HIPCHK(h, hipMemsetAsync(h->d_gather, 0, 4, h->stream));
    int r = f(h->d_gather, h->d_gather, 1, /*ncclInt32*/ 2, /*ncclSum*/ 0, h->comm, h->stream);
    if (r) return fail(h, "ncclAllReduce failed: %d", r);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
