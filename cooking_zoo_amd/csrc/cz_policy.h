// cz_policy.h -- the MLP policy the library evaluates itself (definition and host model: cooking_zoo_amd/policy.py): the packed
// weight table, cz_exp, and the device functions that go from a float32 row in LDS to an action and a value: policy_hidden, policy_heads
// and policy_value.  k_policy and k_value (cz_query.h) and k_step<..., ROLLOUT_POLICY / ROLLOUT_POLICY_VALUE> (cz_kernels.h) all call
// them, so the launches of their own and the fused rollouts cannot differ.
// Beside them cz_log and policy_logprob, the log-probability and entropy of the distribution policy_heads samples from (k_logprob;
// definition: cooking_zoo_amd/targets.py), and policy_all_logits and policy_ppo_logit_grad, the forward and the float64 part of PPO's
// gradients (k_ppo_forward; definition: cooking_zoo_amd/ppo.py).
#pragma once
#include "cz_device.h"

namespace cz {

constexpr int POLICY_HIDDEN = 64;            // one lane per hidden unit
constexpr int POLICY_MAX_SETS = 4, POLICY_MAX_ACTIONS = 8;
constexpr uint32_t POLICY_NONE = 0xFFu;      // an agent's byte of `sets`: no policy for this agent
constexpr uint32_t POLICY_AGENT_KEY = 0x300u;   // agent key of the sampling draw (0..3 spawn draws, 0x100 layouts, 0x200 tasks)
enum : uint32_t { POLICY_GREEDY = 0, POLICY_SAMPLE = 1 };

// One weight set in the table, as floats: W1 as [Fq][64][4] - unit j's weights of features 4q .. 4q+3 in one 16-byte word, so that
// lane j's load of a quad is coalesced with its neighbours'; weights of features past F are 0.0 - then b1 [64], W2 [8][64] and b2 [8]
// (rows past C are 0.0 and never read).
__host__ __device__ inline int policy_quads(int F) { return (F + 3) >> 2; }
__host__ __device__ inline uint32_t policy_set_floats(int F) {
    return (uint32_t)policy_quads(F) * 256u + POLICY_HIDDEN + POLICY_MAX_ACTIONS * POLICY_HIDDEN + POLICY_MAX_ACTIONS;
}
// Behind the POLICY_MAX_SETS sets, in the same allocation: the value heads (cz_load_value_device), wv [4][64] then bv [4].  A set's
// value head reads that set's hidden vector.
__host__ __device__ inline uint32_t policy_value_offset(int F) { return POLICY_MAX_SETS * policy_set_floats(F); }
constexpr uint32_t POLICY_VALUE_FLOATS = POLICY_MAX_SETS * POLICY_HIDDEN + POLICY_MAX_SETS;
__host__ __device__ inline uint32_t policy_table_floats(int F) { return policy_value_offset(F) + POLICY_VALUE_FLOATS; }
// `sets` (agent a's set in byte a, 0xFF none) and the mode in 13 bits: three bits per agent, 7 = none, mode in bit 12
constexpr int POLICY_VSETS_BITS = 3 * MAX_AGENTS, POLICY_SETS_BITS = POLICY_VSETS_BITS + 1;
static_assert(POLICY_MAX_SETS <= 7, "a set index takes three bits, and 7 stays free for `none`");
__host__ __device__ inline uint32_t policy_pack_sets(uint32_t sets, uint32_t mode, int A) {
    uint32_t pk = (mode & 1u) << POLICY_VSETS_BITS;
    for (int a = 0; a < MAX_AGENTS; ++a) {
        const uint32_t s = a < A ? (sets >> (8 * a)) & 0xFFu : POLICY_NONE;
        pk |= (s == POLICY_NONE ? 7u : s) << (3 * a);
    }
    return pk;
}

// `vsets` (agent a's value set in byte a, 0xFF none) in 12 bits, three per agent as above
__host__ __device__ inline uint32_t policy_pack_vsets(uint32_t vsets, int A) { return policy_pack_sets(vsets, 0u, A); }

// ---- The policy rollouts' borrowed slots (k_step<..., ROLLOUT_POLICY / ROLLOUT_POLICY_VALUE>): this description, policy_encode and
// the two decoders are everything that knows them.  The step kernel's argument block must not grow, and a float32 fused launch leaves
// `actions`, `obs` and `marks_out` of Params unused - and the kernel block's own `actions` dead, since the leading scalar e_actions
// (early_of) stands in for it.  What a policy rollout adds to such a launch:
struct PolicyLaunch {
    int32_t *actions = nullptr;        // output int32 [T][N][A], every agent's action as played (may be null) -> Params::actions, so e_actions
    float *logits = nullptr;           // output float [T][N][A][C], policy agents only (may be null)          -> Params::obs
    const float *table = nullptr;      // the weight table, with `packed` (policy_pack_sets) as its tag         -> Params::marks_out
    uint32_t packed = 0;
    float *values = nullptr;           // output float [T + 1][N][A]; null: ROLLOUT_POLICY.  With `vpacked`     -> the kernel block's `actions`
    uint32_t vpacked = 0;              // (policy_pack_vsets) as its tag
};
// A tag rides in the bits of a slot that no device address uses
constexpr int POLICY_TAG_SHIFT = 48;
constexpr uint64_t POLICY_ADDRESS_MASK = (1ull << POLICY_TAG_SHIFT) - 1;
static_assert(sizeof(void *) == 8 && sizeof(uintptr_t) == 8, "a slot is a 64-bit pointer");
static_assert(POLICY_SETS_BITS <= 64 - POLICY_TAG_SHIFT && POLICY_VSETS_BITS <= 64 - POLICY_TAG_SHIFT, "the packed sets fit the tag");
inline bool policy_taggable(const void *p) { return (reinterpret_cast<uintptr_t>(p) >> POLICY_TAG_SHIFT) == 0; }
// The encoder: the one writer of the four slots.  `P` is the launch's otherwise finished Params - the leading scalars are made from
// it - and `block` becomes the kernel's by-value block.  False, and nothing written: an address reaches into the tag's bits.
inline bool policy_encode(const PolicyLaunch &L, Params &P, Params &block) {
    if (!policy_taggable(L.table) || !policy_taggable(L.values)) return false;
    const auto tagged = [](const void *p, uint32_t tag) { return reinterpret_cast<uintptr_t>(p) | ((uintptr_t)tag << POLICY_TAG_SHIFT); };
    P.actions = L.actions;
    P.obs = reinterpret_cast<double *>(L.logits);
    P.marks_out = reinterpret_cast<uint32_t *>(tagged(L.table, L.packed));
    block = P;
    if (L.values) block.actions = reinterpret_cast<const int32_t *>(tagged(L.values, L.vpacked));
    return true;
}
// The decoders: a tagged slot -> its pointer, its packed bits
template <class T>
__device__ __forceinline__ T *policy_slot_pointer(const void *slot) {
    return reinterpret_cast<T *>(static_cast<uintptr_t>((uint64_t)reinterpret_cast<uintptr_t>(slot) & POLICY_ADDRESS_MASK));
}
__device__ __forceinline__ uint32_t policy_slot_tag(const void *slot) { return (uint32_t)((uint64_t)reinterpret_cast<uintptr_t>(slot) >> POLICY_TAG_SHIFT); }

typedef float float4_t __attribute__((ext_vector_type(4)));
// the float32 rows a policy reads, in LDS: per env A rows of 4 * policy_quads(F) floats, the tail zeroed (sized by the launch)
extern __shared__ float4_t policy_rows[];

// exp on [-64, 64] in plain float64 arithmetic, every operation rounded on its own (the build has -ffp-contract=off): numpy
// reproduces it bit for bit (policy.cz_exp)
__host__ __device__ inline double policy_exp(double z) {
    const double k = floor(z * 1.4426950408889634 + 0.5);
    const double r = (z - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0,
                              1.0 / 362880.0, 1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    double p = c[13];
#pragma unroll
    for (int i = 12; i >= 0; --i) p = p * r + c[i];
    return ldexp(p, (int)k);
}

// log on [1, 8] in the same arithmetic, with no division (targets.cz_log): the chord of log under [1, 2] scaled by the power of two,
// then five Newton steps on S * exp(-y) = 1.  policy_log(1.0) is 0.0 exactly.
__host__ __device__ inline double policy_log(double S) {
    constexpr double ln2 = 0.6931471805599453;
    const int k = (S >= 2.0) + (S >= 4.0) + (S >= 8.0);
    const double m = S * (k == 0 ? 1.0 : k == 1 ? 0.5 : k == 2 ? 0.25 : 0.125);
    double y = (double)k * ln2 + (m - 1.0) * ln2;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double ny = -y;
        y = y + (S * policy_exp(ny > -64.0 ? ny : -64.0) - 1.0);
    }
    return y;
}

// The softmax policy_heads samples from, as log-probabilities (targets.host_logprob): the C logits of one row -> the float64
// log-probability of `action` (0.0 for an action outside 0 .. C-1) and the entropy, each rounded to float32 by the caller.
template <int C>
__host__ __device__ __forceinline__ void policy_logprob(const float (&logit)[C], int action, double &logp, double &entropy) {
    float best = logit[0];
#pragma unroll
    for (int c = 1; c < C; ++c) best = logit[c] > best ? logit[c] : best;
    double z[C], S = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        z[c] = (double)logit[c] - (double)best;
        const double ex = policy_exp(z[c] > -64.0 ? z[c] : -64.0);
        S = c == 0 ? ex : S + ex;
    }
    const double L = policy_log(S);
    double za = 0.0, acc = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        za = action == c ? z[c] : za;
        const double q = z[c] - L;
        const double pq = policy_exp(q > -64.0 ? q : -64.0) * q;
        acc = c == 0 ? pq : acc + pq;
    }
    logp = (unsigned)action < (unsigned)C ? za - L : 0.0;
    entropy = -acc;
}

// p + p of lane (lane xor 2^k) for k = 0..5.  After level k every aligned group of 2^(k+1) lanes holds one value, so a lane may
// take its partner's value from ANY lane of the partner group: the mirrors of the DPP row stand in for xor 4 and xor 8.
__device__ __forceinline__ float policy_butterfly(float p) {
    auto dpp = [](float v, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), decltype(ctrl)::value, 0xF, 0xF, false));
    };
    p = p + dpp(p, std::integral_constant<int, 0xB1>{});         // quad_perm [1, 0, 3, 2]
    p = p + dpp(p, std::integral_constant<int, 0x4E>{});         // quad_perm [2, 3, 0, 1]
    p = p + dpp(p, std::integral_constant<int, 0x141>{});        // row_half_mirror
    p = p + dpp(p, std::integral_constant<int, 0x140>{});        // row_mirror
    p = p + __shfl_xor(p, 16);
    p = p + __shfl_xor(p, 32);
    return p;
}

// The hidden layer of one row (steps 1-2 of policy.py): `set` a weight set (wave-uniform), `x` the row in LDS (4 * Fq floats, 16-byte
// aligned, zero behind F).  Lane j returns h_j.
__device__ __forceinline__ float policy_hidden(const float *__restrict__ set, int Fq, const float *x, int lane) {
    const float *const b1 = set + (uint32_t)Fq * 256u;
    // lane = unit: one rounding per feature, features ascending
    float acc = b1[lane];
#pragma unroll 4
    for (int q = 0; q < Fq; ++q) {
        const float4_t w = *reinterpret_cast<const float4_t *>(set + ((uint32_t)q * 64u + (uint32_t)lane) * 4u);
        const float4_t v = *reinterpret_cast<const float4_t *>(x + 4 * q);                 // the same address on every lane: a broadcast
        acc = __builtin_fmaf(w.x, v.x, acc);
        acc = __builtin_fmaf(w.y, v.y, acc);
        acc = __builtin_fmaf(w.z, v.z, acc);
        acc = __builtin_fmaf(w.w, v.w, acc);
    }
    return acc > 0.0f ? acc : 0.0f;
}

// The action heads on a hidden vector (steps 3-5): C the action count.  Every lane returns the same action; lane c < C returns
// logit c in `mylogit`.  The draw of POLICY_SAMPLE is spawn_uniform(seed, global env id, step, 0x300 + agent, 0).
template <int C>
__device__ __forceinline__ void policy_heads(const float *__restrict__ set, int Fq, float hid, int lane, uint32_t mode, uint64_t seed,
                                             int64_t env_global, uint32_t step, int agent, int &action, float &mylogit) {
    static_assert(C >= 1 && C <= POLICY_MAX_ACTIONS, "action count");
    const float *const w2 = set + (uint32_t)Fq * 256u + POLICY_HIDDEN, *const b2 = w2 + POLICY_MAX_ACTIONS * POLICY_HIDDEN;
    float logit[C];
#pragma unroll
    for (int c = 0; c < C; ++c) logit[c] = policy_butterfly(w2[c * POLICY_HIDDEN + lane] * hid) + b2[c];
    float best = logit[0];
    int arg = 0;
    mylogit = logit[0];
#pragma unroll
    for (int c = 1; c < C; ++c) {
        if (logit[c] > best) { best = logit[c]; arg = c; }          // the smallest c with the largest logit
        mylogit = lane == c ? logit[c] : mylogit;
    }
    action = arg;
    if (mode == POLICY_SAMPLE) {
        const double u = spawn_uniform(seed, (uint64_t)env_global, (uint64_t)step, POLICY_AGENT_KEY + (uint32_t)agent, 0u);
        double S[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double z = (double)logit[c] - (double)best;
            const double ex = policy_exp(z > -64.0 ? z : -64.0);
            S[c] = c == 0 ? ex : S[c - 1] + ex;
        }
        const double thr = u * S[C - 1];
        int pick = C - 1;
#pragma unroll
        for (int c = C - 2; c >= 0; --c) pick = S[c] > thr ? c : pick;
        action = pick;
    }
}

// The value head of set `vs` on that set's hidden vector (step 3b): one more row of the output layer.  Every lane returns the value.
__device__ __forceinline__ float policy_value(const float *__restrict__ table, int F, uint32_t vs, float hid, int lane) {
    const float *const heads = table + policy_value_offset(F);
    return policy_butterfly(heads[vs * POLICY_HIDDEN + (uint32_t)lane] * hid) + heads[POLICY_MAX_SETS * POLICY_HIDDEN + vs];
}

// ---- PPO's clipped-surrogate loss, differentiated (definition: cooking_zoo_amd/ppo.py; kernels: k_ppo_forward, k_ppo_outer and
// k_ppo_reduce in cz_query.h).  The scales the host computes once per call:
struct PpoScales {
    double inv_p, inv_v;           // 1 / (positions * agents with a policy set), ... with a value set; 0.0 where there is none
    double lo, hi;                 // 1 - eps, 1 + eps
    double c_value, c_entropy;
};
constexpr int PPO_CHUNK = 64;                // positions per chunk: every (chunk, set) has accumulators of its own (ppo.py)
constexpr int PPO_TERMS = 8;                 // the statistics' terms of one (position, agent)
// The logits of one row under set `set` - policy_heads' arithmetic, every lane gets every logit
template <int C>
__device__ __forceinline__ void policy_all_logits(const float *__restrict__ set, int Fq, float hid, int lane, float (&logit)[C]) {
    const float *const w2 = set + (uint32_t)Fq * 256u + POLICY_HIDDEN, *const b2 = w2 + POLICY_MAX_ACTIONS * POLICY_HIDDEN;
#pragma unroll
    for (int c = 0; c < C; ++c) logit[c] = policy_butterfly(w2[c * POLICY_HIDDEN + lane] * hid) + b2[c];
}
// The policy part of one (position, agent) in float64 (ppo.py): the C logits, the action (inside 0 .. C-1), logp_old and the
// advantage -> the gradient with respect to the logits, rounded to float32 once, and the statistics' terms 0, 2, 3 and 4.  The
// softmax is policy_logprob's, so q_act here is the float64 whose rounding cz_logprob_device wrote: on the weights that played the
// ratio is exactly 1.
template <int C>
__host__ __device__ __forceinline__ void policy_ppo_logit_grad(const float (&logit)[C], int action, double logp_old, double Adv, const PpoScales &K,
                                                               float (&g)[C], double (&term)[PPO_TERMS]) {
    float best = logit[0];
#pragma unroll
    for (int c = 1; c < C; ++c) best = logit[c] > best ? logit[c] : best;
    double z[C], S = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        z[c] = (double)logit[c] - (double)best;
        const double ex = policy_exp(z[c] > -64.0 ? z[c] : -64.0);
        S = c == 0 ? ex : S + ex;
    }
    const double L = policy_log(S);
    double q[C], p[C], qa = 0.0, acc = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        q[c] = z[c] - L;
        p[c] = policy_exp(q[c] > -64.0 ? q[c] : -64.0);
        const double pq = p[c] * q[c];
        acc = c == 0 ? pq : acc + pq;
        qa = action == c ? q[c] : qa;
    }
    const double H = -acc, lpn = (double)(float)qa;          // what cz_logprob_device writes for these logits
    double d = lpn - logp_old;
    d = d > -64.0 ? d : -64.0;
    d = d < 64.0 ? d : 64.0;
    const double ratio = policy_exp(d);
    const bool clipped = (Adv > 0.0 && ratio > K.hi) || (Adv < 0.0 && ratio < K.lo);
    const double glp = clipped ? 0.0 : -(Adv * ratio);
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = (float)(K.inv_p * (glp * ((action == c ? 1.0 : 0.0) - p[c]) + K.c_entropy * (p[c] * (q[c] + H))));
    double rc = ratio > K.lo ? ratio : K.lo;
    rc = rc < K.hi ? rc : K.hi;
    const double s1 = ratio * Adv, s2 = rc * Adv;
    term[0] = -(s1 < s2 ? s1 : s2);
    term[2] = H;
    term[3] = logp_old - lpn;
    term[4] = clipped ? 1.0 : 0.0;
}

}  // namespace cz
