// cz_adam.h -- the optimiser on the device (cz_adam_reserve, cz_adam_step_device; definition and numpy models: cooking_zoo_amd/adam.py):
// global-norm gradient clipping and Adam / AdamW in float64 with every operation rounded on its own, on the caller's float32 parameters,
// gradients and moments in torch.nn.Linear's layouts behind a leading axis of the loaded sets, and the packed weight table (cz_policy.h)
// written with the same new float32.  Three launches share one argument block: k_adam_norm (one float64 partial per chunk of 1024
// gradient elements), k_adam_finish (one workgroup: the serial total in the pinned order, the finite test, the coefficient, the
// state) and k_adam_update (elementwise).  No kernel reads a state word another workgroup of its launch writes: k_adam_finish is the
// only reader and writer of the state, and what k_adam_update needs of it travels in control words behind the partials.
// Included at the end of cz_query.h.
#pragma once
#include "cz_policy.h"

namespace cz {

constexpr int ADAM_CHUNK = 1024, ADAM_LANES = 256;      // elements per chunk, threads per chunk (adam.py)
constexpr int ADAM_TENSORS = 6;                         // w1, b1, w2, b2, wv, bv: the order of the norm's chain
enum : int { ADAM_CTL_GO = 0, ADAM_CTL_COEF, ADAM_CTL_BC1, ADAM_CTL_BC2, ADAM_CTL_LR, ADAM_CTL_LW, ADAM_CTL_WORDS = 8 };
struct AdamGroup { float *t[ADAM_TENSORS]; };           // one of the four groups; t[4] and t[5] null: no value tensors
struct AdamArgs {
    int32_t F, C, n_sets, with_value;
    uint32_t set_mask;
    AdamGroup P, G, M, V;          // G is only read
    float *table;                  // the packed weight sets and the value heads behind them; null: CZ_ADAM_KEEP_TABLE
    double *state;                 // [8] (adam.py)
    const double *d_lr;            // null: `lr`
    double lr, beta1, beta2, omb1, omb2, eps, wd, max_norm;
    double *partials;              // [POLICY_MAX_SETS][adam_set_chunks(F, C, 1)], then ADAM_CTL_WORDS control words
};
// elements of tensor t in one set
__host__ __device__ inline uint32_t adam_len(int t, int F, int C) {
    return t == 0 ? (uint32_t)POLICY_HIDDEN * (uint32_t)F : t == 1 ? POLICY_HIDDEN : t == 2 ? (uint32_t)C * POLICY_HIDDEN : t == 3 ? (uint32_t)C : t == 4 ? POLICY_HIDDEN : 1u;
}
__host__ __device__ inline uint32_t adam_chunks(int t, int F, int C) { return (adam_len(t, F, C) + ADAM_CHUNK - 1u) / ADAM_CHUNK; }
__host__ __device__ inline int adam_tensors(int with_value) { return with_value ? ADAM_TENSORS : ADAM_TENSORS - 2; }
// chunks, and elements, of one set's tensors
__host__ __device__ inline uint32_t adam_set_chunks(int F, int C, int with_value) {
    uint32_t n = 0;
    for (int t = 0; t < adam_tensors(with_value); ++t) n += adam_chunks(t, F, C);
    return n;
}
__host__ __device__ inline uint32_t adam_set_elements(int F, int C, int with_value) {
    uint32_t n = 0;
    for (int t = 0; t < adam_tensors(with_value); ++t) n += adam_len(t, F, C);
    return n;
}
// the partials of a set lie at set * adam_set_chunks(F, C, 1), whether the call has value tensors or not
__host__ __device__ inline uint32_t adam_partial_stride(int F, int C) { return adam_set_chunks(F, C, 1); }

// Grid (chunk of the set's tensors, set), 256 threads: lane l adds the squares of elements l, l + 256, l + 512, l + 768 of its chunk
// in that order (+0.0 past the segment's end), then the butterfly over the 256 lanes - six levels inside a wavefront, the last two over
// the four wavefronts' values in LDS, (w0 + w1) + (w2 + w3): what lane 0 holds after levels 6 and 7.  One float64 per chunk.
template <int UNUSED = 0>
__global__ __launch_bounds__(ADAM_LANES) void k_adam_norm(const AdamArgs A) {
    const uint32_t set = blockIdx.y, lane = threadIdx.x;
    if (!((A.set_mask >> set) & 1u)) return;
    uint32_t c = blockIdx.x;
    int t = 0;
    for (; t < adam_tensors(A.with_value); ++t) {
        const uint32_t n = adam_chunks(t, A.F, A.C);
        if (c < n) break;
        c -= n;
    }
    if (t >= adam_tensors(A.with_value)) return;
    const uint32_t len = adam_len(t, A.F, A.C);
    const float *const g = A.G.t[t] + (size_t)set * len;
    double s = 0.0;
#pragma unroll
    for (uint32_t r = 0; r < ADAM_CHUNK / ADAM_LANES; ++r) {
        const uint32_t e = c * ADAM_CHUNK + r * ADAM_LANES + lane;
        const double x = e < len ? (double)g[e] : 0.0, sq = x * x;
        s = r == 0 ? sq : s + sq;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) s = s + __shfl_xor(s, k, 64);
    __shared__ double wave_sum[ADAM_LANES / 64];
    if ((lane & 63u) == 0u) wave_sum[lane >> 6] = s;
    __syncthreads();
    if (lane == 0u) A.partials[(size_t)set * adam_partial_stride(A.F, A.C) + blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// One workgroup: the partials go to LDS, thread 0 adds them as one chain - tensors in order, within a tensor the masked sets ascending,
// within a segment the chunks ascending - and decides: a total that is not finite skips the call ([4] = 0, [5] += 1, go = 0),
// otherwise the coefficient, the bias corrections and the learning rate go into the control words and the state advances.
template <int UNUSED = 0>
__global__ __launch_bounds__(ADAM_LANES) void k_adam_finish(const AdamArgs A) {
    extern __shared__ double adam_parts[];
    const uint32_t stride = adam_partial_stride(A.F, A.C), count = stride * (uint32_t)A.n_sets;
    for (uint32_t i = threadIdx.x; i < count; i += ADAM_LANES)
        if ((A.set_mask >> (i / stride)) & 1u) adam_parts[i] = A.partials[i];
    __syncthreads();
    if (threadIdx.x != 0u) return;
    double total = 0.0;
    bool first = true;
    uint32_t base = 0;
    for (int t = 0; t < adam_tensors(A.with_value); ++t) {
        const uint32_t n = adam_chunks(t, A.F, A.C);
        for (uint32_t set = 0; set < (uint32_t)A.n_sets; ++set) {
            if (!((A.set_mask >> set) & 1u)) continue;
            for (uint32_t c = 0; c < n; ++c) {
                const double p = adam_parts[set * stride + base + c];
                total = first ? p : total + p;
                first = false;
            }
        }
        base += n;
    }
    double *const ctl = A.partials + (size_t)stride * POLICY_MAX_SETS;
    const double norm = sqrt(total);
    A.state[3] = norm;
    if (!(total < __builtin_inf())) {
        A.state[4] = 0.0;
        A.state[5] = A.state[5] + 1.0;
        ctl[ADAM_CTL_GO] = 0.0;
        return;
    }
    const double lr = A.d_lr ? *A.d_lr : A.lr;
    double coef = 1.0;
    if (A.max_norm != 0.0) {
        const double q = A.max_norm / (norm + 1e-6);
        coef = q < 1.0 ? q : 1.0;
    }
    const double p1 = A.state[1] * A.beta1, p2 = A.state[2] * A.beta2;
    A.state[0] = A.state[0] + 1.0;
    A.state[1] = p1;
    A.state[2] = p2;
    A.state[4] = coef;
    A.state[6] = lr;
    ctl[ADAM_CTL_GO] = 1.0;
    ctl[ADAM_CTL_COEF] = coef;
    ctl[ADAM_CTL_BC1] = 1.0 - p1;
    ctl[ADAM_CTL_BC2] = 1.0 - p2;
    ctl[ADAM_CTL_LR] = lr;
    ctl[ADAM_CTL_LW] = lr * A.wd;
}

// Grid (256 elements of a set's tensors in torch's order, set): one thread per element reads G, M, V, P, writes M, V, P (coalesced)
// and puts the new parameter where k_policy_pack / k_value_pack would put it - W1 at [q][j][4], then b1, W2, b2, the value heads behind
// the sets - so the table is byte for byte a reload's; its padding entries are never touched.
template <int UNUSED = 0>
__global__ __launch_bounds__(ADAM_LANES) void k_adam_update(const AdamArgs A) {
    const uint32_t set = blockIdx.y;
    if (!((A.set_mask >> set) & 1u)) return;
    const double *const ctl = A.partials + (size_t)adam_partial_stride(A.F, A.C) * POLICY_MAX_SETS;
    if (ctl[ADAM_CTL_GO] == 0.0) return;
    uint32_t o = blockIdx.x * ADAM_LANES + threadIdx.x;
    int t = 0;
    for (; t < adam_tensors(A.with_value); ++t) {
        const uint32_t n = adam_len(t, A.F, A.C);
        if (o < n) break;
        o -= n;
    }
    if (t >= adam_tensors(A.with_value)) return;
    const size_t at = (size_t)set * adam_len(t, A.F, A.C) + o;
    const double coef = ctl[ADAM_CTL_COEF], bc1 = ctl[ADAM_CTL_BC1], bc2 = ctl[ADAM_CTL_BC2], lr = ctl[ADAM_CTL_LR];
    const double g = coef * (double)A.G.t[t][at];
    const float m = (float)(A.beta1 * (double)A.M.t[t][at] + A.omb1 * g);
    const float v = (float)(A.beta2 * (double)A.V.t[t][at] + (A.omb2 * g) * g);
    const double mh = (double)m / bc1, vh = (double)v / bc2;
    double p = (double)A.P.t[t][at];
    if (A.wd != 0.0) p = p - ctl[ADAM_CTL_LW] * p;
    const float out = (float)(p - lr * (mh / (sqrt(vh) + A.eps)));
    A.M.t[t][at] = m;
    A.V.t[t][at] = v;
    A.P.t[t][at] = out;
    if (!A.table) return;
    const uint32_t w1_end = (uint32_t)policy_quads(A.F) * 256u, F = (uint32_t)A.F;
    float *const own = A.table + (size_t)set * policy_set_floats(A.F), *const heads = A.table + policy_value_offset(A.F);
    if (t == 0) {
        const uint32_t j = o / F, f = o - j * F;
        own[(f >> 2) * 256u + j * 4u + (f & 3u)] = out;
    } else if (t == 1) own[w1_end + o] = out;
    else if (t == 2) own[w1_end + POLICY_HIDDEN + o] = out;
    else if (t == 3) own[w1_end + POLICY_HIDDEN + POLICY_MAX_ACTIONS * POLICY_HIDDEN + o] = out;
    else if (t == 4) heads[set * POLICY_HIDDEN + o] = out;
    else heads[POLICY_MAX_SETS * POLICY_HIDDEN + set] = out;
}

}  // namespace cz
