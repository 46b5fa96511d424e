// cz_launch.h -- what an instantiation unit exports: the Launchers table, and Inst<>, which fills it with the launches of one
// instance's kernels (included by the three cz_inst_*.hip units and by cz_api.hip).
#pragma once
#include "cz_kernels.h"
#include "cz_offstep.h"
#include "cz_query.h"

namespace cz {

// launchers exported by each instantiation unit
struct Launchers {
    // lean: k_step_lean (mode STEP, and only where has_lean); otherwise k_step<..., mode>.  Fused modes run P.T steps per launch.
    // The last argument is the kernel's block of the two policy modes (policy_encode), null for every other launch
    hipError_t (*step)(const Params &, hipStream_t, StepChoice, const Params *);
    hipError_t (*reset)(const Params &, hipStream_t, int64_t, int, const int32_t *, const uint32_t *, const uint32_t *, double *);
    hipError_t (*observe)(const Params &, hipStream_t, int64_t, int, double *, uint8_t *);
    bool has_lean;             // the instance carries the k_step_lean kernels
    hipError_t (*observe_f32)(const Params &, hipStream_t, int64_t, int, float *);
    // k_reset_where over all P.N envs: mask, layout ids, float64 rows, float32 rows, codes, refused counter
    hipError_t (*reset_where)(const Params &, hipStream_t, const uint8_t *, const int32_t *, double *, float *, uint8_t *, unsigned long long *);
    // k_restore_where over all P.N envs: slots, archive, its rows, recipes in the table, float64 rows, float32 rows, codes, refused counter
    hipError_t (*restore_where)(const Params &, hipStream_t, const int32_t *, const uint32_t *, int64_t, uint32_t, double *, float *, uint8_t *,
                                unsigned long long *);
    // k_set_tasks over all P.N envs: mask, recipe ids (a word per env), task list (a word per row), its rows, seed, recipes in the table, refused counter
    hipError_t (*set_tasks)(const Params &, hipStream_t, const uint8_t *, const uint32_t *, const uint32_t *, uint32_t, uint64_t, uint32_t,
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

template <int OPL, int CPL, bool HAS_LEAN = false>
struct Inst {
    static hipError_t step(const Params &P, hipStream_t st, StepChoice c, const Params *policy_block) {
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
                case ROLLOUT_POLICY: return launch_policy_step_kernel<CPL>(k_step<OPL, CPL, NA, S, ROLLOUT_POLICY>, P, policy_block, st);
                case ROLLOUT_POLICY_VALUE: return launch_policy_step_kernel<CPL>(k_step<OPL, CPL, NA, S, ROLLOUT_POLICY_VALUE>, P, policy_block, st);
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
    static hipError_t set_tasks(const Params &P, hipStream_t st, const uint8_t *mask, const uint32_t *ids, const uint32_t *list, uint32_t K,
                                uint64_t seed, uint32_t n_recipes, unsigned long long *refused) {
        return CZ_LAUNCH_PER_ENV(k_set_tasks, P.N, mask, ids, list, K, seed, n_recipes, refused);
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
        Launchers L{};
        L.step = &step; L.reset = &reset; L.observe = &observe; L.has_lean = HAS_LEAN; L.observe_f32 = &observe_f32;
        L.reset_where = &reset_where; L.restore_where = &restore_where; L.observe_grid = &observe_grid; L.navigate = &navigate;
        L.partner = &partner; L.action_effects = &action_effects; L.render = &render; L.set_tasks = &set_tasks;
        return L;
    }
};

Launchers launchers_small();   // D <= 64 slots, W*H <= 64 cells
Launchers launchers_large();   // D <= 128 slots, W*H <= 256 cells
Launchers launchers_huge();    // D <= 255 slots, W*H <= 1024 cells

}  // namespace cz