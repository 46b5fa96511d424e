/*
 * cookingzoo.h -- C-ABI of the MI355X-native CookingZoo step() path (libcookingzoo_hip.so).
 *
 * The reference (DavidRother/cooking_zoo) has no FFI: its boundary is the Python API
 * (`cooking_zoo/environment/cooking_env.py:26-46` parallel_env, `:243` accumulated_step, `:271` observe,
 * `:178` reset).  This header is the boundary the build introduces UNDER that API: plain pointers and
 * sizes, no torch types.  Each entry point names the reference code it replaces.  The Python host
 * (cooking_zoo_amd/_native.py) binds it with ctypes; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: every function returns 0 on success, non-zero on failure with a message available from
 * cz_last_error(handle) (or cz_last_error(NULL) for creation failures).  One host thread per handle;
 * one HIP stream per handle (its own, or the caller's after cz_set_stream); the caller owns every buffer it passes; the library owns device state
 * until cz_destroy.  "d_" parameters are device pointers (from cz_dev_alloc or any HIP allocation).
 *
 * Per-env state travels as a flat "record" of cz_record_words() little-endian uint32 words:
 *   word 0 t | 1 recipe-node marks (bit 8r+j) | 2 layout id | 3 status (1 done, 2 terminated, 4 truncated)
 *   | 4 episode | 5 recipe ids (4 x u8) | 6 layout-pool slice (base | count<<16) | 7 marks of recipes 2, 3 (wide recipe tables only) | 8..11 agents (x | y<<8 | orientation<<16 | (held slot+1)<<24)
 *   | 12..19 four float64 running episode returns (statistics only) | cells (W*H bytes: type | READY<<3 | TOGGLE<<4 | ACTIVE<<5 | WALK<<6) | dyn0[D] (x | y<<8 | class<<16 | flags<<24;
 *   flags: 1 alive, 2 chopped, 4 mashed, 8 free) | dyn1[D] ((plate slot+1) | seq<<8), padded to 16 words.
 * (normative description: cooking_zoo_amd/soa.py)
 *
 * WHERE THE REFERENCE RAISES, the step kernels do something defined instead (profiles/r05/deviations.md, generated from the
 * differential fuzz's histograms by tools/deviations.py):
 *   - EXECUTE in front of a READY Cutboard with empty content (TypeError, cooking_world.py:162 <- world_objects.py:250-269; reachable
 *     in scheme1: a mashed Banana on the board is absorbed by a Plate in hand): no-op, the board stays READY
 *     (tests/golden/refcrash_cutboard_*.npz hold the reference's own outputs past that step);
 *   - a scheme1 interaction aimed off the grid (IndexError): no-op;
 *   - max_steps reached while an agent is despawned (IndexError, cooking_env.py:337): the step truncates;
 *   - a respawn that finds no free cell in 1001 tries, or a candidate beyond the grid (ValueError, parsing.py:159,166): the agent stays
 *     where it is and cz_spawn_exhausted counts it;
 *   - a level draw of cz_generate_layouts that fails - no position for an object in 10 001 tries or for an agent in 1 001, more
 *     objects of a class than the meta file lists ("Too many X objects loaded"), more object slots than max_dyn (ValueError,
 *     parsing.py:44,73,99,112,137,149), a second Switch (AttributeError on its first press): the pool slot keeps the layout it held
 *     and cz_generate_failures counts it.
 * Refused before anything runs: a level with two Switches, action scheme 2, more than 4 agents (the reference's own limits or crashes).
 */
#ifndef COOKINGZOO_H
#define COOKINGZOO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The one place the ABI number lives: cz_abi_version() returns it, cooking_zoo_amd/_native.py parses it from this file
 * and refuses a library that reports another one, __graft_entry__.build() and the tests compare against it. */
#define CZ_ABI_VERSION 10

typedef struct cz_handle_s *cz_handle;

/* Batch configuration.  Mirrors the kwargs of CookingEnvironment.__init__ (cooking_env.py:62-64) that
 * reach the step path, plus the batch geometry. */
typedef struct cz_config {
    int32_t num_envs;            /* env instances owned by this handle (one wavefront each)          */
    int32_t num_agents;          /* A <= 4            (cooking_env.py:76, COLORS cooking_world.py:21) */
    int32_t width, height;       /* grid, W <= 32, H <= 32 (parsing.py:17-18)                         */
    int32_t max_dyn;             /* D dynamic-object slots per env, <= 255                            */
    int32_t feat_len;            /* F features per agent (cooking_env.py:114-117)                     */
    int32_t action_scheme;       /* 1 or 3            (cooking_env.py:60; scheme2 is dead upstream)   */
    int32_t max_steps;           /* truncation horizon (cooking_env.py:333-334)                       */
    int32_t end_condition_all;   /* end_condition_all_dishes (cooking_env.py:310-313)                 */
    int32_t num_recipes;         /* recipe graphs per env, num_agents <= R <= 4 (cooking_env.py:106)  */
    int32_t auto_reset;          /* 0: finished envs freeze until cz_reset; 1: the step after `done`
                                    re-instantiates the env from the layout pool (next-step autoreset) */
    int32_t device_id;           /* HIP device ordinal                                                */
    int64_t env_id_base;         /* global id of env 0 of this handle (shard offset; keys layout draws
                                    and the on-device action stream so results do not depend on sharding) */
    double recipe_reward, max_time_penalty, recipe_penalty, recipe_node_reward;   /* cooking_env.py:79-80 */
} cz_config;

/* Episode statistics of one handle (one GPU): what the reference reports through `infos`
 * (cooking_env.py:248,264,329), aggregated on the device. */
typedef struct cz_stats {
    uint64_t env_steps;              /* world steps executed (reset passes excluded)   */
    uint64_t episodes;               /* episodes finished                              */
    uint64_t length_sum;             /* sum of finished-episode lengths                */
    uint64_t truncations;            /* episodes that ended by t >= max_steps          */
    uint64_t terminations;           /* episodes that ended by recipe completion       */
    uint64_t recipes_completed[4];   /* per agent slot: episodes ending with its recipe complete */
    double return_sum[4];            /* per agent slot: sum of finished-episode returns */
} cz_stats;

/* The un-aggregated form: the last episode one env finished, as the reference reports it through `infos` at the step that ends an
 * episode (cooking_env.py:248,264,329) - one entry of cz_episodes_collect's packed list. */
typedef struct cz_episode {          /* cz_sizeof_episode() */
    int64_t  env;                    /* GLOBAL env id (env_id_base + e) */
    uint32_t episode;                /* index of the episode in its env (the record's episode word while it ran) */
    uint32_t length;                 /* world steps of the episode */
    uint32_t flags;                  /* bit 0 terminated; bit 1 truncated; bit 4 + a: recipe a was complete at the end */
    uint32_t finished;               /* episodes this env finished since the last collect (>= 1; > 1: the ones before this one are not itemised) */
    double   ret[4];                 /* per agent slot; slots >= A are 0.0 */
} cz_episode;
#define CZ_EPISODE_TERMINATED 1u
#define CZ_EPISODE_TRUNCATED 2u
#define CZ_EPISODE_ROOT0 16u         /* << a */

/* ---- lifetime ------------------------------------------------------------------------------------- */
int cz_create(const cz_config *cfg, cz_handle *out);
int cz_destroy(cz_handle h);
const char *cz_last_error(cz_handle h);
int32_t cz_record_words(cz_handle h);
int32_t cz_abi_version(void);
int32_t cz_sizeof_config(void);                           /* sizeof(cz_config), for binding self-checks */
int32_t cz_sizeof_stats(void);
int32_t cz_sizeof_episode(void);                          /* sizeof(cz_episode) */
int cz_debug_set_stamps(cz_handle h, void *d_buf);       /* diagnostic builds only (make prof): phase stamp buffer */
/* timeline builds only (make timeline, tools/timeline.py): every step-kernel launch k writes two uint64 per env - entry and
 * exit time of the env's wave on the device-wide 100 MHz clock, with the hardware ids in the upper halves - to
 * d_buf + (k % cap_launches) * num_envs * 2 */
int cz_debug_set_timeline(cz_handle h, void *d_buf, int32_t cap_launches);
int cz_sync(cz_handle h);                                  /* wait for the handle's stream */
/* Order all further work of this handle on a HIP stream of the caller (hipStream_t; e.g. the stream a framework runs its
 * policy on: device-pointer steps then need no host synchronisation on either side).  NULL restores the handle's own
 * stream.  The stream must belong to the handle's device and outlive its use here. */
int cz_set_stream(cz_handle h, void *hip_stream);
/* STREAM CAPTURE.  While that stream is being captured by the caller (hipStreamBeginCapture, torch.cuda.graph), the
 * device-pointer calls - cz_step_device, cz_step_device_compact, cz_step_device_f32, cz_step_device_many / _ring, cz_rollout*,
 * cz_observe_device, cz_observe_device_f32, cz_observe_grid_device, cz_navigate_device, cz_partner_device, cz_action_effects_device, cz_render_device, cz_reset_device, cz_set_tasks_device, cz_infos_device, cz_save_device, cz_restore_device, cz_episodes_collect, cz_probe_policy - are pure kernel launches and legal inside the capture: nothing is queried or synchronised (a layout update
 * staged by cz_update_layouts stays staged until the first call outside the capture; ring runs go out as plain launches).  Replays
 * of the caller's graph then do exactly what the captured launches did (cooking_env.py:243-288 once per captured step).  Calls
 * that copy to / from the host or wait (cz_step, cz_reset, cz_get_state, cz_sync, cz_get_stats, cz_update_layouts,
 * cz_set_layout_group ...) are not; the last two say so, the others fail with HIP's own error.  (cz_generate_layouts is a pure
 * launch too, and so is a cz_set_layout_group that only changes the active part: see there.)  The captured launches carry the
 * table pointers of their time: after cz_load_layouts / cz_load_recipes / cz_set_spawn / cz_set_compact_output /
 * cz_set_f32_output capture again.
 * cz_stream_capturing: 1 while the handle's stream is a stream of the caller that is being captured, else 0 - a host layer that
 * keeps count of the steps it issued (cooking_zoo_amd: layout rotation schedules) must not count captured launches as steps:
 * they run when the caller's graph is replayed, as often as it is replayed. */
int32_t cz_stream_capturing(cz_handle h);

/* ---- tables ---------------------------------------------------------------------------------------- */
/* Recipe graphs: replaces RECIPES[name]() / Recipe.node_list (recipe_drawer.py:109-118, recipe.py:29-34).
 * max_nodes = 8 (compact): table[n][9], word 0 = node count (<= 8), then per node (root first, node_list order)
 *   class | condition<<8 | child-mask<<16 | counts-in-goal-sum<<24; the marks of recipe r are bits 8r.. of record word 1.
 * max_nodes = 16 (wide, for books with a graph of more than 8 nodes): table[n][33], word 0 = node count (<= 16), then per
 *   node TWO words: class | condition<<8 | counts<<24, child-mask (16 bits); marks are 16 bits per recipe: recipes 0, 1 in
 *   record word 1, recipes 2, 3 in word 7.  Wide batches re-evaluate every recipe on every step that changed an object.
 * class: 0..6 static type, 16..25 dynamic class, 255 none; condition: 0 none, 1 chopped, 2 mashed, 3 not chopped,
 * 4 not mashed, or 0x10 | accept mask over the object state (chopped | mashed << 1) for several (attr, value) conditions
 * on one node (recipe.py:96-98 loops over all of them). */
int cz_load_recipes(cz_handle h, const uint32_t *table, int32_t n_recipes, int32_t max_nodes);

/* Layout pool: replaces load_level / parsing (load_level.py:55-71, parsing.py:5-151) results.  Per layout:
 * its initial record (cz_record_words words; t, marks, status ignored) and its observation descriptor
 * (feat_len words, op | ref<<8; ops listed in cooking_zoo_amd/soa.py) which encodes the meta-file class
 * order and per-class list order that get_feature_vector (cooking_env.py:352-373) iterates. */
int cz_load_layouts(cz_handle h, const uint32_t *init_records, const uint32_t *obs_desc, int32_t n_layouts);

/* Fresh layouts under a stepping batch (the reference draws a new level at every reset, cooking_env.py:191-195,
 * parsing.py:21-151; the device redraws from the resident pool).  cz_update_layouts replaces pool slots
 * [first, first + count) - same formats as cz_load_layouts - without touching the handle's stream: the tables stay where they
 * are, the caller's arrays are free again on return, and the copy runs on a stream of the library's own, issued once every
 * step issued before the call has completed (checked at later call boundaries, never a device-side wait) and not waited for
 * by later steps.  Never replace slots that envs can still draw or are still
 * playing on: cz_set_layout_group(h, groups, active) cuts every env's pool slice into `groups` equal parts and lets the envs
 * draw their next episodes from part `active` only (1, 0 = the whole slice, the default), from the next step on (stream
 * order); it waits - on the device - for the updates issued so far, so no env draws a half-written slot.  Rotation:
 * switch to part b; issue at least max_steps + 1 more steps (every episode that started on part a has ended); update
 * part a; ... (cooking_zoo_amd.vec_env.CookingVecEnv.rotate_layouts does this with a background process).  Every pool slice's
 * length must be a multiple of `groups`.  cz_update_layouts with count 0 only creates the copy stream and the staging block
 * (so that the first real update does not pay for them).  cz_layout_updates: slots replaced so far. */
int cz_update_layouts(cz_handle h, int32_t first, int32_t count, const uint32_t *init_records, const uint32_t *obs_desc);
int cz_set_layout_group(cz_handle h, int32_t groups, int32_t active);
int64_t cz_layout_updates(cz_handle h);

/* Fresh layouts DRAWN ON THE DEVICE: what parse_level_layout / parse_static_objects / parse_dynamic_objects / parse_agents
 * (parsing.py:5-18, 21-76, 79-115, 118-151) do at every reset of the reference (cooking_env.py:191-195), one wavefront per pool
 * slot, followed by what cooking_zoo_amd/cooking_world/layout.py makes of the result (initial record, observation descriptor in
 * the order get_feature_vector iterates, cooking_env.py:352-373).  No producer process, no host arrays, no PCIe.
 * DRAWS.  The n-th draw of pool slot s in generation g under `seed`, counted in the reference's call order - one random() per
 * placement attempt of an OPTIONAL object, then random.sample(X_POSITION, 1), random.sample(Y_POSITION, 1) - is
 * cz_spawn_uniform(seed, env_global = s, episode = 0, t = g, agent = 0x100, draw = n), and a coordinate is
 * candidates[(int)(u * n_candidates)].  s is the index in the whole pool, so every shard of a sharded batch generates the same
 * bytes.  Host model: engine/load_level.py instantiate with level_program.KeyedDraws; tests/golden/layouts_keyed_ref.json holds what
 * the unmodified reference parser returns under this stream.
 * cz_load_level_programs: `programs` holds n_levels (1..255) level programs one after the other, `words` uint32 in all - the
 * level file, the meta file and the batch geometry as flat words (cooking_zoo_amd/cooking_world/engine/level_program.py
 * compile_level documents them) -; level_of_slot[i] (NULL: all 0) is the level that pool slot i is drawn from, one byte per
 * slot of the resident pool.  Validates (class codes, offsets, candidates within [0, width] x [0, height] - the reference raises
 * on a drawn position beyond that, parsing.py:34 - geometry and feature length against the handle) and uploads; call it again
 * after cz_load_layouts.
 * cz_generate_layouts: ONE launch on the handle's stream that redraws slots [first, first + count) with generation
 * `generation`.  Stream-ordered with the steps issued before and after it and with cz_set_layout_group; nothing is allocated,
 * copied or waited for, so it is legal while the caller captures that stream (as is a cz_set_layout_group that only switches
 * the active part of a cut already in place, with no cz_update_layouts outstanding).  The rule of cz_update_layouts holds:
 * never redraw slots that envs can still draw or are still playing on.  Once the pool is cut into groups > 1 parts, a range that
 * touches the part the envs draw from is refused (the parts are taken per run of slots of one level in level_of_slot - the
 * pool slices cooking_zoo_amd uses); with one group it is the caller's duty, which allows filling the pool before the first
 * reset.  Inside a capture the checks see the state at capture time.  Counts into cz_layout_updates (when issued or captured).
 * A draw that fails (see the deviations above) leaves the slot's record and descriptor as they were;
 * cz_generate_failures: how many did since cz_load_level_programs (waits for the stream), -1 on error. */
int cz_load_level_programs(cz_handle h, const uint32_t *programs, int64_t words, int32_t n_levels, const uint8_t *level_of_slot);
int cz_generate_layouts(cz_handle h, int32_t first, int32_t count, uint64_t seed, uint32_t generation);
int64_t cz_generate_failures(cz_handle h);

/* Agent despawn / respawn (cooking_world.py:267-290 handle_agent_spawn, despawn_agent, respawn_agent; parsing.py:154-167
 * generate_location) for every world of the batch, evaluated by the step kernels themselves - on every path: cz_step,
 * cz_step_device*, ring runs, cz_rollout, cz_rollout_actions.  The reference takes its draws from numpy's process-global
 * stream, which defines them for one world per process; here every draw comes from a counter-based stream keyed by (seed,
 * global env id, episode << 32 | t, agent, draw index) (cz_spawn_uniform is the host mirror), so results depend neither on the
 * batch size nor on the sharding nor on the launch form; tests/golden/spawn_keyed_*.npz are trajectories of the unmodified
 * reference functions fed with exactly these draws.  The record's status word carries a "despawned" bit per agent (bit 8 +
 * agent) and a grace countdown each from bit 12 on: 5 bits wide while grace_period <= 31, else 20 / num_agents bits (so grace_period may be
 * up to 1023 for two agents, 63 for three, 31 for four; the reference takes any int, parsing.py:142).  A despawned agent does not act (whatever its action
 * says), is reported truncated in the step it leaves, and stays in the world as an obstacle; an agent that holds something stays.
 * TAKES EFFECT WITH THE NEXT STEP: worlds reset from then on start with everybody present and the grace period running
 * (parsing.py:142); episodes that are already running continue with whatever their status words hold (grace 0 unless the
 * caller set it), i.e. they draw from their next step on.  A call that moves grace_period across 31 changes the width of the
 * countdown fields: the resident records are re-packed to the new width by the call itself (a countdown that does not fit the
 * narrower field becomes 31).  A record does not say which width it was packed with: cz_set_state takes records in the width
 * of the handle's CURRENT grace_period (records saved under the other width must be re-packed by the caller,
 * cooking_zoo_amd/spawn.py decode_status / status_bits).  Rates 0, 0 switch it off.
 * Spawn areas (the level files' AGENTS entries, parsing.py:118-151) are per level: level_of_layout[i] (NULL: all 0) is the
 * level that layout i of the resident pool instantiates - call again after cz_load_layouts changed the pool size -,
 * spawn_x / spawn_y are [n_levels][num_agents][stride] candidate coordinates, n_x / n_y [n_levels][num_agents] how many of
 * them count (1..stride, stride <= 1024).  Differences from the reference, which raises in both cases: a candidate outside the
 * grid is skipped, and a respawn that finds no free Floor cell in 1001 tries puts the agent back where it stood -
 * cz_spawn_exhausted counts those. */
int cz_set_spawn(cz_handle h, double despawn_rate, double respawn_rate, int32_t grace_period, uint64_t seed,
                 int32_t n_levels, const uint8_t *level_of_layout, int32_t stride, const uint8_t *spawn_x, const int32_t *n_x,
                 const uint8_t *spawn_y, const int32_t *n_y);
int64_t cz_spawn_exhausted(cz_handle h);
double cz_spawn_uniform(uint64_t seed, int64_t env_global, uint32_t episode, uint32_t t, int32_t agent, uint32_t draw);

/* ---- state ----------------------------------------------------------------------------------------- */
int cz_set_state(cz_handle h, int64_t env_begin, int64_t env_count, const uint32_t *records);
int cz_get_state(cz_handle h, int64_t env_begin, int64_t env_count, uint32_t *records);

/* reset(): cooking_env.py:178-210.  Re-instantiates envs [env_begin, env_begin+env_count) from
 * layout_ids[i], assigns recipe_ids[i][0..3] (0xFF = unused) and pool_words[i] (base | count<<16: the slice of
 * the layout pool the env redraws from under auto_reset; NULL = whole pool), evaluates the recipe marks of the
 * fresh world (cooking_env.py:197-198) and, if obs != NULL (host, [env_count][A][F] float64), returns observe(). */
int cz_reset(cz_handle h, int64_t env_begin, int64_t env_count, const int32_t *layout_ids,
             const uint8_t *recipe_ids, const uint32_t *pool_words, double *obs);

/* reset() (cooking_env.py:178-210) for CHOSEN envs of the handle, decided and carried out on the device: every pointer is a device
 * pointer, the call is ONE kernel launch on the handle's stream - no copy, no query, no wait; legal inside a stream capture - and
 * takes no env-step, unlike the next-step auto-reset pass.  With auto_reset = 0 it is what un-freezes finished envs without a
 * host round trip.
 * Chosen: d_mask == NULL - every env whose status word has the done bit (what the auto-reset pass would restart); otherwise d_mask is
 * uint8 [N] and env e is chosen when d_mask[e] != 0, finished or in mid-episode.
 * A chosen env: episode += 1; its layout is d_layout_ids[e] when d_layout_ids != NULL and d_layout_ids[e] >= 0 (any slot of the
 * pool, as in cz_reset), else the keyed draw of the auto-reset pass - cz_next_layout_group(env_id_base + e, new episode, the
 * record's pool word, n_layouts, groups, active) with the layout-control words of cz_set_layout_group.  The rest is cz_reset's work:
 * the record is the pool's init record, t = 0, status 0 (everybody present and the grace period running while despawn / respawn is
 * on), recipe ids and pool word kept from the old record, the recipe marks evaluated on the fresh world (cooking_env.py:197-198),
 * the running returns zeroed.
 * An explicit layout id >= n_layouts is REFUSED: the env stays exactly as it was - no episode bump, no row - and a device counter is
 * incremented; cz_reset_device_refused reads it (envs refused since cz_create; waits for the stream; -1 on error).
 * Statistics: a chosen env that was not done adds its t to the env-step count, as cz_reset does (no episode is counted for it);
 * cz_get_stats after this call equals cz_get_stats after cz_reset calls on the same envs.
 * Outputs, each may be NULL and each is laid out for the WHOLE batch: d_obs float64 [N][A][F], d_obs32 float [N][A][F] (dense, the
 * rounding of cz_step_device_f32), d_codes uint8 [N][A][cz_codes_pitch] (padding 255) - observe() (cooking_env.py:271,352-373) of
 * the fresh world in rows e of the chosen, not refused envs; every other byte stays untouched, so after a step has written
 * everyone's rows the call overwrites just the rows of the envs that restarted.  cz_set_compact_output / cz_set_f32_output are
 * ignored, as the rollouts ignore them. */
int cz_reset_device(cz_handle h, const uint8_t *d_mask, const int32_t *d_layout_ids,
                    double *d_obs, float *d_obs32, uint8_t *d_codes);
int64_t cz_reset_device_refused(cz_handle h);

/* SAVE, RESTORE AND FORK env states on the device.  A record is a self-contained value - layout id, recipe ids, pool slice, status,
 * episode, t, marks, running returns, cells and objects, cz_record_words words in all - so an ARCHIVE of records in device memory,
 * d_records = uint32 [capacity][cz_record_words], owned by the caller, is all that tree search, archives of interesting states,
 * restarts from saved curriculum states or copying the best env over the worst need.  Every pointer is a device pointer; each call
 * is ONE kernel launch on the handle's stream - no copy, no query, no wait; legal inside a stream capture - and no step (the
 * host-pointer way is cz_get_state / cz_set_state, which copy and wait).  The archive must not overlap memory of the handle.
 *
 * cz_save_device: env e writes its whole record, the running-return words included, to row d_slot[e].  d_slot == NULL: row e, and
 * capacity >= num_envs is required (checked on the host, before anything is launched).  A negative slot skips the env.  A slot >=
 * capacity writes nothing, and NO counter is kept for it.  Two envs that name the same row leave that row unspecified: distinct rows
 * are the caller's contract.  Nothing of the handle changes.
 *
 * cz_restore_device: env e takes row d_slot[e]; d_slot == NULL: row e, capacity >= num_envs required as above.  A negative slot
 * leaves the env alone (its wavefront reads that one word and leaves).  ANY NUMBER of envs may name the same row: that is the fork.
 * A chosen env's record becomes the row word for word: its layout id, recipe ids and pool word, its status with the despawn bits
 * and grace countdowns, its episode word, t, recipe marks and running returns.  Keyed draws stay keyed by the env's own global id
 * (env_id_base + e) - the layout an auto-reset takes, the on-device action stream of cz_rollout, despawn / respawn draws - so forks
 * of one state DIVERGE wherever a draw is made, and stay identical where none is (same actions, no auto-reset, no spawn draws).
 * REFUSED: a row is checked on the device before any word of it is used as an index, by the checks of cz_set_state - layout id <
 * n_layouts, each of the num_recipes recipe ids < the recipe table's size, the pool slice inside the pool, no slot that is not alive
 * but carries a container tag.  An env whose slot is >= capacity or whose row fails stays exactly as it was, none of its output rows
 * is touched, and a device counter is incremented; cz_restore_device_refused reads it (envs refused since cz_create; waits for the
 * stream; -1 on error).
 * Statistics: env_steps keeps meaning steps this handle took.  A restored env adds the old record's t to its step count if the old
 * record was not done (an episode cut short: its steps stay counted, as after cz_reset) and subtracts the new record's t if the new
 * record is not done (steps that arrive already taken, as cz_reset_stats treats episodes in flight).  No episode is counted; the
 * env's last-episode row is left alone, so an episode cut short by a restore leaves no record in cz_episodes_collect; a restored
 * episode that later ends reports the record's whole length and the inherited return plus the later rewards in step order.
 * Outputs, each may be NULL and each is laid out for the WHOLE batch: d_obs float64 [N][A][F], d_obs32 float [N][A][F] (dense, the
 * rounding of cz_step_device_f32), d_codes uint8 [N][A][cz_codes_pitch] (padding 255) - observe() (cooking_env.py:271,352-373) of
 * the restored state in rows e of the chosen, not refused envs; every other byte stays untouched.  cz_set_compact_output /
 * cz_set_f32_output are ignored.
 * The caller keeps the archive consistent with the layout pool: a record saved before its layout slot was rewritten
 * (cz_update_layouts, cz_generate_layouts) restores its own cells and objects but is encoded with the slot's CURRENT descriptor row.
 * This is not checked. */
int cz_save_device(cz_handle h, const int32_t *d_slot, uint32_t *d_records, int64_t capacity);
int cz_restore_device(cz_handle h, const int32_t *d_slot, const uint32_t *d_records, int64_t capacity,
                      double *d_obs, float *d_obs32, uint8_t *d_codes);
int64_t cz_restore_device_refused(cz_handle h);

/* observe() (cooking_env.py:271,352-373) of the current state of envs [env_begin, env_begin+env_count):
 * host buffer [env_count][A][F] float64. */
int cz_observe(cz_handle h, int64_t env_begin, int64_t env_count, double *obs);
/* ... the same observation in its compact form (see cz_step_device_compact): host buffer uint8 [env_count][A][cz_codes_pitch]. */
int cz_observe_compact(cz_handle h, int64_t env_begin, int64_t env_count, uint8_t *codes);
/* ... and into DEVICE buffers, float64 rows [env_count][A][F] and / or codes [env_count][A][cz_codes_pitch] (either may be NULL):
 * the first observation of a consumer that stays on the device, after cz_reset / cz_set_state.  Stream-ordered, nothing is
 * synchronised. */
int cz_observe_device(cz_handle h, int64_t env_begin, int64_t env_count, double *d_obs, uint8_t *d_codes);
/* ... and as FLOAT32 rows (cooking_env.py:271,352-373 in the dtype of cz_step_device_f32): device buffer float [env_count][A][F],
 * dense.  Stream-ordered, nothing is synchronised. */
int cz_observe_device_f32(cz_handle h, int64_t env_begin, int64_t env_count, float *d_obs32);

/* The GRID observation: the spatial state tensor the reference declares for obs_spaces=["full"] - a (width, height,
 * graph_representation_length) tensor next to agent_location and goal_vector (cooking_env.py:118-123, 274-278), allocated at
 * cooking_env.py:149-150 and never written upstream - filled from the per-object vectors every class of world_objects.py carries
 * (numeric_state_representation(), state_length(); 32 channels in GAME_CLASSES order, all 0 / 1, the maximum where objects of a
 * class share a cell).  extended = 1 appends 16 channels the reference vectors leave out (mashed food, free / held / in-plate,
 * appliance and switch state, which agent stands where); cooking_zoo_amd/grid.py names every channel and is the host model.
 * Cell (x, y) is at index x * H + y - the reference's (W, H, C) per env - in every form, C = cz_grid_channels(extended):
 *   d_bits    uint32 [env_count][W][H][C / 32]   channel c = bit c & 31 of word c >> 5           (8-byte aligned)
 *   d_grid8   uint8  [env_count][W][H][C]        0 / 1                                           (16-byte aligned)
 *   d_grid32  float  [env_count][W][H][C]        exactly 0.0f / 1.0f                             (16-byte aligned)
 *   d_agent_xy int32 [env_count][A][2]           the agent_location entry
 * Any of the four may be NULL (not all); every channel of every cell of a named form is written.  env_count == 0 returns 0.
 * Refused: all four NULL, extended other than 0 / 1, a range outside the batch.  Stream-ordered on the handle's stream: no copy, no
 * wait, no query - legal inside a stream capture of the caller. */
int cz_observe_grid_device(cz_handle h, int64_t env_begin, int64_t env_count, int32_t extended,
                           uint32_t *d_bits, uint8_t *d_grid8, float *d_grid32, int32_t *d_agent_xy);
int32_t cz_grid_channels(int32_t extended);     /* 32 or 48; -1 for any other argument */

/* Shortest-path NAVIGATION: walk_to_location and reachable of the reference's scripted partner (cooking_agents/base_agent.py:62-126)
 * for every agent of every env and T candidate goals each, from the current records.  The reference searches breadth first from the
 * agent's cell over the observation's Floor tiles, the goal cell admitted whatever it is, neighbours in the order of the walk codes
 * 1:(-1,0) 2:(+1,0) 3:(0,+1) 4:(0,-1), and returns the first move of the first path found - the lexicographically smallest shortest
 * path.  Here one flood fill from the goal gives field[c] (0 at the goal; for a Floor cell the length of the shortest path from the
 * goal that enters Floor cells only; 0xFFFF everywhere else), and for the agent's cell s: s == goal gives action 0, steps 0;
 * otherwise the neighbour of s with the smallest finite field wins, the first code on ties: action = its code, steps = field + 1;
 * no such neighbour: action 0, steps -1.  reachable(a, b) of the reference is steps >= 0.  cooking_zoo_amd/nav.py is the host model.
 *   d_target int32  [env_count][A][T][2]    x, y per agent and candidate                              (4-byte aligned)
 *   d_action int32  [env_count][A][T]       0..4, the walk codes both action schemes share; with T = 1 the [N][A] array cz_step_device takes
 *   d_steps  int32  [env_count][A][T]       path length, 0 at the goal, -1 unreachable / no target
 *   d_field  uint16 [env_count][A][T][W*H]  cell (x, y) at x * H + y as in the grid observation; 0xFFFF unreachable (2-byte aligned)
 * Any of the three outputs may be NULL (not all).  T in 1..cz_nav_max_targets(); flags: known bits only.  env_count == 0 returns 0.
 * Deviations from the reference: a target with a coordinate outside [0, W) x [0, H) is "no target" - action 0, steps -1, field all
 * 0xFFFF; (-1, -1) is the padding value (the reference would walk towards an off-grid goal next to a floor tile); a despawned agent is
 * routed from its stored location; the reference's reachable() cache can answer from a stale world, there is no cache here.
 * Refused: all three outputs NULL, d_target NULL, T outside 1..8, unknown flag bits, a range outside the batch.  Stream-ordered on
 * the handle's stream: no copy, no wait, no query, no allocation - legal inside a stream capture of the caller; the records are
 * only read. */
#define CZ_NAV_WALKABLE_BLOCKS 1u  /* a Block whose walkable bit is set counts as floor too (what world_step lets an agent enter);
                                      default: Floor cells only, what BaseAgent sees */
int32_t cz_nav_max_targets(void);  /* 8 */
int cz_navigate_device(cz_handle h, int64_t env_begin, int64_t env_count, int32_t T, uint32_t flags,
                       const int32_t *d_target, int32_t *d_action, int32_t *d_steps, uint16_t *d_field);

/* The SCRIPTED PARTNER: the action the reference's heuristic CookingAgent (cooking_agents/cooking_agent.py:9-119,
 * base_agent.py:128-198) returns, for the chosen agents of every env, from the current records - which object to walk to (recipe
 * marks of the asked recipe, the unmarked node with the highest index, the condition branch with generic_sequence, the contains
 * branch) and the first move of that walk (cz_navigate_device's).  cooking_zoo_amd/partner.py is the definition and the host model.
 *   agents   bit a set: agent a is driven; the entries of every other agent are left untouched in ALL outputs, so a learner's actions
 *            and the partner's can share the one [N][A] array cz_step_device takes.  0, or a bit at or above A, is refused.
 *   d_recipe int32 [env_count][A]     indices into the loaded recipe table; NULL: the env's own recipe of slot a (record word 5; 0xFF:
 *                                     DONE).  An index outside the table gives that agent IDLE and adds one to cz_partner_bad_recipes.
 *   d_action int32 [env_count][A]     0..4, the walk codes both action schemes share
 *   d_target int32 [env_count][A][2]  the location handed to the walk whose result is the action, (-1, -1) when no walk produced
 *                                     it: directly a T = 1 target array of cz_navigate_device
 *   d_status uint8 [env_count][A]     CZ_PARTNER_DONE every node marked, or the recipe slot unused (action 0); _WALK the action is the
 *                                     result of a walk to the target (0 at the goal or when it is unreachable); _IDLE the reference
 *                                     returns 0 without a walk; _RAISES the reference raises here (action 0); _ABSENT the agent's
 *                                     despawn bit is set (action 0; the reference's demo does not ask such an agent)
 * Any output may be NULL (not all).  flags must be 0.  env_count == 0 returns 0.  Needs the partner table (cz_load_partner_table:
 * the ordered conditions of every node, which the step kernels' accept masks lose) and the rank rows of the layout pool
 * (cz_load_layout_ranks; cz_generate_layouts writes them itself): the list order of the static objects, which decides ties between
 * equidistant Counters and appliances and which the records do not hold.  Deviations from the reference: those of
 * cz_navigate_device; a condition on an attribute the object's class lacks counts as unmet (the reference raises AttributeError);
 * a slot outside the grid or of no class is not an object, an agent outside the grid is IDLE (no valid record has either).
 * Refused: all three outputs NULL, agents 0 or a bit >= A, flags != 0, a range outside the batch, no partner table, a pool slot
 * without its rank row.  Stream-ordered on the handle's stream: no copy, no wait, no query, no allocation - legal inside a stream
 * capture of the caller; the records are only read. */
#define CZ_PARTNER_DONE 0
#define CZ_PARTNER_WALK 1
#define CZ_PARTNER_IDLE 2
#define CZ_PARTNER_RAISES 3
#define CZ_PARTNER_ABSENT 4
int cz_partner_device(cz_handle h, int64_t env_begin, int64_t env_count, uint32_t agents, uint32_t flags,
                      const int32_t *d_recipe, int32_t *d_action, int32_t *d_target, uint8_t *d_status);
int64_t cz_partner_bad_recipes(cz_handle h);   /* agents asked for a recipe outside the table since cz_load_partner_table; waits */
/* one row of cz_partner_row_words() (33) words per recipe of the table cz_load_recipes loaded, from the same graphs: the node count;
 * then per node  class | number of conditions << 8 | child mask << 16  and the conditions in the node's own order, 4 bits each:
 * attribute (0 chop_state, 1 blend_state) | wanted value << 1 (0 fresh, 1 chopped / in progress, 2 mashed); at most 8 per node */
int32_t cz_partner_row_words(void);
int cz_load_partner_table(cz_handle h, const uint32_t *rows, int32_t n_recipes);   /* after every cz_load_recipes, which drops the table */
/* rank rows of pool slots [first, first + count): uint16 [count][W*H], the position of every cell's static object in the reference's
 * world_objects[class] list.  After cz_load_layouts / cz_update_layouts of those slots; the array is free again on return and the
 * rows are in place before anything issued later on the handle's stream runs (the caller's thread does not wait); not inside a capture.
 * The copy starts at once, on a stream of the library's own: it is NOT ordered behind cz_partner_device launches already issued, so -
 * as for cz_update_layouts - only for slots that no env plays on or can draw (nothing checks this).  The wait is put on the stream
 * the handle has at the time of the call: after a later cz_set_stream, cz_sync (or a wait of your own) before the next cz_partner_device. */
int cz_load_layout_ranks(cz_handle h, int32_t first, int32_t count, const uint16_t *ranks);

/* TASKS: which recipes an env plays, changed and read on the device.  The reference fixes them in the constructor and rebuilds their
 * graphs at every reset() (cooking_env.py:197-201); its infos carry recipe_done and task per agent (cooking_env.py:317-331) and the
 * "full" observation goal_vector = recipe_mapping[agent].goals_completed(num_goals) (cooking_env.py:277, recipe.py:36-40).
 * cooking_zoo_amd/tasks.py is the definition and the host model of both calls.
 *
 * cz_load_goal_table: goal_ids uint8 [n_recipes][16] - the goal id (RecipeNode.id_num, recipe.py:16) of node j of recipe r, 0xFF past
 *   the recipe's last node - and num_goals, the length of a goal vector (1..255; cooking_env.py:100-105).  n_recipes must be the
 *   loaded recipe table's; an id of a node must be < num_goals (the reference raises IndexError there, recipe.py:34).  After every
 *   cz_load_recipes, which drops the table; not inside a capture.  cz_num_goals: num_goals, -1 before a table is loaded / null handle.
 *
 * cz_set_tasks_device: lines 197-201 of reset() applied to fresh graphs of OTHER names on the env's current world, for chosen envs.
 *   d_mask        uint8 [N] or NULL   env e is chosen when d_mask[e] != 0, in mid-episode or finished (a finished env's status word is
 *                                     not touched: it stays done until it is reset).  NULL: every env whose record has t == 0 - the
 *                                     start of an episode, after cz_reset, cz_reset_device or the auto-reset pass; a finished env has
 *                                     t >= 1 and is never chosen this way.
 *   d_recipe_ids  uint8 [N][4]        the new ids of env e: row e.  NULL: row task_draw(seed, env_id_base + e, the record's episode
 *   d_task_list   uint8 [K][4]        word, K) = min((int)(u * K), K - 1) of d_task_list, u = cz_spawn_uniform(seed, env_id_base + e,
 *                                     episode, 0, 0x200, 0): the project's one counter-based stream under a key nobody else uses
 *                                     (spawn draws: agents 0..3, cz_generate_layouts: 0x100).  Keyed by the episode word, so calling
 *                                     it after every step is idempotent, with auto_reset = 1 and 0 alike.
 *   A chosen env: record word 5 becomes the new ids (the bytes of slots >= num_recipes are ignored and stored as 0xFF), every recipe's
 *   marks are evaluated from scratch on the current world (word 1, and word 7 for wide tables); everything else in the record - t,
 *   status, episode, pool word, running returns, cells, objects - stays byte for byte, no statistics change, and the last-episode
 *   row of cz_episodes_collect is left alone.  Any id of the table is valid for every step kernel the handle can select: what
 *   cz_load_recipes derives for them it derives from the whole table.  An id >= n_recipes in one of the first num_recipes slots is
 *   checked on the device before it is used: the env is refused - it stays word for word as it was - and cz_set_tasks_refused
 *   counts it (envs refused since cz_create; waits for the stream; -1 on error).
 *   Refused on the host, before anything is launched: both sources NULL, a list with K < 1, the source in use not 4-byte aligned
 *   (with an id array the list is ignored, whatever it is).
 *   One launch on the handle's stream: no copy, no query, no wait, no allocation - legal inside a stream capture of the caller;
 *   outside one a layout update staged by cz_update_layouts is flushed first, as by cz_reset_device and every device-pointer call.
 *
 * cz_infos_device: the task state of envs [env_begin, env_begin + env_count) on the current records, any subset of five outputs
 *   (not none):
 *   d_goal8       uint8 [n][A][G]     G = num_goals.  The goal vector of agent a is that of recipe slot a (recipe_mapping,
 *   d_goal32      float [n][A][G]     cooking_env.py:201): [id] = 1 while the LAST node of node_list that carries goal id `id` is
 *                                     not marked, 0 once it is, and 0 for ids no node of the recipe carries; float: 0.0 / 1.0
 *   d_recipe_done uint8 [n][A]        the root's mark (infos[agent]["recipe_done"])
 *   d_task        int32 [n][A]        the recipe's index in the loaded table (infos[agent]["task"] names it)
 *   d_t           int32 [n]           the record's step counter
 *   Refused: no goal table for the loaded recipes, all five NULL, a range outside the batch.  env_count == 0 returns 0.  One launch:
 *   no copy, no query, no wait, no allocation - legal inside a stream capture of the caller; the records are only read. */
int cz_load_goal_table(cz_handle h, const uint8_t *goal_ids, int32_t n_recipes, int32_t num_goals);
int32_t cz_num_goals(cz_handle h);
int cz_set_tasks_device(cz_handle h, const uint8_t *d_mask, const uint8_t *d_recipe_ids, const uint8_t *d_task_list, int32_t K,
                        uint64_t seed);
int64_t cz_set_tasks_refused(cz_handle h);
int cz_infos_device(cz_handle h, int64_t env_begin, int64_t env_count, uint8_t *d_goal8, float *d_goal32, uint8_t *d_recipe_done,
                    int32_t *d_task, int32_t *d_t);

/* ACTION EFFECTS AND MASKS: which of an agent's actions would do anything at all, from the current records (the PettingZoo
 * `action_mask` convention; the reference offers none).  cooking_zoo_amd/effects.py is the definition and the host model.
 * For an env whose done bit is clear, an agent a that is present, and an action code c of the env's scheme:
 *   - Codes are 0 .. n_actions - 1.  n_actions is 5 for scheme3 and 8 for scheme1 (cz_num_actions; action_scheme3.py:4-43,
 *     action_scheme1.py:4-40).
 *   - S0 is the record after world_step with every present agent playing 0.
 *   - Sc is the record after world_step with agent a playing c and every other present agent playing 0.
 *   - world_step means perform_agent_actions + progress_world + the linked interactions + the free-flag normalisation
 *     (cooking_world.py:104-108).
 *   - world_step here does NOT include handle_agent_spawn (cooking_world.py:109-112), t, recipe marks, rewards or flags.
 *   - A despawned agent takes no part, as in the step kernels (action -1).
 *   - S0 is not S: a running Blender progresses by itself.
 * effects[a][c] is a byte of five bits.  Each bit is a difference between Sc and S0, in the words a step would write:
 *   bit 0 CZ_EFFECT_MOVED    agent a's (x, y) differs
 *   bit 1 CZ_EFFECT_TURNED   agent a's orientation differs
 *   bit 2 CZ_EFFECT_HAND     agent a's held-slot field differs (picked up, put down, swapped)
 *   bit 3 CZ_EFFECT_OBJECTS  any dyn0 / dyn1 word differs (an object moved, changed state, was created, deleted, plated, delivered)
 *   bit 4 CZ_EFFECT_CELLS    any cell byte differs (appliance READY / TOGGLE, Switch, Block)
 * Other agents' words cannot differ while they play 0, so there is no bit for them.
 *   - effects[a][0] = 0.
 *   - mask[a][c] = 1 if c == 0 or (effects[a][c] & ~ignore) != 0, else 0.
 *   - ignore is a caller's bit set.  For example, CZ_EFFECT_TURNED makes "only turns on the spot" count as a no-op.
 * Special cases: a despawned agent gets mask = [1, 0, ...] and effects 0.  A finished env (done bit set) gets the same for every
 * agent: the next step resets or freezes it whatever is played.  Where the reference raises and the build has a defined no-op, the
 * effect is 0 like any no-op: EXECUTE on a READY Cutboard with empty content, and a scheme1 interaction aimed off-grid (DESIGN.md
 * section 2).
 * The one caveat: the mask speaks about one agent acting alone.  With several agents acting at once, the collision filter and the
 * serial interaction order can change what happens; that is what every per-agent action mask means.
 *   agents    bit a set: agent a is asked for; the rows of every other agent are left untouched in both outputs.  0, or a bit at
 *             or above A, is refused.
 *   ignore    CZ_EFFECT_ bits; a bit outside the five is refused.
 *   d_mask    uint8 [env_count][A][n_actions]   0 / 1
 *   d_effects uint8 [env_count][A][n_actions]   the bytes
 * Either output may be NULL; both NULL is refused, and so is a range outside [0, N].  env_count == 0 returns 0.  Rows are dense:
 * every element of a written row is written exactly once, nothing behind the last row.  One launch on the handle's stream: no copy,
 * no wait, no query, no allocation - legal inside a stream capture of the caller; the records are only read, and the launch is not
 * a step: no counter or statistic moves. */
#define CZ_EFFECT_MOVED 1
#define CZ_EFFECT_TURNED 2
#define CZ_EFFECT_HAND 4
#define CZ_EFFECT_OBJECTS 8
#define CZ_EFFECT_CELLS 16
int32_t cz_num_actions(cz_handle h);          /* 5 (scheme3) or 8 (scheme1); -1 for a null handle */
int cz_action_effects_device(cz_handle h, int64_t env_begin, int64_t env_count, uint32_t agents, uint32_t ignore,
                             uint8_t *d_mask, uint8_t *d_effects);

/* ---- frames ---------------------------------------------------------------------------------------- */
/* Frames of the current state (k_render; cooking_zoo_amd/render.py is the definition and the host model): the reference's
 * GraphicPipeline.render (environment/game/graphic_pipeline.py) as a display list per cell - (sprite, x0, y0, size) in draw order:
 * Counter and the cell's own sprite (a Deliversquare: a rect of Color.DELIVERY, then its sprite), the agents on the cell with
 * their orientation arrows, the cell's alive slots in slot order as Plate / food stack - composited per pixel with the project's
 * own rule: a draw of size s at (x0, y0) samples the M x M sprite at ((px - x0) * M / s, (py - y0) * M / s) in integers, and per
 * channel t = src * a + dst * (255 - a) + 128, dst = (t + (t >> 8)) >> 8 over a canvas that starts at Color.FLOOR.  P is the tile
 * size in pixels (the reference's PIXEL_PER_TILE = 80), 4 <= P <= 128; the geometry follows from P by the reference's own double
 * expressions.  d_rgb8 uint8 [env_count][H * P][W * P][3] and / or d_chw32 float [env_count][3][H * P][W * P] = v * (1.0f / 255.0f) (a table: torch's `x / 255` on the device);
 * every byte is written exactly once.  d_rgb8 must be 4-byte aligned and d_chw32 16-byte aligned.  `vis` bit a: agent a is drawn
 * as `robot`, otherwise as `human`.  env_count = 0 is a no-op.
 * Deviations from the reference: (1) Cucumber is drawn as `default_dynamic` without text (the reference's font.render() without
 * arguments raises there); (2) an agent whose despawn bit is set is not drawn (what it holds still is), and agent a always uses
 * `vis` bit a and colour a - the reference draws relevant_agents, which keeps a just-despawned agent one step longer, and indexes
 * agent_visualization by the position in that list; (3) the sprite is resampled from the M x M master, not from the original
 * file; (4) the blend rule is the project's: equality with pygame's blitter is unverified; (5) slots or agents whose coordinates
 * lie outside the grid are not drawn.
 * cz_load_sprites takes the sheet uint8 [cz_render_sprites()][M][M][4] RGBA from HOST memory, 1 <= M <= 128, uploads it once
 * together with the float table and replaces an earlier sheet; it allocates, copies and waits: NOT capturable.
 * cz_render_device is one launch on the handle's stream: no copy, wait or allocation, legal inside a stream capture; the records
 * are only read. */
int32_t cz_render_sprites(void);              /* the number of sprites of a sheet (cooking_zoo_amd/render.py SPRITES) */
int cz_load_sprites(cz_handle h, const uint8_t *rgba, int32_t n_sprites, int32_t M);
int cz_render_device(cz_handle h, int64_t env_begin, int64_t env_count, int32_t P, uint32_t vis, uint8_t *d_rgb8, float *d_chw32);

/* ---- step ------------------------------------------------------------------------------------------ */
/* One batched env step = accumulated_step (cooking_env.py:243-269): world_step (cooking_world.py:104-112),
 * compute_rewards (cooking_env.py:290-315), compute_truncated (:333-350), then observe (:271, :352-373).
 * An action < 0 marks an agent that is not in the list world_step acts on (despawned, cooking_world.py:105-108,267-290):
 * it does not turn, move, interact or take part in the collision filter, but keeps its cell.
 * Host-pointer form: actions int32 [N][A]; outputs obs float64 [N][A][F] (may be NULL), rewards float64 [N][A],
 * terminations / truncations uint8 [N][A].  Synchronous. */
int cz_step(cz_handle h, const int32_t *actions, double *obs, double *rewards, uint8_t *terminations,
            uint8_t *truncations);

/* Recipe-node marks (record word 1: bit 8r+j = node j of the env's r-th recipe is met, bit 8r = recipe r complete) of
 * every env after the most recent cz_step: what compute_infos reports as `recipe_done` (cooking_env.py:317-331).
 * uint32 [N][2]: record words 1 and 7 (the second is 0 unless the recipe tables are wide).  Fails if cz_step has not run
 * on this handle. */
int cz_last_marks(cz_handle h, uint32_t *marks);

/* Device-pointer form, asynchronous on the handle's stream (d_obs may be NULL: encode skipped). */
int cz_step_device(cz_handle h, const int32_t *d_actions, double *d_obs, double *d_rewards,
                   uint8_t *d_terminations, uint8_t *d_truncations);

/* The same step with a COMPACT observation for consumers that stay on the device: every feature of get_feature_vector
 * (cooking_env.py:352-373) is one of at most 256 values - quotients (x - ax) / W, (y - ay) / H, 0.0, 1.0 - so d_codes
 * (uint8 [N][A][cz_codes_pitch(h)], pitch = F rounded up to 16, padding bytes 255) receives for every feature the INDEX of its
 * value in a table of 256 float64 (cz_obs_table: a host copy; cz_obs_table_device: the resident one), i.e.
 * table[d_codes[e][a][f]] is bit for bit the float64 observation - 1/8 of the bytes, losslessly.  d_obs may be NULL (codes
 * only) or a float64 [N][A][F] buffer that is written as well. */
int cz_step_device_compact(cz_handle h, const int32_t *d_actions, uint8_t *d_codes, double *d_obs, double *d_rewards,
                           uint8_t *d_terminations, uint8_t *d_truncations);
/* ... or as a setting of the handle: from now on every one-step launch (cz_step_device, _many, _ring, cz_step) writes the compact
 * observation to d_codes as well - with d_obs = NULL in those calls, instead of the float64 rows; NULL switches it off. */
int cz_set_compact_output(cz_handle h, uint8_t *d_codes);
/* host-pointer form (synchronous, like cz_step) that returns the codes instead of the float64 rows: 1/8 of the bytes over PCIe */
int cz_step_compact(cz_handle h, const int32_t *actions, uint8_t *codes, double *rewards, uint8_t *terminations, uint8_t *truncations);
int32_t cz_codes_pitch(cz_handle h);
int cz_obs_table(cz_handle h, double table[256]);
const void *cz_obs_table_device(cz_handle h);

/* The same step with the observation of observe() / get_feature_vector (cooking_env.py:271,352-373) as FLOAT32 rows, the dtype a
 * policy network takes: d_obs32 float [N][A][F], dense (no pitch: a float32 tensor of that shape is contiguous), every element
 * (float) of the reference's float64 feature, rounded to nearest even - bit for bit np.float32(x), what torch's .float() gives.
 * The values are gathered from a second 256-entry table, the float64 one rounded once (cz_obs_table_f32 is its host mirror):
 * half the observation bytes of cz_step_device and no conversion pass behind it.  d_obs32 must not be NULL; rewards stay
 * float64.  Asynchronous on the handle's stream. */
int cz_step_device_f32(cz_handle h, const int32_t *d_actions, float *d_obs32, double *d_rewards, uint8_t *d_terminations,
                       uint8_t *d_truncations);
/* ... or as a setting of the handle (cooking_env.py:271,352-373 for every launch that follows): from now on every one-step
 * launch (cz_step_device, _many, _ring, cz_step) called with d_obs = NULL writes the float32 rows to d_obs32; NULL switches it
 * off.  Refused: setting it while a compact output is set (and the reverse), and a one-step call with d_obs != NULL while it is
 * set.  Ring graphs built before the call are dropped; fused ring runs (cz_set_ring_fused) are issued as one-step launches
 * while it is set.  The fused rollouts (cz_rollout*) ignore it: their float32 trajectory is a call of its own (cz_rollout_f32,
 * cz_rollout_actions_f32). */
int cz_set_f32_output(cz_handle h, float *d_obs32);
/* host mirror of the table those rows are gathered from (cooking_env.py:352-373: every feature is one of these values):
 * table[i] == (float)cz_obs_table[i], and d_obs32[e][a][f] == table[codes[e][a][f]] bit for bit. */
int cz_obs_table_f32(cz_handle h, float table[256]);

/* K consecutive steps, one launch each, issued from C: step k reads its actions at d_actions + (k % action_period) *
 * action_stride (in int32 elements) and overwrites the same output buffers.  Equivalent to K cz_step_device calls. */
int cz_step_device_many(cz_handle h, int32_t K, const int32_t *d_actions, int64_t action_stride, int32_t action_period,
                        double *d_obs, double *d_rewards, uint8_t *d_terminations, uint8_t *d_truncations);

/* The same for actions kept in a ring of `action_period` slots (slot s at d_ring + s * action_stride): step k reads slot
 * (first_slot + k) % action_period.  Runs of consecutive slots (cut where the ring wraps and at 256 launches; at least
 * 48 launches long - CZ_GRAPH_MIN_RUN) are captured into HIP graphs on first use, keyed by (first slot, length), and replayed
 * afterwards (no host work per launch, stable kernel-argument memory); shorter pieces are launched directly (a graph's first
 * kernel starts later than a plain launch's, which a short run cannot win back); identical results.
 * At most 64 graphs are kept per handle: keep the runs of a loop aligned to the same slots. */
int cz_step_device_ring(cz_handle h, int32_t K, const int32_t *d_ring, int64_t action_stride, int32_t action_period,
                        int32_t first_slot, double *d_obs, double *d_rewards, uint8_t *d_terminations, uint8_t *d_truncations);

/* Optional: build the graphs of one such call up front (nothing is stepped), e.g. before a timed region. */
int cz_ring_prepare(cz_handle h, int32_t K, const int32_t *d_ring, int64_t action_stride, int32_t action_period,
                    int32_t first_slot, double *d_obs, double *d_rewards, uint8_t *d_terminations, uint8_t *d_truncations);

/* FUSED RING RUNS (opt-in).  With cz_set_ring_fused(h, 1), a run of two or more steps of cz_step_device_ring / _many whose action
 * slots are densely packed (action_stride == num_envs * num_agents) goes out as ONE launch per stretch of consecutive slots
 * (cut where the ring wraps): cz_rollout_actions' kernel over the ring's own rows, the env state in registers across the
 * steps, every step's observation / rewards / flags written IN PLACE to the [N][A]... buffers of the call.  Afterwards state,
 * output buffers and statistics are bit for bit what K one-step launches leave (cooking_env.py:243-269 K times) - at the cost
 * per step of a fused rollout, without launch boundaries.  Open loop by nature (the actions
 * of the whole run are read by one launch).  Runs with other strides, a compact
 * output (cz_set_compact_output), a float32 output (cz_set_f32_output) or kernel timing switched on are issued as before.  Returns the previous setting, -1 for a
 * null handle; cz_ring_fused_steps: env steps issued this way so far (reset != 0: zero the count after reading). */
int cz_set_ring_fused(cz_handle h, int32_t enabled);
int64_t cz_ring_fused_steps(cz_handle h, int32_t reset);

/* SPLIT RUNS.  A run of one-step launches of cz_step_device_ring / _many can go out as two launch chains over the two halves of the
 * batch - envs [0, ceil(N / 2)) rounded up to whole workgroups, and the rest -, part 0 on the handle's stream and part 1 on a
 * second stream of the handle's, forked from and joined onto the handle's stream once per graph replay or directly launched piece:
 * one half computes while the other sits in its kernel boundary.  A replayed piece is two linear graphs, one per chain; the second
 * one starts behind a short fixed delay that keeps the chains out of phase.  Envs never interact, so state, outputs, statistics and
 * cz_launch_counts (which keeps counting steps) are bit for bit those of the unsplit run.  mode: -1 automatic (the default: the
 * replayed pieces of the batch sizes at which the split measured faster, DESIGN.md "Ring runs"; directly launched pieces stay
 * whole), 0 off, 2 two parts, replayed and directly launched pieces alike; CZ_RING_SPLIT in the environment of cz_create sets
 * the initial mode.  Never split, whatever the mode: a run inside a stream capture of the caller, with kernel timing on, as fused
 * launches (cz_set_ring_fused), of fewer than 2 envs, and any run of a process whose environment sets GPU_MAX_HW_QUEUES below 4
 * (the variable is only read).  Drops the ring graphs built so far.  Returns the previous mode, -2 on error.
 * cz_ring_split_parts: in how many chains (1 or 2) the replayed pieces of a run outside a capture go out as things stand. */
int cz_set_ring_split(cz_handle h, int32_t mode);
int32_t cz_ring_split_parts(cz_handle h);

/* How many step kernels cz_step_device_ring has replayed from graphs / launched directly on this handle so far
 * (reset != 0: zero both after reading).  bench.py describes its run from these numbers.  Fused ring runs (cz_set_ring_fused) are
 * not in either count: cz_ring_fused_steps has theirs. */
int cz_launch_counts(cz_handle h, int64_t *graph_kernels, int64_t *direct_kernels, int32_t reset);

/* T fused steps in one launch with on-device uniform random actions (counter-based stream keyed by
 * (seed, global env id, agent, step0 + t)); state stays in registers between steps.  d_obs, if not NULL,
 * is a trajectory buffer [T][N][A][F]; d_rewards [T][N][A]; d_term/d_trunc [T][N][A] (each may be NULL
 * to keep only device-side statistics).  Asynchronous. */
int cz_rollout(cz_handle h, int32_t T, uint64_t seed, uint32_t step0, double *d_obs, double *d_rewards,
               uint8_t *d_terminations, uint8_t *d_truncations);

/* ... with the trajectory as compact observations: d_codes uint8 [T][N][A][cz_codes_pitch(h)] (cz_step_device_compact explains the
 * codes); d_obs (float64 [T][N][A][F]) may be NULL - codes only - or is written as well. */
int cz_rollout_compact(cz_handle h, int32_t T, uint64_t seed, uint32_t step0, uint8_t *d_codes, double *d_obs, double *d_rewards,
                       uint8_t *d_terminations, uint8_t *d_truncations);

/* The same fused launch over actions of the caller (replay, open-loop search): d_actions int32 [T][N][A], step t reads row t
 * (values as for cz_step_device: action & 7, negative = the agent does not act).  Same results as T cz_step_device launches
 * over those rows, with every step's outputs in the trajectory buffers. */
int cz_rollout_actions(cz_handle h, int32_t T, const int32_t *d_actions, double *d_obs, double *d_rewards,
                       uint8_t *d_terminations, uint8_t *d_truncations);

/* cz_rollout with the trajectory as FLOAT32 rows (cooking_env.py:243-269 T times, each step's observation - :271,352-373 - in the
 * dtype a policy network takes): d_obs32 float [T][N][A][F], dense, every element (float) of the reference's float64 feature as in
 * cz_step_device_f32 - half the bytes of the float64 trajectory, written once, no conversion or gather pass behind the launch.
 * d_obs32 must not be NULL (without a trajectory: cz_rollout with d_obs = NULL).  Rewards stay float64; d_rewards and the flags
 * [T][N][A] may each be NULL.  State, statistics, rewards and flags afterwards are bit for bit what cz_rollout leaves from the same
 * start.  A pure launch on the handle's stream (legal inside a capture of the caller); ignores cz_set_compact_output /
 * cz_set_f32_output like every rollout.  Same limit on T as cz_rollout (T * num_envs * num_agents * 8 below 4 GiB). */
int cz_rollout_f32(cz_handle h, int32_t T, uint64_t seed, uint32_t step0, float *d_obs32, double *d_rewards,
                   uint8_t *d_terminations, uint8_t *d_truncations);
/* ... and cz_rollout_actions likewise (cooking_env.py:243-269 T times over the caller's actions, :352-373): d_actions int32
 * [T][N][A], step t reads row t and writes row t of d_obs32 float [T][N][A][F].  The same rows, rewards, flags, state and statistics
 * as T cz_step_device_f32 launches over those action rows. */
int cz_rollout_actions_f32(cz_handle h, int32_t T, const int32_t *d_actions, float *d_obs32, double *d_rewards,
                           uint8_t *d_terminations, uint8_t *d_truncations);

/* ---- The MLP policy the library evaluates itself (definition and numpy model: cooking_zoo_amd/policy.py).
 * A weight set is the parameters of Sequential(Linear(F, 64), ReLU(), Linear(64, C)) in torch's own layout: W1 float32 [64][F],
 * b1 [64], W2 [C][64], b2 [C]; F the handle's row length, C = cz_num_actions(h), hidden width 64; up to 4 sets per handle.  For a
 * float32 row x: acc_j = b1[j], then acc_j = fmaf(W1[j][f], x[f], acc_j) for f ascending; h_j = acc_j > 0 ? acc_j : 0; per action
 * p_j = W2[c][j] * h_j, six butterfly levels p_j += p_(j xor 2^k) in float32, logit_c = p + b2[c].  CZ_POLICY_GREEDY: the smallest c
 * with the largest logit.  CZ_POLICY_SAMPLE, in float64, every operation rounded on its own: z_c = logit_c - max,
 * e_c = cz_exp(max(z_c, -64)), running sums S_c, thr = u * S_(C-1), the smallest c with S_c > thr, else C - 1;
 * u = cz_spawn_uniform(seed, global env id, 0, step, 0x300 + agent, 0).  numpy reproduces all of it bit for bit; NaN, infinities and
 * subnormal intermediates are NOT pinned.
 *
 * cz_load_policy_device: n_sets (1..4) sets from DEVICE memory, sets contiguous in the layouts above; one repack launch on the
 * handle's stream.  The handle's first call allocates the table (room for 4 sets), no later call allocates: those are legal inside a
 * stream capture, so a learner reloads after every optimiser step with no host trip.  F and C are fixed by cz_create: neither
 * cz_load_layouts nor cz_load_recipes drops the table.  Refused: n_sets outside 1..4, a NULL pointer. */
#define CZ_POLICY_GREEDY 0
#define CZ_POLICY_SAMPLE 1
int cz_load_policy_device(cz_handle h, int32_t n_sets, const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2);
int32_t cz_policy_sets(cz_handle h);           /* sets the last load filled; 0: none */
/* The policy on rows of the caller, one launch (k_policy): d_obs32 float32 [env_count][A][F] -> d_actions int32 [env_count][A] and /
 * or d_logits float32 [env_count][A][C].  `sets`: agent a's set index in byte a, 0xFF = none - that agent's entries are left
 * untouched in both outputs (cz_partner_device's convention: a partner's and a learner's actions can share one array).  `step` keys
 * the draw of CZ_POLICY_SAMPLE.  Stream-ordered: no copy, no wait, no allocation - legal inside a stream capture of the caller; no
 * record is read.  Refused: a set index >= the loaded count, no table loaded, both outputs NULL, a range outside the batch. */
int cz_policy_device(cz_handle h, int64_t env_begin, int64_t env_count, const float *d_obs32, uint32_t sets, int32_t mode,
                     uint64_t seed, uint32_t step, int32_t *d_actions, float *d_logits);
/* cz_rollout_f32 (cooking_env.py:243-269 T times, :352-373) with the policy in front of every fused step, T policy-driven steps in one
 * launch (k_step<..., ROLLOUT_POLICY>): agent a's action at fused step t is the policy's on the env's float32 row before that step -
 * t = 0: what cz_observe_device_f32 would write at launch; t > 0: row t - 1 of the trajectory, whatever it is, the row of a reset
 * pass included - with the draw keyed by step = step0 + t.  Agents whose byte of `sets` is 0xFF play cz_rollout's own stream,
 * cz_action(seed, env, a, step0 + t, C).  d_obs32 float32 [T][N][A][F] is required; d_actions int32 [T][N][A] (every agent's action
 * as played, stream agents included) and d_logits float32 [T][N][A][C] (policy agents only, the rest untouched) may be NULL; rewards,
 * flags, state, statistics and episode records are cz_rollout_actions_f32's over the same actions.  The rows are staged in LDS next
 * to their stores (A * 4 * ceil(F / 4) * 4 bytes per env): a handle whose rows do not fit a workgroup's LDS is refused.  Refused
 * besides: what cz_rollout_f32 refuses, every agent at 0xFF, a set index >= the loaded count, no table loaded. */
int cz_rollout_policy(cz_handle h, int32_t T, uint32_t sets, int32_t mode, uint64_t seed, uint32_t step0, float *d_obs32,
                      int32_t *d_actions, float *d_logits, double *d_rewards, uint8_t *d_terminations, uint8_t *d_truncations);

/* ---- The critic (policy.py, step 3b).  A weight set may carry a value head, Linear(64, 1) in torch's layout: wv float32 [64]
 * (weight[0]) and bv [1].  With h_j of the set's hidden layer: p_j = wv[j] * h_j, the same six butterfly levels, value = p + bv -
 * the arithmetic of one logit, which policy.host_value reproduces bit for bit.  Every call below takes `vsets`, agent a's byte: the
 * weight set whose W1, b1 and value head give agent a's value, 0xFF = none (entries untouched).  It is independent of `sets`: a
 * shared trunk is vsets == sets, a separate critic is another weight set whose action head is never used.  Equal bytes: one hidden
 * pass; different bytes: a second one; the bits are the same either way.  A byte >= min(cz_policy_sets, cz_value_sets) is refused.
 *
 * cz_load_value_device: the value heads of sets 0 .. n_sets-1 from DEVICE memory, d_wv [n][64] and d_bv [n][1]; one repack launch on
 * the handle's stream, legal inside a stream capture.  The heads live in the policy table's allocation: refused before the first
 * cz_load_policy_device.  Refused besides: n_sets outside 1..4, a NULL pointer. */
int cz_load_value_device(cz_handle h, int32_t n_sets, const float *d_wv, const float *d_bv);
int32_t cz_value_sets(cz_handle h);            /* sets whose value head the last load filled; 0: none */
/* The value alone on rows of the caller, one launch (k_value): d_obs32 float32 [rows][A][F] -> d_values float32 [rows][A].  `rows`
 * counts [A][F]-rows as in cz_logprob_device and is not tied to the batch: a whole [T + 1] * N trajectory is one launch.  Stream-
 * ordered and capturable; no record is read.  Refused: rows < 1, a NULL pointer, every agent at 0xFF, a byte past the loaded heads. */
int cz_value_device(cz_handle h, int64_t rows, const float *d_obs32, uint32_t vsets, float *d_values);
/* cz_rollout_policy plus d_values float32 [T + 1][N][A], required (k_step<..., ROLLOUT_POLICY_VALUE>).  Row t is the value on exactly
 * the row the policy reads in front of fused step t; row T is the value on the row staged by step T - 1 - the row a following
 * launch's step 0 would read - so d_values goes into cz_gae_device as it is.  Everything else is bit for bit what cz_rollout_policy
 * leaves for the same arguments.  Unlike cz_rollout_policy, every agent may be at 0xFF in `sets` as long as one has a `vsets` byte:
 * values under the action stream.  Refused: what cz_rollout_policy refuses otherwise, a NULL d_values, every agent at 0xFF in both
 * words. */
int cz_rollout_policy_value(cz_handle h, int32_t T, uint32_t sets, uint32_t vsets, int32_t mode, uint64_t seed, uint32_t step0,
                            float *d_obs32, int32_t *d_actions, float *d_logits, float *d_values, double *d_rewards,
                            uint8_t *d_terminations, uint8_t *d_truncations);

/* ---- What an on-policy learner trains on, from the trajectory cz_rollout_policy leaves in device memory (definition and numpy
 * model: cooking_zoo_amd/targets.py).  Float64 throughout, every operation rounded on its own, outputs rounded to float32 once; numpy
 * reproduces both calls bit for bit; NaN, infinities and subnormal intermediates are NOT pinned.  Both are one launch on the handle's
 * stream over dense arrays of the caller - no copy, no wait, no allocation, legal inside a stream capture of the caller; no record is
 * read.  The extents are the caller's own and not tied to the handle's batch: a shard or a slice passes its own.
 *
 * cz_gae_device: generalised advantage estimation.  d_rewards float64 [T][env_count][A], d_terminations / d_truncations uint8
 * [T][env_count][A] (d_truncations may be NULL), d_values float32 [T + 1][env_count][A]: row t the critic on the state BEFORE step t,
 * row T the bootstrap.  Per series, gl = gamma * lambda, A = 0, for t = T - 1 down to 0: done = term[t] || trunc[t];
 * d = (r[t] + (done ? 0 : gamma * V[t + 1])) - V[t]; A = d + (done ? 0 : gl * A); adv[t] = (float)A; ret[t] = (float)(A + V[t]).  The
 * serial order is the definition.  Done is terminal for truncations too: under auto-reset the row behind a finished episode is the
 * next episode's first observation.  `agents`: bit a = agent a's series are computed, the others neither read nor written.  One of
 * d_advantages / d_returns may be NULL.  Refused: T < 1, env_count < 1, NULL rewards / terminations / values, both outputs NULL,
 * `agents` without an agent below A, gamma or lambda outside [0, 1] or NaN. */
int cz_gae_device(cz_handle h, int32_t T, int64_t env_count, const double *d_rewards, const uint8_t *d_terminations,
                  const uint8_t *d_truncations, const float *d_values, double gamma, double lambda, uint32_t agents,
                  float *d_advantages, float *d_returns);
/* cz_logprob_device: the log-probability of the action played and the entropy of the distribution CZ_POLICY_SAMPLE draws from, from
 * its own z_c = logit_c - max, e_c = cz_exp(max(z_c, -64)) and running sum S: logp = (float)(z_a - cz_log(S)); q_c = z_c - cz_log(S),
 * p_c = cz_exp(max(q_c, -64)), entropy = (float)(-(p_0 q_0 + p_1 q_1 + ...)) in ascending c.  cz_log on [1, 8]: k = (S >= 2) + (S >= 4)
 * + (S >= 8), m = S * 2^-k, y = k ln2 + (m - 1) ln2, five steps y = y + (S * cz_exp(max(-y, -64)) - 1); no division; cz_log(1) = 0.
 * d_logits float32 [rows][A][C], d_actions int32 [rows][A] -> d_logp and / or d_entropy float32 [rows][A]; `rows` counts [A]-rows: T * N
 * for a trajectory, n for cz_policy_device's output.  An action outside 0 .. C-1 gets logp 0.0 (its entropy is written).  Agents whose
 * byte of `sets` is 0xFF are left untouched in both outputs (their logits were never written).  Refused: rows < 1, NULL logits or
 * actions, both outputs NULL, every agent below A at 0xFF. */
int cz_logprob_device(cz_handle h, int64_t rows, const float *d_logits, const int32_t *d_actions, uint32_t sets,
                      float *d_logp, float *d_entropy);

/* ---- PPO's update phase: the clipped-surrogate loss with value and entropy terms, differentiated by the library over the weight sets
 * it plays with, in the rollout's own arithmetic (definition and numpy model: cooking_zoo_amd/ppo.py, which numpy reproduces bit for
 * bit; zeros compare equal whatever their sign; NaN, infinities and subnormal intermediates are NOT pinned).  The forward is
 * cz_rollout_policy_value's and the softmax cz_logprob_device's, so on the weights that played ratio == 1.0 exactly.
 *
 * cz_ppo_reserve: the workspace for minibatches of up to max_positions positions over the sets loaded now - per (position, agent)
 * two pass slots and the statistics' terms, per (chunk of cz_ppo_chunk() positions, loaded set) one partial gradient.  It allocates,
 * so call it outside a stream capture; a call that asks for no more than is reserved does nothing.  Refused: no table loaded,
 * max_positions < 1 or past 2^30 / A, an allocation inside a capture.  cz_ppo_reserved: the positions reserved (0: none). */
int cz_ppo_reserve(cz_handle h, int64_t max_positions);
int64_t cz_ppo_reserved(cz_handle h);
int32_t cz_ppo_chunk(void);                    /* 64: the reduction order of ppo.py is in chunks of this many positions */
/* cz_ppo_grad_device: d_obs32 float32 [rows][A][F], d_actions int32 [rows][A], d_logp_old / d_adv / d_ret float32 [rows][A] - a
 * trajectory flattened to rows = T * N.  d_index int32 [positions] is the minibatch, position m uses row d_index[m] (rows may repeat;
 * an index outside 0 .. rows-1 contributes nothing and is counted in d_stats[7]); NULL means positions == rows and row m.  `sets` /
 * `vsets`: agent a's policy and value set in byte a, 0xFF = none, as in cz_rollout_policy_value.  Per (position, agent): the policy
 * part if the agent has a set and its action is inside 0 .. C-1 - ratio = cz_exp((float)q_act - logp_old), q_act rounded to the float32 cz_logprob_device writes, clipped where it left [1 - clip,
 * 1 + clip] on the advantage's side - and the value part c_value * 0.5 * (v - ret)^2; both averaged over positions and agents with a
 * set; the entropy bonus c_entropy * H.  Advantage normalisation is the caller's.  The gradients come in torch.nn.Linear's layouts
 * behind a leading axis of cz_policy_sets(h) - the stacking the two loads take, so a stacked parameter's .grad can be the buffer:
 * d_gw1 [n][64][F], d_gb1 [n][64], d_gw2 [n][C][64], d_gb2 [n][C], d_gwv [n][64], d_gbv [n][1] (the last two may be NULL when every
 * byte of `vsets` is 0xFF); sets no agent uses get zeros.  The sums run in float32 fmaf chains in a fixed order, chunk by chunk
 * (ppo.py): independent of grid shape and device.  d_stats float64 [8] (may be NULL): surrogate loss, value loss, entropy, the
 * plain KL estimate, clipped fraction, policy parts, value parts, indices out of range.  Three launches on the handle's stream - no
 * copy, no wait, no allocation, legal inside a stream capture of the caller; no record is read.  Refused: no table loaded, a set
 * past the loaded ones, every agent at 0xFF in both words, positions < 1 or past the reserved ones, rows < 1, d_index == NULL with
 * positions != rows, a NULL required pointer, clip / c_value / c_entropy negative or NaN, more sets loaded than were reserved for. */
int cz_ppo_grad_device(cz_handle h, int64_t rows, int64_t positions, const int32_t *d_index /* may be NULL */,
                       const float *d_obs32, const int32_t *d_actions, const float *d_logp_old, const float *d_adv, const float *d_ret,
                       uint32_t sets, uint32_t vsets, double clip, double c_value, double c_entropy,
                       float *d_gw1, float *d_gb1, float *d_gw2, float *d_gb2, float *d_gwv, float *d_gbv, double *d_stats);

/* ---- The optimiser: global-norm gradient clipping and Adam / AdamW on the caller's arrays, in a pinned float64 arithmetic that numpy
 * reproduces bit for bit (definition and numpy models: cooking_zoo_amd/adam.py; zeros compare equal whatever their sign; NaN and
 * subnormal intermediates are NOT pinned).  The library keeps no optimiser state: parameters, gradients, first and second moments are
 * four groups of six float32 tensors in torch.nn.Linear's layouts behind a leading axis of cz_policy_sets(h) - w1 [n][64][F], b1 [n][64],
 * w2 [n][C][64], b2 [n][C], wv [n][64], bv [n][1], what cz_ppo_grad_device writes and the two loads take - and d_state is float64 [8] in
 * device memory: steps taken, the running products of the beta1 and beta2 values used, the last call's gradient norm and clip
 * coefficient, calls skipped, the learning rate last used, one word never written; a fresh state is {0, 1, 1, 0, 0, 0, 0, 0}.
 *
 * cz_adam_reserve: one float64 per chunk of cz_adam_chunk() gradient elements for four sets.  It allocates, so call it outside a
 * stream capture; every later call does nothing.
 * cz_adam_step_device: bit k of set_mask set means set k takes part; every array of another set is neither read nor written.  The
 * squared norm of the masked gradients is summed in a fixed order (chunks of 1024, a butterfly within a chunk, one serial chain over
 * the chunks: adam.py), independent of grid shape and device.  A total that is not finite skips the call: parameters, moments and
 * table stay byte for byte, word 4 of the state becomes 0.0 and word 5 counts it.  Otherwise coef = max_norm == 0 ? 1 : min(1,
 * max_norm / (norm + 1e-6)), the moments advance on coef * g, bias correction uses the running products, weight_decay != 0 decays
 * the parameter by lr * weight_decay first (decoupled, AdamW), and the parameter moves by lr * mh / (sqrt(vh) + eps).  lr is *d_lr where
 * d_lr is given (device memory: a schedule inside a captured graph), the by-value argument otherwise.  The moments are stored as
 * float32 and read back as stored, so a run restarted from saved buffers continues bit for bit.  Unless CZ_ADAM_KEEP_TABLE is set,
 * the masked sets of the weight table - and their value heads, when the value tensors are given - become the new parameters in the
 * same launch, byte for byte what cz_load_policy_device / cz_load_value_device of the updated arrays would leave: no reload follows.
 * The four structs are host memory, read during the call; wv and bv are given in all four or in none.  Three launches on the
 * handle's stream - no copy, no wait, no allocation, legal inside a stream capture of the caller.  Refused: no table loaded, no
 * cz_adam_reserve, set_mask empty or with a bit at or past cz_policy_sets, value tensors with a masked set at or past cz_value_sets
 * (unless CZ_ADAM_KEEP_TABLE), value pointers present in some groups only, any other NULL pointer, lr / weight_decay / max_norm
 * negative or NaN, a beta outside [0, 1) or NaN, eps <= 0 or NaN, unknown flag bits. */
typedef struct cz_params { float *w1, *b1, *w2, *b2, *wv, *bv; } cz_params;   /* cz_sizeof_params() */
#define CZ_ADAM_KEEP_TABLE 1u
int32_t cz_sizeof_params(void);
int32_t cz_adam_chunk(void);                   /* 1024: the norm's summation order of adam.py is in chunks of this many elements */
int cz_adam_reserve(cz_handle h);
int cz_adam_step_device(cz_handle h, uint32_t set_mask, const cz_params *params, const cz_params *grads,
                        const cz_params *exp_avg, const cz_params *exp_avg_sq, double *d_state,
                        double lr, const double *d_lr /* may be NULL */, double beta1, double beta2, double eps,
                        double weight_decay, double max_norm, uint32_t flags);

/* the action the on-device stream draws (host mirror, for parity tests) */
uint32_t cz_action(uint64_t seed, int64_t env_global, int32_t agent, uint32_t step, uint32_t n_actions);
/* the layout an env draws for its k-th episode under auto_reset */
uint32_t cz_next_layout(int64_t env_global, uint32_t episode, uint32_t pool_word, uint32_t n_layouts);
/* ... when the envs draw from part `active` of `groups` (cz_set_layout_group) */
uint32_t cz_next_layout_group(int64_t env_global, uint32_t episode, uint32_t pool_word, uint32_t n_layouts, uint32_t groups,
                              uint32_t active);

/* ---- device memory + timing helpers (so the Python host needs no torch) ----------------------------- */
void *cz_dev_alloc(cz_handle h, size_t bytes);
int cz_dev_free(cz_handle h, void *d_ptr);
/* pinned host memory: host buffers taken from here (actions / observations / rewards / flags of cz_step, cz_reset,
 * cz_observe) are written and read by the copy engines directly -- no per-call pinning or staging of pageable pages */
void *cz_host_alloc(cz_handle h, size_t bytes);
int cz_host_free(cz_handle h, void *ptr);
int cz_memcpy_h2d(cz_handle h, void *d_dst, const void *src, size_t bytes);
int cz_memcpy_d2h(cz_handle h, void *dst, const void *d_src, size_t bytes);
int cz_timer_start(cz_handle h);                           /* hipEventRecord on the handle's stream */
int cz_timer_stop(cz_handle h, float *elapsed_ms);         /* record + synchronize + elapsed        */
/* brackets every kernel launch of the step path with HIP events and accumulates device time */
int cz_kernel_time_reset(cz_handle h, int32_t enable);
int cz_kernel_time_read(cz_handle h, double *total_ms, int64_t *launches);
/* measurement aid: average duration of `reps` back-to-back launches of a kernel of the step kernel's grid shape that does
 * nothing but write `bytes` (<= 2 GiB) to d_dst with the encode's 16-byte write-through stores -- the floor of a launch
 * that has to emit that much output (bench.py reports it next to the roofline).  d_dst is overwritten. */
int cz_probe_output_only(cz_handle h, void *d_dst, size_t bytes, int32_t reps, float *us_per_launch);
/* measurement aid: a CLOSED loop - K times (cz_step_device, then a tiny policy kernel that derives every agent's next action
 * from the observation it was just given, same stream), one HIP graph, replayed `reps` times; average microseconds per
 * step (step + policy).  d_actions (int32 [N][A]) is read and rewritten in place; K <= 1024. */
int cz_probe_closed_loop(cz_handle h, int32_t K, int32_t reps, int32_t *d_actions, double *d_obs, double *d_rewards,
                         uint8_t *d_terminations, uint8_t *d_truncations, float *us_per_step);
/* ... the same loop over the compact observation: cz_step_device_compact (codes only), then a policy kernel that reads the same
 * four features as table indices - it takes the same actions as cz_probe_closed_loop's. */
int cz_probe_closed_loop_compact(cz_handle h, int32_t K, int32_t reps, int32_t *d_actions, uint8_t *d_codes, double *d_rewards,
                                 uint8_t *d_terminations, uint8_t *d_truncations, float *us_per_step);
/* test / measurement aid: one launch, on the handle's stream, of the stand-in policy those loops use - d_actions[env][agent] = a
 * hash of four features of the observation in d_obs (float64 rows) or, with d_obs NULL, in d_codes (compact rows; the same
 * actions).  tests/test_gpu_capture.py captures [cz_probe_policy, cz_step_device] into a graph of the caller with it. */
int cz_probe_policy(cz_handle h, const double *d_obs, const uint8_t *d_codes, int32_t *d_actions);

/* ---- statistics + multi-GPU ------------------------------------------------------------------------- */
int cz_get_stats(cz_handle h, cz_stats *out);              /* device reduction over this handle's envs */
int cz_reset_stats(cz_handle h);                           /* ... and forgets the episodes no cz_episodes_collect has reported yet */
/* Which envs finished an episode since the last collect, with what return per agent, after how many steps, and how it ended: the
 * `episode` / `_episode` entries of the reference's `infos` (cooking_env.py:248,264,329) for the whole batch, resident on the device.
 * The wave that ends an episode keeps the env's last finished episode - every kernel, every mode, always; an episode cut short by
 * cz_reset / cz_reset_device leaves nothing - and this call reports every env whose episode counter moved since the previous call:
 *   d_mask   uint8  [N]     1 where an episode finished since the last collect, else 0 - every byte is written;
 *   d_return double [N][A]  the return of every agent, the float64 sum of its rewards in step order, bit for bit;
 *   d_length int32  [N]     world steps of the episode;
 *   d_flags  uint32 [N]     cz_episode::flags.            Rows of envs with mask 0 stay untouched in these three;
 *   d_list   cz_episode [capacity]  the same set packed in ascending env order (a function of the state alone: ballots and prefix
 *            counts, no atomic append); entries whose rank is >= capacity are dropped from the list only;
 *   d_count  int32  [1]     the number of envs found, also when it exceeds capacity.
 * Every pointer is a device pointer and may be NULL; every env found is marked seen whatever the capacity is, so a call with all
 * outputs NULL just marks.  An env that finished several episodes in between (a fused rollout) reports the last one and says how many
 * in `finished`.  One or two kernel launches on the handle's stream: no copy, no query, no wait - legal inside a stream capture. */
int cz_episodes_collect(cz_handle h, uint8_t *d_mask, double *d_return, int32_t *d_length, uint32_t *d_flags,
                        cz_episode *d_list, int32_t capacity, int32_t *d_count);
/* RCCL over xGMI: the only collective of the path is an all-gather of one cz_stats per rank. */
int cz_comm_unique_id(uint8_t id[128]);
int cz_comm_init(cz_handle h, int32_t n_ranks, int32_t rank, const uint8_t id[128]);
int cz_stats_allgather(cz_handle h, cz_stats *out /* [n_ranks] */);
/* barrier over the communicator (a 4-byte all-reduce on the handle's stream + stream synchronisation) */
int cz_comm_barrier(cz_handle h);
/* diagnostics: the files that serve this process -- the RCCL library the communicator binds (a copy already loaded in
 * the process wins) and the HIP runtime this library runs on; each buffer holds `cap` bytes, either may be NULL */
int cz_runtime_paths(char *rccl_path, char *hip_path, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* COOKINGZOO_H */
