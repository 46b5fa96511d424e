"""CookingVecEnv: N independent CookingZoo worlds advanced by one HIP grid launch per step.

This is the batched form of the reference's `CookingEnvironment` (environment/cooking_env.py:49-385):
same kwargs (level, meta_file, num_agents, max_steps, recipes, end_condition_all_dishes, action_scheme,
reward_scheme), plus the batch geometry.  All world state lives in HBM behind the C-ABI of
include/cookingzoo.h; this class only prepares tables (layout pool, recipe tables) and moves arrays.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import random as _random

import numpy as np

from cooking_zoo_amd import _native, effects as _effects, grid as _grid, nav as _nav, partner as _partner, policy as _policy, render as _render, rotation as _rotation, soa, tasks as _tasks
from cooking_zoo_amd.cooking_book import recipe_drawer
from cooking_zoo_amd.cooking_world.actions import ACTION_SCHEMES
from cooking_zoo_amd.cooking_world.engine import load_level as _ll
from cooking_zoo_amd.cooking_world.layout import feature_length

DEFAULT_REWARD_SCHEME = {"recipe_reward": 20, "max_time_penalty": -5, "recipe_penalty": -40, "recipe_node_reward": 0}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class DeviceBuffer:
    """A typed HBM allocation owned by a CookingVecEnv (no torch involved)."""

    def __init__(self, env, shape, dtype):
        self.env, self.shape, self.dtype = env, tuple(int(s) for s in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = _native.lib().cz_dev_alloc(env._h, self.nbytes)
        if not self.ptr:
            _native.check(env._h, 1)

    def to_host(self, out=None):
        out = np.empty(self.shape, self.dtype) if out is None else out
        _native.check(self.env._h, _native.lib().cz_memcpy_d2h(self.env._h, _ptr(out), self.ptr, self.nbytes))
        return out

    def from_host(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.nbytes == self.nbytes
        _native.check(self.env._h, _native.lib().cz_memcpy_h2d(self.env._h, self.ptr, _ptr(arr), self.nbytes))

    def free(self):
        if self.ptr:
            _native.lib().cz_dev_free(self.env._h, self.ptr)
            self.ptr = None


def _dev_ptr(b):
    """device address of a DeviceBuffer / raw int / object with data_ptr() (e.g. a torch tensor); None stays None"""
    if b is None:
        return None
    if hasattr(b, "ptr"):
        return b.ptr
    if hasattr(b, "data_ptr"):
        if hasattr(b, "is_contiguous") and not b.is_contiguous():
            raise ValueError("device buffers must be contiguous")
        return C.c_void_p(b.data_ptr())
    return C.c_void_p(int(b))


def _address(b):
    """`_dev_ptr` as a plain integer (None stays None): what a pointer field of a ctypes structure takes"""
    q = _dev_ptr(b)
    return q.value if isinstance(q, C.c_void_p) else q


def resolve_recipe_tables(recipes):
    """-> (registry dict, names list).  Same rule as cooking_env.py:100-105: a non-empty user
    RECIPE_STORE replaces the default book."""
    book = recipe_drawer.RECIPE_STORE if recipe_drawer.RECIPE_STORE else recipe_drawer.RECIPES
    return book, list(book.keys())


class SpawnView:
    """Read-only view of the device's despawn / respawn bookkeeping (record word W_STATUS, cz_set_spawn): `active` [N, A],
    `grace` [N, A] as of the last `refresh()` (every host-array `step` / `reset` refreshes), `changed` [N, A] = whose
    presence flipped between the last two refreshes of a running episode (cooking_world.py status_changed)."""

    def __init__(self, env):
        self._env = env
        self.active = np.ones((env.num_envs, env.num_agents), dtype=bool)
        self.grace = np.full((env.num_envs, env.num_agents), env._spawn_cfg[2], dtype=np.int64)
        self.changed = np.zeros((env.num_envs, env.num_agents), dtype=bool)
        self._episode = None

    def refresh(self, reset=False):
        from cooking_zoo_amd.spawn import decode_status, grace_bits
        recs = self._env.get_state()
        active, grace = decode_status(recs[:, soa.W_STATUS], self._env.num_agents, grace_bits(self._env._spawn_cfg[2], self._env.num_agents))
        episode = recs[:, soa.W_EPISODE].copy()
        same = (not reset) and self._episode is not None
        self.changed = (active != self.active) & (episode == self._episode)[:, None] if same else np.zeros_like(active)
        self.active, self.grace, self._episode = active, grace, episode
        return self

    def relevant(self):
        """[N, A] bool: the agents a step reports on (active, or despawned in this very step): cooking_world.py:292-293"""
        return self.active | self.changed


class BatchTables:
    """Everything of a batch that is prepared on the host and never touches the device: meta file, levels, recipe tables and
    per-env recipe ids, the layout pool (one contiguous slice per level), dims, per-env level, spawn areas.  A `CookingVecEnv`
    is one of these plus a device handle; `ShardedVecEnv` makes one for the whole batch and hands every device a `shard` of
    it (same pool and tables, a contiguous range of global env ids), so that nothing is drawn or parsed twice."""

    def __init__(self, num_envs, level, meta_file, num_agents, max_steps, recipes, end_condition_all_dishes=False,
                 action_scheme="scheme1", reward_scheme=None, *, num_layouts=256, layout_seed=0, layouts=None,
                 env_id_base=0, max_dyn=None, agent_respawn_rate=0.0, grace_period=20, agent_despawn_rate=0.0, spawn_seed=0):
        self._spawn_cfg = (float(agent_despawn_rate), float(agent_respawn_rate), int(grace_period), int(spawn_seed))
        if action_scheme not in ACTION_SCHEMES:
            raise ValueError("action_scheme must be 'scheme1' or 'scheme3' (scheme2 raises AttributeError in the "
                             "reference: action_scheme2.py:15)")
        self.num_envs, self.num_agents, self.max_steps = int(num_envs), int(num_agents), int(max_steps)
        self.env_id_base = int(env_id_base)
        self.action_scheme = action_scheme
        self.scheme_class = ACTION_SCHEMES[action_scheme]
        self.n_actions = len(self.scheme_class.ACTIONS)
        self.meta = _ll.load_meta_file(meta_file)
        assert self.num_agents <= self.meta["Agent"], "Too many agents for this level"      # cooking_env.py:93
        self.levels = [level] if isinstance(level, str) else list(level)
        self.level_objects = [_ll.load_level_file(l) for l in self.levels]
        self.reward_scheme = dict(reward_scheme or DEFAULT_REWARD_SCHEME)
        self.end_condition_all_dishes = bool(end_condition_all_dishes)
        self.F = feature_length(self.meta)

        # ---- recipe tables
        self.book, self.book_names = resolve_recipe_tables(recipes)
        graphs = [self.book[n]() for n in self.book_names]
        # compact tables while every graph of the book has at most 8 nodes, wide ones (16) otherwise
        self.recipe_nodes = soa.NARROW_NODES if max(len(g.node_list) for g in graphs) <= soa.NARROW_NODES else soa.MAX_NODES
        self.recipe_table = np.stack([g.flatten(self.recipe_nodes) for g in graphs])
        self.recipe_graphs = graphs                                      # the book as it stood when the tables were made
        self.partner_rows = _partner.partner_rows(graphs)               # the scripted partner's view of the same graphs
        self.num_goals = _tasks.current_num_goals()                     # cooking_env.py:100-105
        # the goal id of every node (infos_device).  A registry with more than 255 goals (the reference's id counter is process-global
        # and never goes back: every registered recipe takes fresh ids) has none: a goal id no longer fits the table's byte, so
        # `infos_device` is refused there (cz_num_goals: -1; `num_goals` stays the reference's number) and everything else works.
        # A node id outside [0, num_goals) is a malformed book and raises here, as the reference does when the Recipe is made.
        self.goal_table = _tasks.goal_table(graphs, self.num_goals) if self.num_goals <= _tasks.MAX_GOALS else None
        if isinstance(recipes, np.ndarray):
            rid = np.asarray(recipes, dtype=np.int64)
            assert rid.shape[0] == self.num_envs
            self.recipe_names = None
        else:
            self.recipe_names = list(recipes)
            rid = np.tile(np.array([self.book_names.index(r) for r in recipes], dtype=np.int64), (self.num_envs, 1))
        self.num_recipes = rid.shape[1]
        if not (self.num_agents <= self.num_recipes <= soa.MAX_RECIPES_PER_ENV):
            raise ValueError("need one recipe per agent and at most 4 recipes (cooking_env.py:329)")
        self.recipe_ids = np.full((self.num_envs, 4), 0xFF, dtype=np.uint8)
        self.recipe_ids[:, :self.num_recipes] = rid

        # ---- layout pool (per level a contiguous slice)
        self.layout_seed = int(layout_seed)
        rng = _random.Random(layout_seed)
        self.layouts = []
        self.pool_slices = []
        for li, lv in enumerate(self.level_objects):
            base = len(self.layouts)
            if layouts is not None:
                mine = layouts[li] if isinstance(layouts[0], (list, tuple)) else layouts
            else:
                mine = [_ll.instantiate(lv, self.meta, self.num_agents, rng) for _ in range(int(num_layouts))]
            self.layouts += list(mine)
            self.pool_slices.append((base, len(mine)))
        W, H = self.layouts[0].width, self.layouts[0].height
        if any((l.width, l.height) != (W, H) for l in self.layouts):
            raise ValueError("all levels of one batch must share the grid size")
        D = max_dyn if max_dyn is not None else max(max(_ll.level_max_dyn(lv) for lv in self.level_objects),
                                                    max(l.slots_used for l in self.layouts))
        self.dims = soa.Dims(W, H, max(1, D), self.num_agents, self.F)
        # env e of the whole (unsharded) batch plays level e % len(levels): keyed by the GLOBAL id, so a shard sees its own part
        self.env_level = (self.env_id_base + np.arange(self.num_envs)) % len(self.levels)
        self.spawn_cells = self.level_of_layout = None
        if self._spawn_cfg[0] or self._spawn_cfg[1]:
            # spawn areas per level (parsing.py:118-151: the AGENTS entries of the level file, one per agent up to MAX_COUNT each)
            self.spawn_cells = []                                        # [level][agent] -> (x candidates, y candidates)
            for lv in self.level_objects:
                cells = [(spec["X_POSITION"], spec["Y_POSITION"]) for spec in lv["AGENTS"] for _ in range(spec["MAX_COUNT"])][:self.num_agents]   # parsing.py:145
                self.spawn_cells.append([(list(xs), list(ys)) for xs, ys in cells])
            self.level_of_layout = np.zeros(len(self.layouts), dtype=np.uint8)
            for li, (base, count) in enumerate(self.pool_slices):
                self.level_of_layout[base:base + count] = li

    def shard(self, begin, count):
        """The tables of envs [begin, begin + count) of this batch: the same pool, recipes and spawn areas (shared, not
        copied), global ids env_id_base + begin ..."""
        import copy
        if not (0 <= begin and begin + count <= self.num_envs and count > 0):
            raise ValueError(f"shard [{begin}, {begin + count}) outside the batch of {self.num_envs} envs")
        t = copy.copy(self)
        t.num_envs, t.env_id_base = int(count), self.env_id_base + int(begin)
        t.recipe_ids = np.ascontiguousarray(self.recipe_ids[begin:begin + count])
        t.env_level = self.env_level[begin:begin + count]
        t.layouts = list(self.layouts)            # (every handle keeps its own record of what its pool holds after updates)
        return t


class CookingVecEnv:
    def __init__(self, num_envs, level=None, meta_file=None, num_agents=None, max_steps=None, recipes=None,
                 end_condition_all_dishes=False, action_scheme="scheme1", reward_scheme=None, *, num_layouts=256,
                 layout_seed=0, layouts=None, auto_reset=True, device_id=0, env_id_base=0, max_dyn=None, pinned_outputs=False,
                 agent_respawn_rate=0.0, grace_period=20, agent_despawn_rate=0.0, spawn_seed=0, tables=None):
        """`level` may be one level name/path or a list (env e uses levels[e % len], e the global id); `recipes` is a list of
        names (every env the same) or an int array [num_envs, R] of indices into the recipe book.
        `layouts` (optional) supplies pre-instantiated Layout objects per level instead of drawing
        `num_layouts` of them with random.Random(layout_seed).
        `pinned_outputs=True`: `step` / `reset` / `observe` return views of page-locked host buffers owned by the env
        (overwritten by the next call) instead of fresh arrays -- the copy engines then write them directly, which is what
        a host-array step of thousands of envs spends its time on (18 MB of observations per step at 4096 envs).
        `agent_despawn_rate` / `agent_respawn_rate` / `grace_period`: agent despawn / respawn (cooking_world.py:267-290)
        for every world of the batch, evaluated by the step kernels themselves with keyed random streams (cz_set_spawn) -
        on every stepping path (`step`, `step_device`, `step_device_ring`, `rollout`).  `self.spawn` is a read-only view of
        that bookkeeping (`active`, `grace`, and after a host-array `step` also `changed`).
        `tables`: a prepared `BatchTables` (then the configuration arguments before `auto_reset` are ignored)."""
        self._pinned = bool(pinned_outputs)
        self._pin_bufs = {}
        self.spawn = None
        if tables is None:
            tables = BatchTables(num_envs, level, meta_file, num_agents, max_steps, recipes, end_condition_all_dishes,
                                 action_scheme, reward_scheme, num_layouts=num_layouts, layout_seed=layout_seed,
                                 layouts=layouts, env_id_base=env_id_base, max_dyn=max_dyn,
                                 agent_respawn_rate=agent_respawn_rate, grace_period=grace_period,
                                 agent_despawn_rate=agent_despawn_rate, spawn_seed=spawn_seed)
        self.tables = tables
        for k, v in vars(tables).items():           # the env reads (and, for the layout pool, edits) its own copies of the names
            setattr(self, k, v)
        W, H = self.dims.W, self.dims.H

        # ---- device handle
        L = _native.lib()
        rs = self.reward_scheme
        self._cfg = _native.CzConfig(self.num_envs, self.num_agents, W, H, self.dims.D, self.F, self.scheme_class.CODE,
                                     self.max_steps, int(self.end_condition_all_dishes), self.num_recipes,
                                     int(bool(auto_reset)), int(device_id), int(self.env_id_base),
                                     float(rs["recipe_reward"]), float(rs["max_time_penalty"]),
                                     float(rs["recipe_penalty"]), float(rs["recipe_node_reward"]))
        h = C.c_void_p()
        rc = L.cz_create(C.byref(self._cfg), C.byref(h))
        if rc != 0:
            raise _native.NativeError((L.cz_last_error(None) or b"cz_create failed").decode())
        self._h = h
        self.device_id = int(device_id)
        assert L.cz_record_words(self._h) == self.dims.RW
        _native.check(self._h, L.cz_load_recipes(self._h, _ptr(self.recipe_table), len(self.book_names), self.recipe_nodes))
        _native.check(self._h, L.cz_load_partner_table(self._h, _ptr(self.partner_rows), len(self.book_names)))
        # (no table: goal ids beyond a byte, or a library built before the task calls - CZ_LIB in an A/B run; the rest works without)
        if self.goal_table is not None and _native.has("cz_load_goal_table"):
            _native.check(self._h, L.cz_load_goal_table(self._h, _ptr(self.goal_table), len(self.book_names), self.num_goals))
        self._upload_layouts()
        self._buffers = []
        self._policy_stage = {}          # load_policy's device copies of numpy weights, by role and shape
        self._ep_bufs = None                  # finished_episodes: the packed list and the count
        self._fork_buf = None                 # fork_device: the scratch archive, one row per env
        self._steps = 0                       # env steps issued so far (every stepping method counts; `advance` adds replayed ones)
        self.captured_steps = 0               # steps captured into graphs of the caller (they run at replay, see `advance`)
        self._caller_stream, self._warned_capture = False, False
        self._lay_groups, self._lay_active = 1, 0
        self._rot = None                      # rotate_layouts: the rotation.Rotation while one runs
        self.rotation_events = []             # (step index, "group", groups, active) / (step index, "layouts", first slot, [Layout])
                                              # / (step index, "generated", first slot, count, seed, generation)
        self._programs_for = None             # pool size the level programs on the device were uploaded for (generate_layouts)
        self._generated = {}                  # slot -> [Layout before, (seed, generation), ...]: device draws `self.layouts` has not caught up with
        if self.spawn_cells is not None:
            self._set_spawn()
            self.spawn = SpawnView(self)

    def _set_spawn(self):
        L, nl, A = _native.lib(), len(self.spawn_cells), self.num_agents
        stride = max(max(len(xs), len(ys)) for lv in self.spawn_cells for xs, ys in lv)
        if not 1 <= stride <= 1024:
            raise ValueError("a spawn area lists 1..1024 x and y candidates")
        sx, sy = np.zeros((nl, A, stride), dtype=np.uint8), np.zeros((nl, A, stride), dtype=np.uint8)
        nx, ny = np.zeros((nl, A), dtype=np.int32), np.zeros((nl, A), dtype=np.int32)
        for li, lv in enumerate(self.spawn_cells):
            if len(lv) < A:
                raise ValueError(f"level {self.levels[li]} has spawn areas for {len(lv)} agent(s) only")
            for a, (xs, ys) in enumerate(lv):
                if not xs or not ys:
                    raise ValueError("a spawn area lists 1..1024 x and y candidates")
                nx[li, a], ny[li, a] = len(xs), len(ys)
                # (a candidate beyond the grid can never be taken: 255 stands for any of them)
                sx[li, a, :len(xs)] = [v if 0 <= v < 255 else 255 for v in xs]
                sy[li, a, :len(ys)] = [v if 0 <= v < 255 else 255 for v in ys]
        d, r, g, seed = self._spawn_cfg
        _native.check(self._h, L.cz_set_spawn(self._h, d, r, g, seed, nl, _ptr(self.level_of_layout), stride, _ptr(sx), _ptr(nx), _ptr(sy), _ptr(ny)))

    def set_spawn_rates(self, agent_despawn_rate, agent_respawn_rate, grace_period, spawn_seed=None):
        """Change the despawn / respawn parameters of a live batch (cz_set_spawn: takes effect with the next step; running episodes keep
        their countdowns, re-packed by the library if the period crosses 31 and the fields change their width)."""
        if self.spawn_cells is None:
            raise ValueError("the env was made without despawn / respawn (no spawn areas were collected)")
        seed = self._spawn_cfg[3] if spawn_seed is None else int(spawn_seed)
        self._spawn_cfg = (float(agent_despawn_rate), float(agent_respawn_rate), int(grace_period), seed)
        self._set_spawn()

    def spawn_exhausted(self):
        """respawns that found no free cell of their spawn area in 1001 tries (the reference raises there) since the env was made"""
        return int(_native.lib().cz_spawn_exhausted(self._h))

    # ------------------------------------------------------------------ tables
    def _upload_layouts(self):
        recs = np.stack([l.init_record(self.dims, i) for i, l in enumerate(self.layouts)])
        desc = np.stack([l.obs_descriptor(self.meta, self.dims) for l in self.layouts])
        self._lay_records, self._lay_desc = recs, desc
        _native.check(self._h, _native.lib().cz_load_layouts(self._h, _ptr(recs), _ptr(desc), len(self.layouts)))
        self._upload_ranks(0, self.layouts)

    def _upload_ranks(self, first, layouts, ranks=None):
        """the rank rows of pool slots [first, first + len(layouts)): the list order of the static objects (partner_device)"""
        if ranks is None:
            ranks = np.stack([_partner.rank_table(l) for l in layouts])
        ranks = np.ascontiguousarray(ranks, dtype=np.uint16)
        _native.check(self._h, _native.lib().cz_load_layout_ranks(self._h, int(first), len(layouts), _ptr(ranks)))

    def set_layouts(self, layouts):
        """Replace the whole pool (single-level batches; used by the single-env facade at reset)."""
        if self.spawn is not None and len(self.levels) > 1:
            raise ValueError("set_layouts replaces the pool of a single-level batch; a multi-level batch with despawn / respawn "
                             "would lose its layout -> level map (use update_layouts, which keeps every slot's level)")
        self.layouts = list(layouts)
        self.pool_slices = [(0, len(self.layouts))]
        self._programs_for, self._generated = None, {}               # (cz_load_layouts drops the level programs' slot map)
        self._upload_layouts()
        if self.spawn is not None:                                       # (the spawn tables map every layout of the pool to its level)
            self.level_of_layout = np.zeros(len(self.layouts), dtype=np.uint8)
            self._set_spawn()

    # ------------------------------------------------------------------ fresh layouts under a stepping batch
    def update_layouts(self, first, layouts):
        """Replace pool slots [first, first + len(layouts)) while the batch keeps stepping (cz_update_layouts: a copy stream
        of the library's own; the handle's stream is not touched).  Only slots that no env can draw or is playing on."""
        recs = np.stack([l.init_record(self.dims, first + k) for k, l in enumerate(layouts)])
        desc = np.stack([l.obs_descriptor(self.meta, self.dims) for l in layouts])
        self._update_layout_arrays(first, layouts, recs, desc)

    def _update_layout_arrays(self, first, layouts, recs, desc, ranks=None):
        _native.check(self._h, _native.lib().cz_update_layouts(self._h, int(first), len(layouts), _ptr(recs), _ptr(desc)))
        self._upload_ranks(first, layouts, ranks)
        self.layouts[first:first + len(layouts)] = list(layouts)
        self._lay_records[first:first + len(layouts)] = recs
        self._lay_desc[first:first + len(layouts)] = desc
        self.rotation_events.append((self._steps, "layouts", int(first), list(layouts)))

    # ------------------------------------------------------------------ fresh layouts drawn on the device
    def level_of_slot(self):
        """uint8 [pool size]: the level (index into `levels`) every pool slot instantiates"""
        out = np.zeros(len(self.layouts), dtype=np.uint8)
        for li, (base, count) in enumerate(self.pool_slices):
            out[base:base + count] = li
        return out

    def load_level_programs(self):
        """Compile every level of the batch into a level program (engine/level_program.py) and upload them with the slot ->
        level map (cz_load_level_programs).  `generate_layouts` does this on first use and after the pool changed size."""
        from cooking_zoo_amd.cooking_world.engine import level_program as _lp
        progs = [_lp.compile_level(lv, self.meta, self.num_agents, self.dims) for lv in self.level_objects]
        words = np.ascontiguousarray(np.concatenate(progs), dtype=np.uint32)
        los = self.level_of_slot()
        _native.check(self._h, _native.lib().cz_load_level_programs(self._h, _ptr(words), int(words.size), len(progs), _ptr(los)))
        self._programs_for = len(self.layouts)

    def keyed_layouts(self, first, count, seed, generation, previous=None):
        """The host model of `generate_layouts`: ([Layout] of slots [first, first + count) for (seed, generation), failed draws).
        A failed draw (the reference raises) keeps `previous[k]`, None without `previous`."""
        from cooking_zoo_amd.cooking_world.engine import level_program as _lp
        return _lp.keyed_layouts(self.level_objects, self.meta, self.num_agents, self.dims, self.level_of_slot(), seed, generation,
                                 first, count, previous)

    def generate_layouts(self, first, count, generation, seed=None, mirror=True):
        """Draw pool slots [first, first + count) anew ON THE DEVICE: one launch on the env's stream (cz_generate_layouts), no
        host arrays, legal inside a stream capture of the caller.  Every draw comes from the stream keyed by (seed, pool slot,
        generation) - `seed` defaults to the env's `layout_seed` -, so the result depends on nothing else: not on the batch size,
        the shard or the timing.  Only slots that no env can draw or is playing on (refused for the part in use once
        `set_layout_group` has cut the pool).  `mirror=True` also evaluates the host model (`keyed_layouts`) so that
        `self.layouts` stays what the pool holds; `mirror=False` leaves that to `resolve_layouts()` (until then the slots read None)."""
        first, count, generation = int(first), int(count), int(generation)
        seed = int(self.layout_seed if seed is None else seed)
        if self._programs_for != len(self.layouts):
            self.load_level_programs()
        _native.check(self._h, _native.lib().cz_generate_layouts(self._h, first, count, seed, generation))
        self.rotation_events.append((self._steps, "generated", first, count, seed, generation))
        for s in range(first, first + count):
            hist = self._generated.setdefault(s, [self.layouts[s]])       # what the slot held, then the draws since
            hist.append((seed, generation))
            self.layouts[s] = None
        if mirror:
            self.resolve_layouts()

    def resolve_layouts(self):
        """Bring `self.layouts` up to date with the device draws issued with `mirror=False` (host model, milliseconds)."""
        los = self.level_of_slot()
        from cooking_zoo_amd.cooking_world.engine import level_program as _lp
        for s, hist in sorted(self._generated.items()):
            lay = hist[0]
            for seed, generation in hist[1:]:
                new, _ = _lp.keyed_layout(self.level_objects[int(los[s])], self.meta, self.num_agents, self.dims, seed, s, generation)
                lay = new if new is not None else lay            # a failed draw leaves the slot as it was
            self.layouts[s] = lay
            self._lay_records[s] = lay.init_record(self.dims, s)
            self._lay_desc[s] = lay.obs_descriptor(self.meta, self.dims)
        self._generated = {}

    def generate_failures(self):
        """device draws that failed (the reference raises there; the slot kept its layout) since the level programs were loaded"""
        return int(_native.lib().cz_generate_failures(self._h))

    def set_layout_group(self, groups, active):
        """From the next step on the envs draw their next episodes from part `active` of their pool slices cut into `groups`
        equal parts (cz_set_layout_group; waits on the device for the updates issued so far)."""
        if any(count % groups for _, count in self.pool_slices):
            raise ValueError("every level's pool slice must be a multiple of `groups` layouts long")
        _native.check(self._h, _native.lib().cz_set_layout_group(self._h, int(groups), int(active)))
        self._lay_groups, self._lay_active = int(groups), int(active)
        self.rotation_events.append((self._steps, "group", int(groups), int(active)))

    def rotate_layouts(self, every, *, groups=2, seed=0, prefetch=2, blocking=True, device=False):
        """Keep the layout pool fresh while the batch steps - the batched counterpart of the reference instantiating a new
        level at every reset (cooking_env.py:191-195, parsing.py:21-151).  The pool slices are cut into `groups` parts; the
        envs draw from one; every `every` steps (at the next call boundary) the next part becomes the one drawn from, and
        once the episodes that started on the old part are over (max_steps + 2 steps later) it is refilled with layouts
        a background process has instantiated meanwhile (engine/load_level.py, its own seeded stream per refill).  Which
        layouts an env sees is a function of the sequence of stepping calls only (the refill waits for that process if it
        has to), so a run can be replayed: `rotation_events` lists what was switched / replaced at which step.
        `blocking=False` never waits: a refill whose layouts are not ready yet is tried again at the next call boundary (and
        the next switch with it), which keeps the stepping thread free of stalls at the price of a timing-dependent schedule.
        Steps that run as replays of a graph of the CALLER (captured `step_device*` launches) are invisible here: report them with
        `advance(k)` after every replay - the switches and refills then happen in that call, between replays.
        `device=True`: the same switch / refill schedule with no process, no threads and no waiting - refill number r (1, 2, ...)
        is `generate_layouts` of the retired part with generation r under `seed`, a launch on the env's own stream
        (`rotation_events` then holds "generated" entries; `keyed_layouts` turns them into `Layout`s)."""
        if self._rot is not None:
            raise RuntimeError("rotate_layouts is already running")
        if groups < 2 or any(count % groups for _, count in self.pool_slices):
            raise ValueError("need groups >= 2 and pool slices that are multiples of `groups` long")
        if every < self.max_steps + 3:
            raise ValueError("`every` must be at least max_steps + 3 steps: a part is refilled max_steps + 2 steps after the "
                             "envs stopped drawing from it, and before they draw from it again")
        start = self._lay_active if self._lay_groups == groups else 0        # the part in use now: the first one to be refilled
        if device:
            if self._programs_for != len(self.layouts):
                self.load_level_programs()
            source = _rotation.DeviceRefill(groups, seed)
        else:
            _native.check(self._h, _native.lib().cz_update_layouts(self._h, 0, 0, None, None))     # copy stream + staging, ahead of time
            source = _rotation.ProcessRefill.spawn((self.level_objects, self.meta, self.num_agents, self.dims.as_tuple(),
                                                    list(self.pool_slices), int(groups), int(seed), int(start)), prefetch, blocking)
        self._rot = _rotation.Rotation(source, every, groups, start, self._steps)
        self.set_layout_group(groups, start)
        source.start()

    def stop_rotation(self):
        if self._rot is not None:
            rot, self._rot = self._rot, None
            rot.source.stop()

    def rotation_ready(self):
        """refills the background process has ready right now (a measurement may want to start with a full queue)"""
        return 0 if self._rot is None else self._rot.source.ready()

    def _issued(self, k):
        """a device-pointer call of k steps has returned: count them - unless the call was CAPTURED into a graph of the caller
        (nothing ran; the steps run whenever that graph is replayed, which Python does not see: the caller reports them with
        `advance`)"""
        if self._caller_stream and _native.lib().cz_stream_capturing(self._h):
            self.captured_steps += int(k)
            if self._rot is not None and not self._warned_capture:
                self._warned_capture = True
                import warnings
                warnings.warn("steps captured into a graph of the caller while rotate_layouts is active: call env.advance(k) after "
                              "every replay of k captured steps, or the layout pool is never switched / refilled", RuntimeWarning, stacklevel=3)
            return
        self._advance(k)

    def advance(self, k):
        """Tell the env that k env steps ran which it did not issue itself: replays of a graph of the caller that holds captured
        `step_device*` / `rollout*` launches (hipGraphLaunch, torch.cuda.CUDAGraph.replay()).  Keeps `rotate_layouts` on schedule:
        the switch to the next part of the pool and the refill of the retired one happen here, between replays."""
        if self._caller_stream and _native.lib().cz_stream_capturing(self._h):
            raise RuntimeError("advance() inside a stream capture: call it after the replay, outside the capture")
        self._advance(k)

    def _advance(self, k):
        """k more env steps have been issued: switch / refill when due"""
        self._steps += int(k)
        if self._rot is None:
            return
        self._rot.advanced(self)

    # ------------------------------------------------------------------ reset / step
    def initial_layout_ids(self):
        """Episode-0 layout of every env: the same keyed draw auto-reset uses (shard invariant)."""
        ids = np.empty(self.num_envs, dtype=np.int32)
        pools = np.empty(self.num_envs, dtype=np.uint32)
        L = _native.lib()
        for e in range(self.num_envs):
            base, count = self.pool_slices[self.env_level[e]]
            pools[e] = base | (count << 16)
            ids[e] = L.cz_next_layout_group(self.env_id_base + e, 0, int(pools[e]), len(self.layouts), self._lay_groups, self._lay_active)
        return ids, pools

    def reset(self, layout_ids=None, return_obs=True, env_begin=0, env_count=None, return_codes=False):
        """-> the float64 observation [n, A, F] (return_obs), the compact one uint8 [n, A, codes_pitch] (return_codes; then
        return_obs is ignored), or None"""
        if return_codes:
            self.reset(layout_ids, False, env_begin, env_count)
            return self.observe_compact(env_begin, env_count)
        n = self._count(env_count)
        ids, pools = self.initial_layout_ids()
        if layout_ids is not None:
            ids = np.ascontiguousarray(layout_ids, dtype=np.int32)
        else:
            ids = ids[env_begin:env_begin + n].copy()
        pools = np.ascontiguousarray(pools[env_begin:env_begin + n])
        obs = self._host_array("obs", (n, self.num_agents, self.F), np.float64) if return_obs else None
        rid = np.ascontiguousarray(self.recipe_ids[env_begin:env_begin + n])
        _native.check(self._h, _native.lib().cz_reset(self._h, env_begin, n, _ptr(ids), _ptr(rid), _ptr(pools), _ptr(obs)))
        if self.spawn is not None:
            self.spawn.refresh(reset=True)
        return obs

    def _count(self, env_count):
        """the env count of a ranged call: every env unless given"""
        return self.num_envs if env_count is None else int(env_count)

    @contextlib.contextmanager
    def _scratch(self, *specs):
        """scratch DeviceBuffers for one call, one per (shape, dtype[, initial host array]); all freed on exit"""
        bufs = []
        try:
            for shape, dtype, *init in specs:
                bufs.append(DeviceBuffer(self, shape, dtype))
                if init:
                    bufs[-1].from_host(init[0])
            yield bufs
        finally:
            for b in bufs:
                b.free()

    def _host_array(self, key, shape, dtype):
        """a fresh array, or (pinned_outputs) the env's page-locked buffer of that role"""
        if not self._pinned:
            return np.empty(shape, dtype=dtype)
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        buf = self._pin_bufs.get(key)
        if buf is None or buf[1] < nbytes:
            if buf is not None:
                _native.lib().cz_host_free(self._h, buf[0])
            p = _native.lib().cz_host_alloc(self._h, max(nbytes, 1))
            if not p:
                _native.check(self._h, 1)
            buf = self._pin_bufs[key] = (p, max(nbytes, 1))
        raw = (C.c_uint8 * nbytes).from_address(buf[0])
        return np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def step(self, actions, return_obs=True):
        """actions int [N, A] -> (obs f64 [N, A, F] | None, rewards f64 [N, A], terminations u8, truncations u8).
        An action of -1 means "this agent is despawned": it is left out of the step (cooking_world.py:105-108)."""
        N, A = self.num_envs, self.num_agents
        acts = self._host_array("act", (N, A), np.int32)
        acts[...] = np.asarray(actions).reshape(N, A)
        if acts.size and int(acts.max()) >= self.n_actions:
            raise ValueError(f"actions must be in [0, {self.n_actions}) for {self.action_scheme} (negative = despawned agent)")
        obs = self._host_array("obs", (N, A, self.F), np.float64) if return_obs else None
        rew = self._host_array("rew", (N, A), np.float64)
        term = self._host_array("term", (N, A), np.uint8)
        trunc = self._host_array("trunc", (N, A), np.uint8)
        _native.check(self._h, _native.lib().cz_step(self._h, _ptr(acts), _ptr(obs), _ptr(rew), _ptr(term), _ptr(trunc)))
        if self.spawn is not None:
            self.spawn.refresh()                                          # (the kernel did the bookkeeping: this only reads it back)
        self._advance(1)
        return obs, rew, term, trunc

    def step_compact(self, actions):
        """`step` with the observation as one byte per feature: -> (codes uint8 [N, A, codes_pitch], rewards, terminations,
        truncations); `obs_table()[codes[..., :F]]` is the float64 observation bit for bit.  An eighth of the bytes over PCIe."""
        N, A = self.num_envs, self.num_agents
        acts = self._host_array("act", (N, A), np.int32)
        acts[...] = np.asarray(actions).reshape(N, A)
        if acts.size and int(acts.max()) >= self.n_actions:
            raise ValueError(f"actions must be in [0, {self.n_actions}) for {self.action_scheme} (negative = despawned agent)")
        codes = self._host_array("codes", (N, A, self.codes_pitch), np.uint8)
        rew = self._host_array("rew", (N, A), np.float64)
        term = self._host_array("term", (N, A), np.uint8)
        trunc = self._host_array("trunc", (N, A), np.uint8)
        _native.check(self._h, _native.lib().cz_step_compact(self._h, _ptr(acts), _ptr(codes), _ptr(rew), _ptr(term), _ptr(trunc)))
        if self.spawn is not None:
            self.spawn.refresh()
        self._advance(1)
        return codes, rew, term, trunc

    def last_marks(self):
        """Recipe-node marks after the most recent host-array `step`: uint64 [N], bit 8r + j = node j of the env's r-th
        recipe (compact tables) or bit 16r + j (wide tables, `recipe_nodes == 16`)."""
        words = np.empty((self.num_envs, 2), dtype=np.uint32)
        _native.check(self._h, _native.lib().cz_last_marks(self._h, _ptr(words)))
        return words[:, 0].astype(np.uint64) | (words[:, 1].astype(np.uint64) << np.uint64(32))

    def marks_of(self, marks, r):
        """the node marks of recipe r inside a marks value (an int): bit j = node j of node_list"""
        bits = 8 if self.recipe_nodes == soa.NARROW_NODES else 16
        return (int(marks) >> (bits * r)) & ((1 << bits) - 1)

    def observe(self, env_begin=0, env_count=None):
        n = self._count(env_count)
        obs = self._host_array("obs", (n, self.num_agents, self.F), np.float64)
        _native.check(self._h, _native.lib().cz_observe(self._h, env_begin, n, _ptr(obs)))
        return obs

    def observe_compact(self, env_begin=0, env_count=None):
        """`observe` as one byte per feature: uint8 [n, A, codes_pitch]; `obs_table()[codes[..., :F]]` is the float64 observation"""
        n = self._count(env_count)
        codes = self._host_array("codes", (n, self.num_agents, self.codes_pitch), np.uint8)
        _native.check(self._h, _native.lib().cz_observe_compact(self._h, env_begin, n, _ptr(codes)))
        return codes

    def observe_device(self, d_obs=None, d_codes=None, env_begin=0, env_count=None, d_obs32=None):
        """the current observation into device buffers (float64 [n, A, F] and / or codes uint8 [n, A, codes_pitch] and / or float32
        [n, A, F] rows, the form of `step_device_f32`), stream-ordered: what a device-resident consumer reads before its first step"""
        n = self._count(env_count)
        if d_obs is not None or d_codes is not None or d_obs32 is None:
            _native.check(self._h, _native.lib().cz_observe_device(self._h, env_begin, n, _dev_ptr(d_obs), _dev_ptr(d_codes)))
        if d_obs32 is not None:
            _native.check(self._h, _native.lib().cz_observe_device_f32(self._h, env_begin, n, _dev_ptr(d_obs32)))

    def grid_shape(self, extended=False):
        """(W, H, C) of one env's grid observation: C = 32 reference channels, 48 when `extended` (cooking_zoo_amd/grid.py)"""
        return (self.dims.W, self.dims.H, _grid.n_channels(extended))

    def observe_grid_device(self, d_bits=None, d_grid8=None, d_grid32=None, d_agent_xy=None, extended=False, env_begin=0, env_count=None):
        """the grid observation of the current state - the reference's (W, H, 32) `full` tensor, cell (x, y) at x * H + y - into
        device buffers, stream-ordered and capturable: `d_bits` uint32 [n, W, H, C / 32], `d_grid8` uint8 [n, W, H, C], `d_grid32`
        float32 [n, W, H, C] (a torch tensor's `permute(0, 3, 1, 2)` is the channels_last image), `d_agent_xy` int32 [n, A, 2];
        at least one of them"""
        n = self._count(env_count)
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_observe_grid_device(self._h, env_begin, n, int(extended), p(d_bits), p(d_grid8), p(d_grid32),
                                                                    p(d_agent_xy)))

    def observe_grid(self, extended=False, env_begin=0, env_count=None):
        """host convenience: (uint8 [n, W, H, C], int32 [n, A, 2]) of envs [env_begin, env_begin + n)"""
        n = self._count(env_count)
        shape = (n,) + self.grid_shape(extended)
        if n == 0:
            return np.zeros(shape, np.uint8), np.zeros((0, self.num_agents, 2), np.int32)
        with self._scratch((shape, np.uint8), ((n, self.num_agents, 2), np.int32)) as (d_grid, d_xy):
            self.observe_grid_device(d_grid8=d_grid, d_agent_xy=d_xy, extended=extended, env_begin=env_begin, env_count=n)
            return d_grid.to_host(), d_xy.to_host()

    def load_sprites(self, sprites=None, M=None):
        """the sprite sheet `render_device` draws with: uint8 [render.N_SPRITES, M, M, 4] RGBA (cooking_zoo_amd/render.py: SPRITES,
        `builtin_sprites`, `load_directory`); None: the builtin procedural sheet at M (default 16).  Uploads once and replaces an
        earlier sheet; not capturable"""
        if sprites is None:
            sprites = _render.builtin_sprites(16 if M is None else M)
        sheet = _render.check_sheet(sprites)
        if M is not None and int(M) != sheet.shape[1]:
            raise ValueError(f"load_sprites: M = {M}, the sheet is {sheet.shape[1]} x {sheet.shape[2]}")
        _native.check(self._h, _native.lib().cz_load_sprites(self._h, _ptr(sheet), sheet.shape[0], sheet.shape[1]))
        self._sprites_loaded = True

    def frame_shape(self, P=16):
        """(H * P, W * P, 3) of one env's frame at tile size P: gymnasium's (height, width, 3)"""
        return (self.dims.H * int(P), self.dims.W * int(P), 3)

    def render_device(self, d_rgb8=None, d_chw32=None, P=16, vis=0, env_begin=0, env_count=None):
        """frames of the current state (cooking_zoo_amd/render.py) into device buffers, stream-ordered and capturable: `d_rgb8` uint8
        [n, H * P, W * P, 3] and / or `d_chw32` float32 [n, 3, H * P, W * P] = `render.to_chw32` (what a convolution takes); at least one of
        them.  `vis` bit a: agent a is drawn as a robot.  Needs a sheet (`load_sprites`)"""
        n = self._count(env_count)
        _native.check(self._h, _native.lib().cz_render_device(self._h, env_begin, n, int(P), int(vis), _dev_ptr(d_rgb8), _dev_ptr(d_chw32)))

    def render(self, env_begin=0, env_count=1, P=16, vis=0):
        """host convenience: uint8 [n, H * P, W * P, 3] of envs [env_begin, env_begin + n); loads the builtin sheet on first use"""
        n = int(env_count)
        shape = (n,) + self.frame_shape(P)
        if not getattr(self, "_sprites_loaded", False):
            self.load_sprites()
        if n == 0:
            return np.zeros(shape, np.uint8)
        with self._scratch((shape, np.uint8)) as (d_rgb,):
            self.render_device(d_rgb8=d_rgb, P=P, vis=vis, env_begin=env_begin, env_count=n)
            return d_rgb.to_host()

    def navigate_device(self, d_target, d_action=None, d_steps=None, d_field=None, walkable_blocks=False, env_begin=0, env_count=None,
                        T=None):
        """shortest-path navigation on the current state - the reference's `BaseAgent.walk_to_location` / `reachable` for every
        agent and T candidate goals each (cooking_zoo_amd/nav.py) - into device buffers, stream-ordered and capturable:
        `d_target` int32 [n, A, T, 2] (x, y; (-1, -1) or any off-grid value: no target), `d_action` int32 [n, A, T] (walk codes
        0..4; with T = 1 the array `step_device` takes), `d_steps` int32 [n, A, T] (0 at the goal, -1 unreachable), `d_field`
        uint16 [n, A, T, W * H] (cell (x, y) at x * H + y, 0xFFFF unreachable); at least one output.  T is read from the target
        buffer's shape ([n, A, T, 2], or [n, A, 2] for T = 1) unless given."""
        n = self._count(env_count)
        if T is None:
            shape = tuple(getattr(d_target, "shape", ()))
            if len(shape) not in (3, 4) or shape[-1] != 2 or shape[-3 if len(shape) == 4 else -2] != self.num_agents:
                raise ValueError(f"navigate_device: the target buffer's shape is {shape}, not [n, A, T, 2] (or [n, A, 2]); pass T")
            T = shape[2] if len(shape) == 4 else 1
        flags = _nav.WALKABLE_BLOCKS if walkable_blocks else 0
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_navigate_device(self._h, env_begin, n, int(T), flags, p(d_target), p(d_action), p(d_steps),
                                                                p(d_field)))

    def navigate(self, targets, walkable_blocks=False, env_begin=0, env_count=None):
        """host convenience: targets int [n, A, T, 2] (or [n, A, 2]) -> (actions int32 [n, A, T], steps int32 [n, A, T]) of envs
        [env_begin, env_begin + n)"""
        n = self._count(env_count)
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        T = tg.shape[2] if tg.ndim == 4 else 1
        if n == 0:
            return np.zeros((0, self.num_agents, T), np.int32), np.zeros((0, self.num_agents, T), np.int32)
        tg = tg.reshape(n, self.num_agents, T, 2)
        shape = (n, self.num_agents, T)
        with self._scratch((tg.shape, np.int32, tg), (shape, np.int32), (shape, np.int32)) as (d_t, d_a, d_s):
            self.navigate_device(d_t, d_a, d_s, walkable_blocks=walkable_blocks, env_begin=env_begin, env_count=n)
            return d_a.to_host(), d_s.to_host()

    def _recipe_indices(self, recipes, n, width=None):
        """recipe names or table indices, one per agent or [n, A] -> int32 [n, A] indices into the loaded recipe table (`width`: per
        recipe slot, [R] or [n, R], instead)"""
        width = self.num_agents if width is None else int(width)
        flat = [self.book_names.index(r) if isinstance(r, str) else int(r) for r in np.asarray(recipes, dtype=object).reshape(-1)]
        idx = np.asarray(flat, dtype=np.int32)
        if idx.size == width:
            idx = np.tile(idx, (n, 1))
        return np.ascontiguousarray(idx.reshape(n, width))

    def partner_device(self, d_action=None, d_target=None, d_status=None, agents=None, d_recipe=None, env_begin=0, env_count=None):
        """the scripted partner on the current state - the action the reference's heuristic `CookingAgent` returns
        (cooking_zoo_amd/partner.py) - into device buffers, stream-ordered and capturable: `d_action` int32 [n, A] (walk codes 0..4:
        the array `step_device` takes), `d_target` int32 [n, A, 2] (where the walk goes, (-1, -1) without one: a T = 1 target array
        of `navigate_device`), `d_status` uint8 [n, A] (partner.DONE / WALK / IDLE / RAISES / ABSENT); at least one output.
        `agents`: bit a = agent a is driven (None: all); the entries of the other agents are left untouched in every output.
        `d_recipe` int32 [n, A]: indices into the recipe table (`book_names`); None: every env's own recipes."""
        n = self._count(env_count)
        mask = (1 << self.num_agents) - 1 if agents is None else int(agents)
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_partner_device(self._h, env_begin, n, mask, 0, p(d_recipe), p(d_action), p(d_target), p(d_status)))

    def partner_bad_recipes(self):
        """agents that `partner_device` was asked to drive with a recipe index outside the table (they got IDLE); waits"""
        return int(_native.lib().cz_partner_bad_recipes(self._h))

    def partner(self, agents=None, recipes=None, env_begin=0, env_count=None):
        """host convenience: (actions int32 [n, A], targets int32 [n, A, 2], status uint8 [n, A]) of envs [env_begin, env_begin + n);
        `recipes`: names or table indices, one per agent or [n, A] (None: the envs' own).  An agent that is not driven reads
        0, (-1, -1), partner.IDLE."""
        n = self._count(env_count)
        A = self.num_agents
        if n == 0:
            return np.zeros((0, A), np.int32), np.zeros((0, A, 2), np.int32), np.zeros((0, A), np.uint8)
        specs = [((n, A), np.int32, np.zeros((n, A), np.int32)), ((n, A, 2), np.int32, np.full((n, A, 2), -1, np.int32)),
                 ((n, A), np.uint8, np.full((n, A), _partner.IDLE, np.uint8))]
        if recipes is not None:
            specs.append(((n, A), np.int32, self._recipe_indices(recipes, n)))
        with self._scratch(*specs) as bufs:
            self.partner_device(bufs[0], bufs[1], bufs[2], agents=agents, d_recipe=bufs[3] if recipes is not None else None,
                                env_begin=env_begin, env_count=n)
            return bufs[0].to_host(), bufs[1].to_host(), bufs[2].to_host()

    @property
    def num_actions(self):
        """action codes per agent: 5 (scheme3) or 8 (scheme1)"""
        return _effects.num_actions(self.scheme_class.CODE)

    def action_effects_device(self, d_mask=None, d_effects=None, agents=None, ignore=0, env_begin=0, env_count=None):
        """action masks of the current state - which of an agent's actions would change anything if it played them alone
        (cooking_zoo_amd/effects.py) - into device buffers, stream-ordered and capturable: `d_mask` uint8 [n, A, num_actions]
        (1: code 0, or the action has an effect outside `ignore`; `logits.masked_fill(~mask.bool(), -inf)`), `d_effects` uint8
        [n, A, num_actions] (effects.MOVED | TURNED | HAND | OBJECTS | CELLS); at least one output.  `agents`: bit a = agent a is
        asked for (None: all); the rows of the other agents are left untouched in both outputs.  `ignore`: effect bits that do not
        make an action count (effects.TURNED: turning on the spot is a no-op).  A despawned agent and every agent of a finished env
        get the noop-only row.  The records are only read; not a step."""
        n = self._count(env_count)
        chosen = (1 << self.num_agents) - 1 if agents is None else int(agents)
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_action_effects_device(self._h, env_begin, n, chosen, int(ignore), p(d_mask), p(d_effects)))

    def action_mask(self, agents=None, ignore=0, env_begin=0, env_count=None):
        """host convenience: (mask uint8 [n, A, num_actions], effects uint8 [n, A, num_actions]) of envs [env_begin, env_begin + n).
        An agent that is not asked for reads the noop-only row and effects 0."""
        n = self._count(env_count)
        shape = (n, self.num_agents, self.num_actions)
        noop = np.zeros(shape, np.uint8)
        noop[..., 0] = 1
        if n == 0:
            return noop, np.zeros(shape, np.uint8)
        with self._scratch((shape, np.uint8, noop), (shape, np.uint8, np.zeros(shape, np.uint8))) as (d_m, d_e):
            self.action_effects_device(d_m, d_e, agents=agents, ignore=ignore, env_begin=env_begin, env_count=n)
            return d_m.to_host(), d_e.to_host()

    # ------------------------------------------------------------------ device-resident API
    def alloc(self, shape, dtype):
        b = DeviceBuffer(self, shape, dtype)
        self._buffers.append(b)
        return b

    def set_ring_fused(self, enabled=True):
        """Runs of two or more steps of `step_device_ring` whose action slots are densely packed (`action_stride == num_envs *
        num_agents`) go out as fused launches - one per stretch of consecutive slots, the state in registers across the steps,
        every step's outputs written in place: the same final state, outputs and statistics as one launch per step, at the cost
        per step of a fused rollout (4.0-4.3 instead of 5.1-5.8 us at 4096 envs).  Open loop only.  Returns the previous setting."""
        rc = _native.lib().cz_set_ring_fused(self._h, 1 if enabled else 0)
        if rc < 0:
            raise _native.NativeError((_native.lib().cz_last_error(self._h) or b"cz_set_ring_fused failed").decode())
        return bool(rc)

    def ring_fused_steps(self, reset=False):
        return int(_native.lib().cz_ring_fused_steps(self._h, 1 if reset else 0))

    def set_ring_split(self, mode=-1):
        """Runs of `step_device_ring` / `step_device_many` as two launch chains over the two halves of the batch, on two streams of
        the handle (cz_set_ring_split): -1 automatic (the default: the replayed pieces of the batch sizes at which it measured
        faster), 0 off, 2 two parts whatever the size, directly launched pieces included.  Results are bit for bit those of the
        unsplit run.  Drops the ring graphs built so far.  Returns the previous mode."""
        rc = _native.lib().cz_set_ring_split(self._h, int(mode))
        if rc < -1:
            raise _native.NativeError((_native.lib().cz_last_error(self._h) or b"cz_set_ring_split failed").decode())
        return int(rc)

    def ring_split_parts(self):
        """in how many launch chains (1 or 2) a run outside a stream capture of the caller goes out as things stand"""
        return int(_native.lib().cz_ring_split_parts(self._h))

    def set_stream(self, stream=None):
        """Order this env's device work on the caller's HIP stream: an int / ctypes pointer, or an object with a
        `cuda_stream` attribute such as torch.cuda.current_stream().  None = the env's own stream."""
        raw = getattr(stream, "cuda_stream", stream)
        raw = getattr(raw, "value", raw)                               # (ctypes.c_void_p)
        _native.check(self._h, _native.lib().cz_set_stream(self._h, C.c_void_p(int(raw)) if raw else None))
        self._caller_stream = bool(raw)

    def step_device(self, d_actions, d_obs, d_rewards, d_term, d_trunc):
        """Device-resident step.  Buffers: DeviceBuffer, a raw device address (int), or anything with `data_ptr()`
        (a torch tensor on this GPU: int32 [N, A] actions, float64 [N, A, F] observations, float64 [N, A] rewards,
        uint8 [N, A] flags, all contiguous)."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_step_device(self._h, p(d_actions), p(d_obs), p(d_rewards), p(d_term),
                                                            p(d_trunc)))
        self._issued(1)

    def step_device_compact(self, d_actions, d_codes, d_rewards, d_term, d_trunc, d_obs=None):
        """Device-resident step whose observation is one byte per feature: d_codes uint8 [N, A, codes_pitch] receives the index
        of every feature's value in `obs_table()` (256 float64; `obs_table()[codes]` is the float64 observation bit for bit).
        d_obs (optional): the float64 [N, A, F] observation as well."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_step_device_compact(self._h, p(d_actions), p(d_codes), p(d_obs), p(d_rewards), p(d_term),
                                                                    p(d_trunc)))
        self._issued(1)

    def reset_device(self, d_mask=None, d_layout_ids=None, d_obs=None, d_obs32=None, d_codes=None):
        """`reset()` (cooking_env.py:178-210) of chosen envs, decided on the device: one launch on the env's stream, no copy and no
        wait, legal inside a capture, and no env-step is spent (unlike the auto-reset pass).  d_mask uint8 [N]: env e restarts when
        d_mask[e] != 0, finished or not; None: every finished env.  d_layout_ids int32 [N]: the layout of env e where >= 0, else (or
        None) the keyed draw auto-reset makes; an id past the pool is refused - the env stays as it was, `reset_device_refused`
        counts it.  d_obs float64 [N, A, F], d_obs32 float32 [N, A, F], d_codes uint8 [N, A, codes_pitch]: whole-batch buffers of which
        only the rows of the restarted envs are written.  Buffers as in `step_device`.  Not a step: layout rotation does not advance."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_reset_device(self._h, p(d_mask), p(d_layout_ids), p(d_obs), p(d_obs32), p(d_codes)))

    def reset_device_refused(self):
        """envs `reset_device` left alone because their explicit layout id was past the pool, since the env was created (waits)"""
        n = int(_native.lib().cz_reset_device_refused(self._h))
        if n < 0:
            _native.check(self._h, 1)
        return n

    # ------------------------------------------------------------------ tasks (cooking_zoo_amd/tasks.py)
    def set_tasks_device(self, d_mask=None, d_recipe_ids=None, d_task_list=None, seed=0, K=None):
        """New recipes for chosen envs, decided on the device: lines 197-201 of the reference's `reset()` applied to fresh graphs of
        other names on the env's current world (cooking_zoo_amd/tasks.py `host_set_tasks`).  One launch on the env's stream, no copy
        and no wait, legal inside a capture; not a step and not a reset.  d_mask uint8 [N]: env e is chosen when d_mask[e] != 0, in
        mid-episode or finished; None: every env whose record has t == 0 (the start of an episode: after `reset`, `reset_device` or
        the auto-reset pass).  d_recipe_ids uint8 [N, 4]: row e holds the new ids (indices into `book_names`; the bytes of slots >=
        num_recipes are ignored); None: row `tasks.task_draw(seed, env_id_base + e, the env's episode, K)` of d_task_list uint8 [K, 4]
        - keyed by the episode, so calling it after every step changes nothing until an env starts its next episode.  K is the list's
        leading dimension where the buffer has a shape, else `K=`.  An id past the recipe table in a used slot is refused: the env
        stays as it was, `set_tasks_refused` counts it.  Word 5 of the record and the marks change, nothing else.
        `self.recipe_ids` does NOT follow: the device owns the truth, `get_state()[:, soa.W_RECIPES]` and `infos_device(d_task=)`
        read it."""
        if K is None:
            shape = tuple(getattr(d_task_list, "shape", ()))
            K = shape[0] if shape else 0
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_set_tasks_device(self._h, p(d_mask), p(d_recipe_ids), p(d_task_list), int(K), int(seed)))

    def set_tasks_refused(self):
        """envs `set_tasks_device` left alone because a new recipe id was past the recipe table, since the env was created (waits)"""
        n = int(_native.lib().cz_set_tasks_refused(self._h))
        if n < 0:
            _native.check(self._h, 1)
        return n

    def infos_device(self, d_goal8=None, d_goal32=None, d_recipe_done=None, d_task=None, d_t=None, env_begin=0, env_count=None):
        """the task state of the current records - what the reference's `infos` and `"full"` observation report per agent
        (cooking_zoo_amd/tasks.py `host_infos`) - into device buffers, stream-ordered and capturable: `d_goal8` uint8 [n, A, num_goals]
        and / or `d_goal32` float32 [n, A, num_goals] (`goal_vector` of the agent's recipe: `torch.cat([obs32, goal32], -1)` is a
        task-conditioned policy's input), `d_recipe_done` uint8 [n, A], `d_task` int32 [n, A] (indices into `book_names`), `d_t` int32
        [n]; at least one of them.  The records are only read."""
        n = self._count(env_count)
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_infos_device(self._h, env_begin, n, p(d_goal8), p(d_goal32), p(d_recipe_done), p(d_task), p(d_t)))

    def set_tasks(self, recipes, mask=None):
        """host convenience: `recipes` - names or indices into `book_names`, [R] (every chosen env the same) or [N, R] - become the
        recipes of the envs where `mask` [N] is nonzero (None: all of them), wherever they are in their episodes; `self.recipe_ids`
        follows.  Returns how many envs were refused (an index past the table); those keep their recipes, here as on the device."""
        N, R = self.num_envs, self.num_recipes
        ids = np.full((N, 4), 0xFF, dtype=np.uint8)
        idx = self._recipe_indices(recipes, N, R)
        if ((idx < 0) | (idx > 0xFF)).any():
            raise ValueError("set_tasks: a recipe index outside 0..255")
        ids[:, :R] = idx
        chosen = np.ones(N, np.uint8) if mask is None else (np.asarray(mask).reshape(N) != 0).astype(np.uint8)
        before = self.set_tasks_refused()
        with self._scratch(((N,), np.uint8, chosen), ((N, 4), np.uint8, ids)) as (d_mask, d_ids):
            self.set_tasks_device(d_mask, d_ids)
            refused = self.set_tasks_refused() - before
        ok = (chosen != 0) & (idx < len(self.book_names)).all(axis=1)
        self.recipe_ids = self.recipe_ids.copy()
        self.recipe_ids[ok] = ids[ok]
        return refused

    def infos(self, env_begin=0, env_count=None):
        """host convenience: {"goal_vector": uint8 [n, A, num_goals], "recipe_done": uint8 [n, A], "task": int32 [n, A], "t": int32 [n]}
        of envs [env_begin, env_begin + n)"""
        n, A, G = self._count(env_count), self.num_agents, self.num_goals
        if n == 0:
            return {"goal_vector": np.zeros((0, A, G), np.uint8), "recipe_done": np.zeros((0, A), np.uint8),
                    "task": np.zeros((0, A), np.int32), "t": np.zeros((0,), np.int32)}
        with self._scratch(((n, A, G), np.uint8), ((n, A), np.uint8), ((n, A), np.int32), ((n,), np.int32)) as (d_g, d_d, d_k, d_t):
            self.infos_device(d_goal8=d_g, d_recipe_done=d_d, d_task=d_k, d_t=d_t, env_begin=env_begin, env_count=n)
            return {"goal_vector": d_g.to_host(), "recipe_done": d_d.to_host(), "task": d_k.to_host(), "t": d_t.to_host()}

    @staticmethod
    def _archive_rows(d_records, capacity):
        """rows of an archive: `capacity`, or the leading dimension of a buffer that has a shape (DeviceBuffer, torch tensor)"""
        if capacity is None:
            shape = getattr(d_records, "shape", None)
            if shape is None or len(shape) != 2:
                raise ValueError("an archive given as a raw address needs capacity=")
            capacity = shape[0]
        return int(capacity)

    def save_device(self, d_records, d_slot=None, capacity=None):
        """Records out of the batch, on the device: env e writes its whole record (`record_words` uint32, running returns included) to
        row d_slot[e] of the archive d_records, uint32 [capacity, record_words] - `alloc((capacity, record_words), np.uint32)` or a
        torch tensor; a raw address needs `capacity`.  d_slot int32 [N]: a negative slot skips the env, a slot >= capacity writes
        nothing (and is not counted); None: row e, and the archive needs N rows.  Two envs that name one row leave it unspecified.
        One launch on the env's stream, no copy and no wait, legal inside a capture; not a step; nothing of the env changes."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_save_device(self._h, p(d_slot), p(d_records), self._archive_rows(d_records, capacity)))

    def restore_device(self, d_records, d_slot=None, d_obs=None, d_obs32=None, d_codes=None, capacity=None):
        """Records into the batch, on the device: env e becomes row d_slot[e] of the archive (`save_device`), word for word - layout,
        recipes, pool slice, status with despawn bits and countdowns, episode, t, marks, running returns.  A negative slot leaves the
        env alone; None: row e.  Any number of envs may name one row: they fork it, and diverge wherever draws are made, which stay
        keyed by each env's own global id (auto-reset layouts, the on-device action stream, despawn / respawn).  A slot >= capacity
        or a row that `set_state` would reject is refused - the env and its rows stay as they were, `restore_device_refused` counts
        it.  d_obs float64 [N, A, F], d_obs32 float32 [N, A, F], d_codes uint8 [N, A, codes_pitch]: whole-batch buffers of which only
        the rows of the restored envs are written, with the observation of the restored state.  `stats()["env_steps"]` keeps counting
        the steps this env took: a running episode that is overwritten keeps its steps, one that arrives brings none; no episode is
        counted, and an episode cut short shows up in no `finished_episodes()`.  The archive must fit the layout pool it was saved
        under (a rewritten slot gives the record's own cells and objects, encoded with the slot's new descriptor row: not checked).
        One launch on the env's stream, no copy and no wait, legal inside a capture; not a step."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_restore_device(self._h, p(d_slot), p(d_records), self._archive_rows(d_records, capacity),
                                                               p(d_obs), p(d_obs32), p(d_codes)))

    def restore_device_refused(self):
        """envs `restore_device` / `fork_device` left alone (slot past the archive, or a row `set_state` would reject) since the env
        was created (waits)"""
        n = int(_native.lib().cz_restore_device_refused(self._h))
        if n < 0:
            _native.check(self._h, 1)
        return n

    def fork_device(self, d_src, d_obs=None, d_obs32=None, d_codes=None):
        """env e becomes a copy of env d_src[e] (int32 [N]; negative: e keeps its state; >= N: refused and counted) as the batch is
        when the call starts: an identity `save_device` into a scratch archive of the env's own (allocated at the first call, freed
        by `close`), then `restore_device` with d_src as the slots - two launches, so sources may be destinations as well."""
        if self._fork_buf is None:
            self._fork_buf = self.alloc((self.num_envs, self.dims.RW), np.uint32)
        self.save_device(self._fork_buf)
        self.restore_device(self._fork_buf, d_src, d_obs, d_obs32, d_codes)

    def set_compact_output(self, d_codes=None):
        """every one-step launch from now on (step_device, step_device_ring, step) also writes the compact observation to d_codes
        (uint8 [N, A, codes_pitch]); None switches it off.  Pass d_obs=None to those calls for codes only."""
        _native.check(self._h, _native.lib().cz_set_compact_output(self._h, _dev_ptr(d_codes)))

    def step_device_f32(self, d_actions, d_obs32, d_rewards, d_term, d_trunc):
        """Device-resident step whose observation is float32: d_obs32 float32 [N, A, F], contiguous (e.g. a torch.float32 tensor of
        that shape), receives np.float32 of every float64 feature bit for bit - what `obs64.float()` gives, without the float64 rows
        and the second pass.  Rewards stay float64."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_step_device_f32(self._h, p(d_actions), p(d_obs32), p(d_rewards), p(d_term), p(d_trunc)))
        self._issued(1)

    def set_f32_output(self, d_obs32=None):
        """every one-step launch from now on (step_device, step_device_ring, step) called with d_obs=None writes the float32 rows to
        d_obs32 (float32 [N, A, F]); None switches it off.  Excludes a compact output, and a float64 buffer in those calls."""
        _native.check(self._h, _native.lib().cz_set_f32_output(self._h, _dev_ptr(d_obs32)))

    def obs_table_f32(self):
        """the 256 float32 values the float32 rows are gathered from: `obs_table().astype(np.float32)`, as the device rounds them"""
        t = np.empty(256, dtype=np.float32)
        _native.check(self._h, _native.lib().cz_obs_table_f32(self._h, _ptr(t)))
        return t

    @property
    def codes_pitch(self):
        """row length of the compact observation in bytes: F rounded up to a multiple of 16 (padding bytes are 255)"""
        return int(_native.lib().cz_codes_pitch(self._h))

    def obs_table(self):
        """the 256 float64 values a compact-observation code stands for"""
        t = np.empty(256, dtype=np.float64)
        _native.check(self._h, _native.lib().cz_obs_table(self._h, _ptr(t)))
        return t

    def step_device_ring(self, K, d_ring, action_stride, action_period, first_slot, d_obs, d_rewards, d_term, d_trunc):
        """K consecutive device-resident steps in one call (cz_step_device_ring: graph replay, or fused launches after set_ring_fused); step k
        reads its actions from ring slot (first_slot + k) % action_period."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_step_device_ring(self._h, int(K), p(d_ring), int(action_stride), int(action_period),
                                                                 int(first_slot), p(d_obs), p(d_rewards), p(d_term), p(d_trunc)))
        self._issued(K)

    def rollout(self, T, seed, step0=0, d_obs=None, d_rewards=None, d_term=None, d_trunc=None):
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_rollout(self._h, int(T), int(seed), int(step0), p(d_obs), p(d_rewards),
                                                        p(d_term), p(d_trunc)))
        self._issued(T)

    def rollout_compact(self, T, seed, step0, d_codes, d_obs=None, d_rewards=None, d_term=None, d_trunc=None):
        """`rollout` with a compact trajectory: d_codes uint8 [T, N, A, codes_pitch] (and, optionally, the float64 one)"""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_rollout_compact(self._h, int(T), int(seed), int(step0), p(d_codes), p(d_obs), p(d_rewards),
                                                                p(d_term), p(d_trunc)))
        self._issued(T)

    def rollout_actions(self, d_actions, T, d_obs=None, d_rewards=None, d_term=None, d_trunc=None):
        """T fused steps over the caller's actions (device int32 [T, N, A]); every step's outputs go to the trajectory
        buffers ([T, N, A, F] / [T, N, A]).  Same results as T `step_device` calls over those rows."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_rollout_actions(self._h, int(T), p(d_actions), p(d_obs), p(d_rewards),
                                                                p(d_term), p(d_trunc)))
        self._issued(T)

    def rollout_f32(self, T, seed, step0, d_obs32, d_rewards=None, d_term=None, d_trunc=None):
        """`rollout` with the trajectory as float32: d_obs32 float32 [T, N, A, F], contiguous (e.g. a torch.float32 tensor of that
        shape), receives np.float32 of every float64 feature bit for bit - half the bytes of the float64 trajectory and no
        conversion pass behind it.  Rewards stay float64; state and statistics afterwards are those of `rollout`."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_rollout_f32(self._h, int(T), int(seed), int(step0), p(d_obs32), p(d_rewards),
                                                            p(d_term), p(d_trunc)))
        self._issued(T)

    def rollout_actions_f32(self, d_actions, T, d_obs32, d_rewards=None, d_term=None, d_trunc=None):
        """`rollout_actions` with the trajectory as float32 (d_obs32 float32 [T, N, A, F]): the same rows as T `step_device_f32` calls
        over those action rows."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_rollout_actions_f32(self._h, int(T), p(d_actions), p(d_obs32), p(d_rewards),
                                                                    p(d_term), p(d_trunc)))
        self._issued(T)

    # ------------------------------------------------------------------ the MLP policy (cooking_zoo_amd/policy.py)
    def _weight_part(self, who, role, k, v, shape):
        """the device side of `who`'s k-th weight array: a device tensor (float32) passes as it is, a numpy array is staged as `shape`
        in a buffer the env keeps by role, position and shape"""
        if hasattr(v, "data_ptr") or hasattr(v, "ptr"):
            if str(v.dtype) not in ("torch.float32", "float32"):
                raise ValueError(f"{who}: device tensors must be float32, not {v.dtype}")
            return v
        key = (role, k, shape)
        buf = self._policy_stage.get(key)
        if buf is None:
            buf = self._policy_stage[key] = self.alloc(shape, np.float32)
        buf.from_host(np.ascontiguousarray(v, np.float32).reshape(shape))
        return buf

    def load_policy(self, w1, b1, w2, b2):
        """load weight sets of `Sequential(Linear(F, 64), ReLU(), Linear(64, num_actions))` in torch's own layouts: w1 [64, F],
        b1 [64], w2 [C, 64], b2 [C], float32 - one set, or a stack of up to 4 with a leading axis.  Device tensors (anything with
        `data_ptr()`, contiguous float32: `module[0].weight` as it is) are repacked by one launch on the env's stream with no host
        trip, so a learner reloads after every optimiser step; numpy arrays go through `alloc` + `from_host` first."""
        F, Cn, H = self.F, self.num_actions, _policy.HIDDEN
        stacked = len(tuple(w1.shape)) == 3
        n = int(w1.shape[0]) if stacked else 1
        want = [(n, H, F), (n, H), (n, Cn, H), (n, Cn)]
        parts = []
        for v, shape in zip((w1, b1, w2, b2), want):
            got = tuple(int(s) for s in v.shape)
            if got != (shape if stacked else shape[1:]):
                raise ValueError(f"load_policy: shape {got}, expected {shape if stacked else shape[1:]} (F = {F}, C = {Cn})")
            parts.append(self._weight_part("load_policy", "policy", len(parts), v, shape))
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_load_policy_device(self._h, n, p(parts[0]), p(parts[1]), p(parts[2]), p(parts[3])))

    @property
    def policy_sets(self):
        """weight sets the last `load_policy` filled (0: none loaded)"""
        return int(_native.lib().cz_policy_sets(self._h))

    def load_value(self, wv, bv):
        """load the value heads of weight sets 0 .. n-1, `Linear(64, 1)` in torch's own layouts: wv [64] or `weight` [1, 64], bv [1],
        float32 - one set, or a stack of up to 4 with a leading axis (wv [n, 64] or [n, 1, 64], bv [n, 1]).  Device tensors are
        repacked by one launch on the env's stream with no host trip, like `load_policy`, which must have been called once before
        (it owns the table); numpy arrays go through `alloc` + `from_host` first."""
        H = _policy.HIDDEN
        wshape, bshape = tuple(int(s) for s in wv.shape), tuple(int(s) for s in bv.shape)
        if wshape in ((H,), (1, H)) and bshape in ((1,), ()):
            n = 1
        elif len(wshape) in (2, 3) and wshape[1:] in ((H,), (1, H)) and bshape in ((wshape[0], 1), (wshape[0],)):
            n = wshape[0]
        else:
            raise ValueError(f"load_value: shapes {wshape} and {bshape}, expected [64] / [1, 64] and [1], or stacks [n, 64] / [n, 1, 64] and [n, 1]")
        parts = [self._weight_part("load_value", "value", k, v, shape) for k, (v, shape) in enumerate(zip((wv, bv), ((n, H), (n, 1))))]
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_load_value_device(self._h, n, p(parts[0]), p(parts[1])))

    @property
    def value_sets(self):
        """weight sets whose value head the last `load_value` filled (0: none loaded)"""
        return int(_native.lib().cz_value_sets(self._h))

    def value_device(self, d_obs32, d_values, vsets=(0, 0, 0, 0), rows=None):
        """the value heads on float32 rows of the caller, one launch, stream-ordered and capturable: `d_obs32` float32 [rows, A, F]
        -> `d_values` float32 [rows, A], bit for bit `policy.host_value`.  `vsets`: agent a's value set - the weight set whose W1, b1
        and value head are used - None / 0xFF = none, that agent's entries are left untouched.  `rows` counts [A, F]-rows: None is
        the handle's N, a whole trajectory passes (T + 1) * N.  No record is read."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_value_device(self._h, self._count(rows), p(d_obs32), _policy.pack_sets(vsets, self.num_agents),
                                                             p(d_values)))

    def policy_device(self, d_obs32, d_actions=None, d_logits=None, sets=(0, 0, 0, 0), mode="greedy", seed=0, step=0, env_begin=0,
                      env_count=None):
        """the policy on float32 rows of the caller, one launch, stream-ordered and capturable: `d_obs32` float32 [n, A, F] ->
        `d_actions` int32 [n, A] and / or `d_logits` float32 [n, A, num_actions].  `sets`: agent a's weight set, None / 0xFF = none -
        that agent's entries are left untouched in both outputs (so a partner's and a learner's actions can share one array).
        `mode`: "greedy" (the smallest action with the largest logit) or "sample" (softmax sampling with the draw keyed by `seed`,
        the global env id, `step` and the agent).  No record is read or written."""
        n = self._count(env_count)
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_policy_device(self._h, env_begin, n, p(d_obs32), _policy.pack_sets(sets, self.num_agents),
                                                              _policy.MODES[mode], int(seed), int(step), p(d_actions), p(d_logits)))

    def rollout_policy(self, T, d_obs32, d_actions=None, d_logits=None, d_rewards=None, d_term=None, d_trunc=None, sets=(0, 0, 0, 0),
                       mode="greedy", seed=0, step0=0):
        """`rollout_f32` driven by the loaded policy, T policy-driven steps in one launch: agent a's action at fused step t is the
        policy's on the env's float32 row before that step (t = 0: what `observe_device(d_obs32=...)` would write now; later: row
        t - 1 of the trajectory, a reset pass's row included), the draw of "sample" keyed by step0 + t.  Agents whose set is None /
        0xFF play `rollout`'s own action stream of `seed`.  `d_obs32` float32 [T, N, A, F] is required; `d_actions` int32 [T, N, A]
        (every agent's action as played) and `d_logits` float32 [T, N, A, num_actions] (policy agents only, the rest untouched)
        are optional; rewards, flags, state, statistics and episode records are `rollout_actions_f32`'s over the same actions.
        (`rollout_policy_value` is this launch with the critic's values beside it.)"""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_rollout_policy(self._h, int(T), _policy.pack_sets(sets, self.num_agents), _policy.MODES[mode],
                                                               int(seed), int(step0), p(d_obs32), p(d_actions), p(d_logits), p(d_rewards),
                                                               p(d_term), p(d_trunc)))
        self._issued(T)

    def rollout_policy_value(self, T, d_obs32, d_values, d_actions=None, d_logits=None, d_rewards=None, d_term=None, d_trunc=None,
                             sets=(0, 0, 0, 0), vsets=None, mode="greedy", seed=0, step0=0):
        """`rollout_policy` that also evaluates the critic (`load_value`) in the same launch: `d_values` float32 [T + 1, N, A],
        required.  Row t is the value on the row the policy reads in front of step t, row T the value on the row step T - 1 left -
        what the next launch's step 0 reads - so `d_values` goes into `gae_device` as it is.  `vsets`: agent a's value set - the
        weight set whose W1, b1 and value head are used - None / 0xFF per agent = no value (entries untouched); `vsets=None` means
        "as `sets`", the shared trunk, which costs one more output row per agent and step; a set of its own is a second hidden
        pass.  Every agent of `sets` may be None as long as one has a value set: values under the action stream.  Everything else
        is bit for bit `rollout_policy` with the same arguments."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_rollout_policy_value(
            self._h, int(T), _policy.pack_sets(sets, self.num_agents), _policy.pack_sets(sets if vsets is None else vsets, self.num_agents),
            _policy.MODES[mode], int(seed), int(step0), p(d_obs32), p(d_actions), p(d_logits), p(d_values), p(d_rewards), p(d_term),
            p(d_trunc)))
        self._issued(T)

    # ------------------------------------------------------------------ what a learner trains on (cooking_zoo_amd/targets.py)
    def gae_device(self, T, d_rewards, d_term, d_trunc, d_values, d_adv=None, d_ret=None, gamma=0.99, lam=0.95, agents=None, env_count=None):
        """generalised advantage estimation over a trajectory in device memory, one launch, stream-ordered and capturable:
        `d_rewards` float64 [T, n, A], `d_term` / `d_trunc` uint8 [T, n, A] (`d_trunc` may be None) - what `rollout_policy` wrote -
        and `d_values` float32 [T + 1, n, A] - row t the critic on the state before step t, row T the bootstrap - ->
        `d_adv` and / or `d_ret` float32 [T, n, A], bit for bit `targets.host_gae`.  A termination or truncation at t cuts the
        bootstrap and the carry.  `agents`: bit a = agent a's series are computed (None: all), the others neither read nor
        written.  `env_count`: n, the caller's own extent (None: the handle's N).  No record is read."""
        n = self._count(env_count)
        mask = (1 << self.num_agents) - 1 if agents is None else int(agents)
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_gae_device(self._h, int(T), n, p(d_rewards), p(d_term), p(d_trunc), p(d_values), float(gamma),
                                                           float(lam), mask, p(d_adv), p(d_ret)))

    def logprob_device(self, d_logits, d_actions, d_logp=None, d_entropy=None, sets=(0, 0, 0, 0), rows=None):
        """the log-probability of the action played and the entropy of the distribution "sample" draws from, one launch,
        stream-ordered and capturable: `d_logits` float32 [rows, A, num_actions], `d_actions` int32 [rows, A] -> `d_logp` and / or
        `d_entropy` float32 [rows, A], bit for bit `targets.host_logprob`.  `rows` counts [A]-rows: None is the handle's N (the
        output of `policy_device`), a trajectory of `rollout_policy` passes T * N.  An action outside 0 .. num_actions - 1 gets
        logp 0.0.  `sets` as in `policy_device`: an agent at None / 0xFF is left untouched in both outputs - its logits were never
        written (the index itself plays no part).  No record is read."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_logprob_device(self._h, self._count(rows), p(d_logits), p(d_actions),
                                                               _policy.pack_sets(sets, self.num_agents), p(d_logp), p(d_entropy)))

    # ------------------------------------------------------------------ PPO's update phase (cooking_zoo_amd/ppo.py)
    def ppo_reserve(self, max_positions):
        """allocate the workspace of `ppo_grad_device` for minibatches of up to `max_positions` positions over the weight sets
        loaded now (`load_policy` first).  It allocates, so call it outside a capture; asking for no more than is reserved does
        nothing -> the positions reserved"""
        _native.check(self._h, _native.lib().cz_ppo_reserve(self._h, int(max_positions)))
        return int(_native.lib().cz_ppo_reserved(self._h))

    def ppo_grad_device(self, d_obs32, d_actions, d_logp_old, d_adv, d_ret, grads, d_index=None, sets=(0, 0, 0, 0), vsets=None, clip=0.2,
                        c_value=0.5, c_entropy=0.01, d_stats=None, rows=None):
        """the gradient of PPO's clipped-surrogate loss with value and entropy terms over a minibatch of a trajectory in device
        memory, three launches, stream-ordered and capturable, bit for bit `ppo.host_ppo_grad`: `d_obs32` float32 [rows, A, F],
        `d_actions` int32 [rows, A], `d_logp_old` / `d_adv` / `d_ret` float32 [rows, A] - what `rollout_policy_value`,
        `logprob_device` and `gae_device` wrote, flattened to rows = T * N (None: the handle's N).  `d_index` int32 [M]: the
        minibatch, position m uses row index[m] (a `torch.randperm` slice as int32; an index outside the rows is counted in
        stats[7] and otherwise ignored); None: every row once.  `sets` / `vsets`: agent a's policy and value set, None / 0xFF =
        none; `vsets=None` means "as `sets`", the shared trunk.  `grads`: six float32 buffers in torch.nn.Linear's layouts behind a
        leading axis of `policy_sets` - gw1 [n, 64, F], gb1 [n, 64], gw2 [n, C, 64], gb2 [n, C], gwv [n, 64] (or [n, 1, 64]), gbv
        [n, 1] - anything with `data_ptr()`, so a stacked parameter's `.grad`; the last two may be None when no agent has a value
        set.  Sets no agent uses get zeros.  `d_stats` float64 [8] (optional): surrogate loss, value loss, entropy, KL estimate,
        clipped fraction, policy parts, value parts, indices out of range.  Advantage normalisation is the caller's.
        `ppo_reserve` must have covered M positions."""
        n = self._count(rows)
        vs = sets if vsets is None else vsets
        if len(grads) != 6:
            raise ValueError(f"ppo_grad_device: grads holds {len(grads)} buffers, not the six of (gw1, gb1, gw2, gb2, gwv, gbv)")
        m = n if d_index is None else int(d_index.shape[0])
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_ppo_grad_device(
            self._h, n, m, p(d_index), p(d_obs32), p(d_actions), p(d_logp_old), p(d_adv), p(d_ret), _policy.pack_sets(sets, self.num_agents),
            _policy.pack_sets(vs, self.num_agents), float(clip), float(c_value), float(c_entropy), *(p(g) for g in grads), p(d_stats)))

    # ------------------------------------------------------------------ the optimiser (cooking_zoo_amd/adam.py)
    def adam_reserve(self):
        """allocate the chunk partials of `adam_step_device` (once per handle; it allocates, so call it outside a capture)"""
        _native.check(self._h, _native.lib().cz_adam_reserve(self._h))

    def adam_step_device(self, params, grads, exp_avg, exp_avg_sq, d_state, sets=None, lr=1e-3, d_lr=None, betas=(0.9, 0.999), eps=1e-8,
                         weight_decay=0.0, max_norm=0.0, keep_table=False):
        """one optimiser step on the caller's device arrays, three launches, stream-ordered and capturable, bit for bit
        `adam.host_adam_step`: global-norm clipping of the gradients to `max_norm` (0: none; `clip_grad_norm_`'s formula), then Adam,
        or AdamW with `weight_decay` != 0.  The four groups are six-sequences (w1, b1, w2, b2, wv, bv) of float32 buffers in
        torch.nn.Linear's layouts behind a leading axis of `policy_sets` - anything with `data_ptr()`, so stacked parameters, their
        `.grad` (what `ppo_grad_device` wrote) and two tensors of zeros for the moments, or `alloc` buffers; the last two entries
        may be None, in all four groups at once.  `d_state` float64 [8] on the device, `adam.fresh_state()` to begin with: steps,
        the running products of the betas, the last gradient norm and clip coefficient, calls skipped (a gradient that is not
        finite changes nothing and is counted), the learning rate used.  `sets`: the set indices that take part, None = every
        loaded set; arrays of the others are neither read nor written.  `d_lr` float64 [1] on the device replaces `lr` (a
        schedule inside a captured graph).  The masked sets of the weight table - and their value heads, when wv and bv are
        given - become the new parameters in the same launch, so no `load_policy` / `load_value` follows; `keep_table=True`
        leaves the table alone.  `adam_reserve` first."""
        groups = []
        for name, grp in (("params", params), ("grads", grads), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            grp = list(grp)
            if len(grp) != 6:
                raise ValueError(f"adam_step_device: {name} holds {len(grp)} buffers, not the six of (w1, b1, w2, b2, wv, bv)")
            groups.append(_native.CzParams(*(_address(b) for b in grp)))
        if sets is None:
            mask = (1 << max(self.policy_sets, 0)) - 1
        else:
            mask = 0
            for k in sets:
                if not 0 <= int(k) < 32:
                    raise ValueError(f"adam_step_device: set {k} is not in 0..31")
                mask |= 1 << int(k)
        b1, b2 = betas
        _native.check(self._h, _native.lib().cz_adam_step_device(
            self._h, mask, *(C.byref(g) for g in groups), _dev_ptr(d_state), float(lr), _dev_ptr(d_lr), float(b1), float(b2), float(eps),
            float(weight_decay), float(max_norm), _native.CZ_ADAM_KEEP_TABLE if keep_table else 0))

    def sync(self):
        _native.check(self._h, _native.lib().cz_sync(self._h))

    # ------------------------------------------------------------------ state / stats
    def get_state(self, env_begin=0, env_count=None):
        n = self._count(env_count)
        recs = np.empty((n, self.dims.RW), dtype=np.uint32)
        _native.check(self._h, _native.lib().cz_get_state(self._h, env_begin, n, _ptr(recs)))
        return recs

    def set_state(self, records, env_begin=0):
        recs = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, self.dims.RW)
        _native.check(self._h, _native.lib().cz_set_state(self._h, env_begin, recs.shape[0], _ptr(recs)))

    def stats(self):
        st = _native.CzStats()
        _native.check(self._h, _native.lib().cz_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def reset_stats(self):
        """zero the statistics; episodes no `collect_episodes` has reported yet are forgotten with them"""
        _native.check(self._h, _native.lib().cz_reset_stats(self._h))

    def collect_episodes(self, d_mask=None, d_return=None, d_length=None, d_flags=None, d_list=None, capacity=0, d_count=None):
        """Which envs finished an episode since the last collect - the `episode` / `_episode` entries of the reference's `infos`
        (cooking_env.py:248,264,329) for the whole batch, on the device: stream-ordered launches, no copy and no wait, legal inside a
        capture.  d_mask uint8 [N] (every byte written: 1 = finished); d_return float64 [N, A], d_length int32 [N], d_flags uint32 [N]
        (bit 0 terminated, bit 1 truncated, bit 4 + a recipe a complete): rows of envs with mask 0 stay untouched.  d_list: `capacity`
        entries of `_native.EPISODE_DTYPE` (56 bytes each), the same set packed in ascending env order, cut at `capacity`; d_count
        int32 [1]: how many envs were found, also beyond `capacity`.  Everything is optional; every env found is marked seen, so a call
        without buffers just marks.  An env that finished several episodes since the last collect reports the last one (`finished` in
        the list says how many).  Buffers as in `step_device`."""
        p = _dev_ptr
        _native.check(self._h, _native.lib().cz_episodes_collect(self._h, p(d_mask), p(d_return), p(d_length), p(d_flags), p(d_list),
                                                                 int(capacity) if d_list is not None else 0, p(d_count)))

    def finished_episodes(self):
        """host convenience: `collect_episodes` into buffers the env owns, a wait, and the episodes found as a numpy structured array
        (`_native.EPISODE_DTYPE`: env - the GLOBAL id -, episode, length, flags, finished, ret[4]) in env order"""
        if self._ep_bufs is None:
            self._ep_bufs = (self.alloc((self.num_envs,), _native.EPISODE_DTYPE), self.alloc((1,), np.int32))
        d_list, d_count = self._ep_bufs
        self.collect_episodes(d_list=d_list, capacity=self.num_envs, d_count=d_count)
        n = int(d_count.to_host()[0])                          # (cz_memcpy_d2h waits for the stream)
        out = np.empty(n, dtype=np.dtype(_native.EPISODE_DTYPE))
        if n:
            _native.check(self._h, _native.lib().cz_memcpy_d2h(self._h, _ptr(out), d_list.ptr, out.nbytes))
        return out

    def close(self):
        if getattr(self, "_rot", None) is not None:
            self.stop_rotation()
        if getattr(self, "_h", None):
            for b in self._buffers:
                b.free()
            for p, _ in self._pin_bufs.values():
                _native.lib().cz_host_free(self._h, p)
            self._pin_bufs = {}
            _native.lib().cz_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
