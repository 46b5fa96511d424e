#!/usr/bin/env python3
"""Golden data of the task calls, from the unmodified reference: tests/golden/tasks_ref.json.gz.

Three parts, all computed by the reference's own `Recipe.update_recipe_state` / `goals_completed` / `accumulated_step`:

  * states: seeded episodes on coop_test, switch_test, crowded_6x5 and dense_8x8 under the heuristic and bumper policies of
    tools/gen_partner_golden.py are replayed; at chosen steps the record (`gen_golden.world_to_record`) is stored and, for EVERY
    recipe name of the default book on a fresh `RECIPES[name]()`, the node marks after `update_recipe_state(world)` (bit j = node
    j of node_list) and `goals_completed(26)`; one more coop_test episode is SCRIPTED (`MashScript`), because neither of those
    policies ever takes a mashed object out of the Blender: the left agent hands the Carrot over the dividing counter, the right one
    mashes Carrot and Banana, plates and delivers them - MashedCarrotBanana's plate and root marked;
  * switches: at step k of an episode fresh graphs of OTHER names are assigned to `env.recipe_graphs`, `env.recipe_mapping` and
    `env.recipe_names`, lines 197-198 of the reference's `reset()` are run on them (no reference code is edited), and the episode is
    played on.  Stored: the record right before and right after the switch, and for every later step the actions, rewards,
    terminations, truncations, `infos[agent]["recipe_done"]` / `["task"]` and `recipe_mapping[agent].goals_completed(num_goals)`,
    the expression the `"full"` observation returns as `goal_vector` (cooking_env.py:277; the `goal_vector` of the infos is another
    thing, a one-hot over the env's loaded recipes, cooking_env.py:161);
  * shared_id: a hand-built user recipe in which two different nodes carry one id_num, evaluated on stored states in which the earlier
    node is marked and the later one is not, with the reference's `goals_completed`.

The tool asserts and stores a census: every node of every recipe that one of the chosen levels can complete is seen marked and
unmarked, at least one root is marked, every info key is present, one switch lands where a node of the new recipe is already satisfied,
one switched trajectory completes its new recipe.  Data only; runs in the build container (needs the reference), never on the test
machines.

Usage: python tools/gen_tasks_golden.py [--out tests/golden/tasks_ref.json.gz]"""
from __future__ import annotations

import argparse
import gzip
import json
import os
import random
import sys
from collections import defaultdict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (puts the reference and the repository on sys.path)
import gen_partner_golden as gp  # noqa: E402

from cooking_zoo.cooking_book.recipe import Recipe as RefRecipe, RecipeNode as RefNode  # noqa: E402
from cooking_zoo.cooking_book.recipe_drawer import RECIPES as REF_RECIPES  # noqa: E402
from cooking_zoo.cooking_world.constants import ChopFoodStates  # noqa: E402
from cooking_zoo_amd import soa  # noqa: E402

NUM_GOALS = 26
PER_EPISODE = 14
INFO_KEYS = ("recipe_done", "task", "t", "goal_vector", "action", "termination_info")


def marks_of(graph):
    return sum(1 << j for j, n in enumerate(graph.node_list) if n.marked)


def evaluate_all(world):
    """per name of RECIPE_NAMES: (marks, goals) of a fresh graph on `world`"""
    marks, goals = [], []
    for name in gg.RECIPE_NAMES:
        g = REF_RECIPES[name]()
        g.update_recipe_state(world)
        marks.append(marks_of(g))
        goals.append([int(v) for v in g.goals_completed(NUM_GOALS)])
    return marks, goals


def shared_id_recipe():
    """Deliversquare(0) > Plate(1) > [Tomato chopped (2), Lettuce chopped (2)]: the two leaves share goal id 2"""
    chopped = ("chop_state", ChopFoodStates.CHOPPED)
    tomato = RefNode(root_type="Tomato", id_num=2, name="Tomato", conditions=[chopped])
    lettuce = RefNode(root_type="Lettuce", id_num=2, name="Lettuce", conditions=[chopped])
    plate = RefNode(root_type="Plate", id_num=1, name="Plate", contains=[tomato, lettuce])
    root = RefNode(root_type="Deliversquare", id_num=0, name="Deliversquare", contains=[plate])
    return RefRecipe(root, 3)


SHARED_NODES = [["Deliversquare", 0, [], [1]], ["Plate", 1, [], [2, 3]], ["Tomato", 2, [["chop_state", "CHOPPED"]], []],
                ["Lettuce", 2, [["chop_state", "CHOPPED"]], []]]        # name, id_num, conditions, children (node_list indices)


def make_env(cfg, seed):
    random.seed(seed)
    np.random.seed(seed)
    env = gg.CookingEnvironment(level=cfg["level"], meta_file=cfg["meta_file"], num_agents=cfg["num_agents"], max_steps=cfg["max_steps"],
                                recipes=cfg["recipes"], obs_spaces=["feature_vector"] * cfg["num_agents"],
                                end_condition_all_dishes=cfg["end_condition_all_dishes"], action_scheme=cfg["action_scheme"],
                                reward_scheme=cfg.get("reward_scheme"))
    env.reset()
    return env


def policies(cfg, names, policy_name, rng):
    out = []
    for i in range(cfg["num_agents"]):
        kind = policy_name if policy_name != "mixed" else ("heuristic" if i % 2 == 0 else "bumper")
        out.append(gg.Bumper(rng, cfg["action_scheme"]) if kind == "bumper" else gg.Heuristic(rng, names[i], f"agent-{i + 1}", eps=0.2))
    return out


class MashScript:
    """coop_test is two rooms with a row of counters between them: the Carrot lies in the left one, Blender, Banana and a Plate in the
    right one.  Phases of (agent, where it walks - `walk_to_location` of the reference's own agent, whose last move into an object is
    the interaction -, until what holds); the other agent stands still.  A Blender that holds an unmashed object is toggled by the
    move into it and switches itself off when the object is MASHED; then the same move takes the object out."""
    HATCH, DELIVER = (3, 2), (4, 0)

    def __init__(self, env):
        from cooking_zoo.cooking_world.constants import BlenderFoodStates
        w = self.world = env.world
        self.agents = [gg.CookingAgent("MashedCarrotBanana", a.name) for a in w.agents]
        left, right = w.agents
        one = lambda name: w.world_objects[name][0]
        plate = [p for p in w.world_objects["Plate"] if p.location[0] > 3][0]
        blender = lambda: one("Blender").location
        mashed = lambda food: one(food).blend_state == BlenderFoodStates.MASHED

        def mash(food):
            return [(1, blender, lambda: right.holding is None), (1, blender, lambda: one("Blender").toggle or mashed(food)),
                    (1, None, lambda: mashed(food)), (1, blender, lambda: right.holding is one(food)),
                    (1, lambda: plate.location, lambda: right.holding is None)]

        self.phases = ([(0, lambda: one("Carrot").location, lambda: left.holding is one("Carrot")),
                        (0, lambda: self.HATCH, lambda: left.holding is None),
                        (1, lambda: self.HATCH, lambda: right.holding is one("Carrot"))] + mash("Carrot") +
                       [(1, lambda: one("Banana").location, lambda: right.holding is one("Banana"))] + mash("Banana") +
                       [(1, lambda: plate.location, lambda: right.holding is plate),
                        (1, lambda: self.DELIVER, lambda: env.recipe_graphs[0].completed())])

    def acts(self):
        while self.phases and self.phases[0][2]():
            self.phases.pop(0)
        act = [0] * len(self.agents)
        if self.phases and self.phases[0][1] is not None:
            who, where, _ = self.phases[0]
            obs = defaultdict(list)
            obs.update(self.world.world_objects)
            obs["Agent"] = self.world.agents
            self.agents[who].update_location(obs)
            act[who] = int(self.agents[who].walk_to_location(where(), obs))
        return act


def episode_head(env, cfg, name, seed, policy_name):
    world = env.world
    dims = soa.Dims(world.width, world.height, cfg["max_dyn"], cfg["num_agents"], env.feature_vector_representation_length)
    level = os.path.basename(cfg["level"]).replace(".json", "")
    return dims, {"set": name, "level": level, "seed": seed, "policy": policy_name, "scheme": cfg["action_scheme"], "dims": list(dims.as_tuple()),
                  "recipes": cfg["recipes"], "static_lists": gp.live_static_lists(world)}


def note(census, level_can, marks):
    for r, m in enumerate(marks):
        if gg.RECIPE_NAMES[r] in level_can:
            n = len(REF_RECIPES[gg.RECIPE_NAMES[r]]().node_list)
            for j in range(n):
                census["seen"][(r, j, bool(m >> j & 1))] += 1


def replay_states(name, cfg, seed, policy_name, max_len, census, shared):
    env = make_env(cfg, seed)
    rng = np.random.default_rng(seed + 7919)
    world = env.world
    dims, ep = episode_head(env, cfg, name, seed, policy_name)
    slotmap = gg.SlotMap(world, cfg["max_dyn"])
    ids = [gg.RECIPE_NAMES.index(r) for r in cfg["recipes"]]
    script = MashScript(env) if policy_name == "scripted" else None
    pols = [] if script else policies(cfg, cfg["recipes"], policy_name, rng)
    alive = {k for k, v in world.world_objects.items() if v}
    # (no_recipe is a Deliversquare that contains a Floor: no level can complete it, its leaf is marked in every state)
    level_can = {n for n in gg.RECIPE_NAMES if n != "no_recipe" and gp.leaf_classes(n) <= alive}
    census["completable"][ep["level"]] = sorted(level_can)
    states, last = [], [None]

    def look(step, force=False):
        marks, goals = evaluate_all(world)
        force = force or (script is not None and marks != last[0])       # the scripted episode: every state in which a mark changed
        last[0] = marks
        note(census, level_can, marks)
        own = [marks_of(g) for g in env.recipe_graphs]
        assert own == [marks[i] for i in ids], "a fresh graph disagrees with the env's own"
        g = shared_id_recipe()
        g.update_recipe_state(world)
        m = marks_of(g)
        wanted = (m >> 2 & 1) and not (m >> 3 & 1) and len(shared) < 3            # the earlier node marked, the later one not
        if not (force or wanted or (len(states) < PER_EPISODE and (step <= 1 or step % 13 == 0 or any(mm & 1 for mm in marks)))):
            return
        record = gg.world_to_record(env, dims, slotmap, 0, ids)
        states.append({"step": step, "record": record.tolist(), "marks": marks, "goals": goals})
        if wanted:
            shared.append({"episode": len(census["episodes"]), "state": len(states) - 1, "marks": m,
                           "goals": [int(v) for v in g.goals_completed(3)]})

    look(0)
    for step in range(max_len):
        env.accumulated_step(script.acts() if script else [p.act(world, i) for i, p in enumerate(pols)])
        done = any(env.terminations.values()) or any(env.truncations.values())
        look(step + 1, force=done)
        if done:
            break
    ep["states"] = states
    census["episodes"].append(name)
    return ep


def replay_switch(name, cfg, seed, policy_name, k, new_names, after_policy, max_len, census):
    env = make_env(cfg, seed)
    rng = np.random.default_rng(seed + 7919)
    world, A = env.world, cfg["num_agents"]
    dims, ep = episode_head(env, cfg, name, seed, policy_name)
    slotmap = gg.SlotMap(world, cfg["max_dyn"])
    old_ids, new_ids = [gg.RECIPE_NAMES.index(r) for r in cfg["recipes"]], [gg.RECIPE_NAMES.index(r) for r in new_names]
    ep.update(initial_record=gg.world_to_record(env, dims, slotmap, 0, old_ids).tolist(), class_order=slotmap.class_order,
              statics=gg.static_lists(env), max_steps=cfg["max_steps"], all_dishes=bool(cfg["end_condition_all_dishes"]),
              meta=os.path.basename(cfg["meta_file"]).replace(".json", ""), switch_step=k, new_recipes=new_names)
    pols = policies(cfg, cfg["recipes"], policy_name, rng)
    for _ in range(k):
        env.accumulated_step([p.act(world, i) for i, p in enumerate(pols)])
        assert not (any(env.terminations.values()) or any(env.truncations.values())), f"{name}: the episode ended before step {k}"
    ep["record_before"] = gg.world_to_record(env, dims, slotmap, 0, old_ids).tolist()
    # ---- the switch: fresh graphs of other names, then reset()'s own lines 197-198 and 201 on them
    env.recipe_graphs = [REF_RECIPES[n]() for n in new_names]
    env.recipe_names = list(new_names)
    for recipe in env.recipe_graphs:
        recipe.update_recipe_state(env.world)
    env.recipe_mapping = dict(zip(env.possible_agents, env.recipe_graphs))
    ep["record_after"] = gg.world_to_record(env, dims, slotmap, 0, new_ids).tolist()
    ep["marks_after"] = [marks_of(g) for g in env.recipe_graphs]
    census["switch_presatisfied"] += int(any(ep["marks_after"]))
    pols = policies(cfg, new_names, after_policy, rng)
    steps = []
    for _ in range(max_len):
        act = [p.act(world, i) for i, p in enumerate(pols)]
        env.accumulated_step(act)
        agents = env.possible_agents
        for a in agents:
            for key in INFO_KEYS:
                assert key in env.infos[a], f"{name}: infos[{a}] lacks {key!r}"
                census["info_keys"][key] += 1
        goal = [[int(v) for v in env.recipe_mapping[a].goals_completed(env.num_goals)] for a in agents[:A]]
        steps.append({"actions": [int(x) for x in act], "rewards": [float(env.rewards[a]).hex() for a in agents],
                      "terms": [int(bool(env.terminations[a])) for a in agents], "truncs": [int(bool(env.truncations[a])) for a in agents],
                      "recipe_done": [int(bool(env.infos[a]["recipe_done"])) for a in agents],
                      "task": [gg.RECIPE_NAMES.index(env.infos[a]["task"]) for a in agents], "goal_vector": goal,
                      "record": gg.world_to_record(env, dims, slotmap, 0, new_ids).tolist()})
        if any(steps[-1]["recipe_done"]):
            census["switch_completed"] += 1
        if any(steps[-1]["terms"]) or any(steps[-1]["truncs"]):
            break
    assert env.num_goals == NUM_GOALS
    ep["steps"] = steps
    return ep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(gg.REPO, "tests", "golden", "tasks_ref.json.gz"))
    args = ap.parse_args()
    own = lambda stem: (os.path.join(gg.REPO, "cooking_zoo_amd", "utils", "level", stem + ".json"),
                        os.path.join(gg.REPO, "cooking_zoo_amd", "utils", "meta_files", stem + ".json"))
    crowd, metac = own("crowded_6x5")
    dense, metad = own("dense_8x8")
    coop = lambda r, **kw: gg.base_cfg("coop_test", 2, r, **kw)
    switch = lambda r, **kw: gg.base_cfg("switch_test", 2, r, max_steps=300, **kw)
    crowded = lambda r: gg.base_cfg(crowd, 4, r, max_steps=200, meta=metac)
    dense8 = lambda r: gg.base_cfg(dense, 4, r, max_steps=120, meta=metad)
    # all dishes end the episode in the heuristic sets, so that an episode goes on after its first completion
    plan = [
        ("coop_heuristic", coop(["TomatoLettuceSalad", "CarrotBanana"], all_dishes=True), 11, "heuristic", 250),
        ("coop_heuristic_mashed", coop(["MashedCarrotBanana", "TomatoSalad"], all_dishes=True), 14, "heuristic", 250),
        ("coop_heuristic_apple", coop(["AppleWatermelon", "AppleWatermelon"], all_dishes=True), 30, "heuristic", 100),
        ("coop_heuristic_mashed_apple", coop(["MashedCarrotBanana", "AppleWatermelon"], all_dishes=True), 34, "heuristic", 120),
        ("coop_bumper", coop(["TomatoLettuceSalad", "CarrotBanana"]), 13, "bumper", 200),
        ("switch_heuristic", switch(["TomatoSalad", "CarrotBanana"], all_dishes=True), 41, "heuristic", 200),
        ("switch_bumper", switch(["MashedCarrotBanana", "TomatoSalad"], scheme="scheme1"), 80, "bumper", 200),
        ("crowded_mixed", crowded(["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"]), 122, "mixed", 200),
        ("crowded_bumper", crowded(["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"]), 123, "bumper", 120),
        ("dense8_mixed", dense8(["TomatoSalad", "no_recipe", "TomatoLettuceSalad", "CarrotBanana"]), 1200, "mixed", 120),
        ("dense8_bumper", dense8(["TomatoSalad", "no_recipe", "TomatoLettuceSalad", "CarrotBanana"]), 1201, "bumper", 120),
        ("coop_scripted_mashed", coop(["MashedCarrotBanana", "TomatoSalad"]), 31, "scripted", 100),
    ]
    census = dict(seen=defaultdict(int), completable={}, episodes=[], switch_presatisfied=0, switch_completed=0, info_keys=defaultdict(int))
    shared, episodes = [], []
    for name, cfg, seed, policy, steps in plan:
        ep = replay_states(name, cfg, seed, policy, steps, census, shared)
        episodes.append(ep)
        print(f"{name} seed {seed} {policy}: {len(ep['states'])} states at steps {[s['step'] for s in ep['states']]}")
    switches = [
        # the tomato is chopped (and more) when TomatoSalad takes over: a node of the new recipe is already satisfied
        replay_switch("coop_switch_late", coop(["TomatoLettuceSalad", "CarrotBanana"], all_dishes=True), 11, "heuristic", 40,
                      ["TomatoSalad", "MashedCarrotBanana"], "heuristic", 200, census),
        replay_switch("coop_switch_early", coop(["CarrotBanana", "TomatoSalad"]), 21, "heuristic", 3,
                      ["TomatoLettuceSalad", "CarrotBanana"], "heuristic", 200, census),
        replay_switch("switch_switch", switch(["TomatoSalad", "CarrotBanana"], scheme="scheme1"), 43, "bumper", 25,
                      ["CarrotBanana", "TomatoLettuceSalad"], "bumper", 60, census),
        replay_switch("crowded_switch", crowded(["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"]), 124, "mixed", 30,
                      ["TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana", "TomatoSalad"], "mixed", 80, census),
    ]
    for ep in switches:
        print(f"{ep['set']}: switch at step {ep['switch_step']} to {ep['new_recipes']}, marks after the switch {ep['marks_after']}, "
              f"{len(ep['steps'])} steps, recipe_done at the end {ep['steps'][-1]['recipe_done']}")
    # ---- census
    can = sorted({n for names in census["completable"].values() for n in names})
    missing = [(gg.RECIPE_NAMES[r], j, m) for r, name in enumerate(gg.RECIPE_NAMES) if name in can
               for j in range(len(REF_RECIPES[name]().node_list)) for m in (False, True)
               if not census["seen"][(r, j, m)]]
    print(f"recipes a chosen level can complete: {can}; node states never seen: {missing}")
    assert not missing, "a node of a completable recipe is never seen marked / unmarked"
    roots = sum(v for (r, j, m), v in census["seen"].items() if j == 0 and m)
    assert roots > 0, "no root is ever marked"
    assert all(census["info_keys"][k] > 0 for k in INFO_KEYS), "an info key never occurs"
    assert census["switch_presatisfied"] > 0, "no switch lands where a node of the new recipe is already satisfied"
    assert census["switch_completed"] > 0, "no switched trajectory completes its new recipe"
    assert shared, "no state with the earlier shared-id node marked and the later one not"
    stored = {"completable": census["completable"], "roots_marked": roots, "info_keys": dict(census["info_keys"]),
              "switch_presatisfied": census["switch_presatisfied"], "switch_completed": census["switch_completed"],
              "seen": {f"{gg.RECIPE_NAMES[r]}:{j}:{int(m)}": v for (r, j, m), v in sorted(census["seen"].items())}}
    doc = {"recipe_names": gg.RECIPE_NAMES, "num_goals": NUM_GOALS, "episodes": episodes, "switches": switches,
           "shared_id": {"nodes": SHARED_NODES, "num_goals": 3, "states": shared}, "census": stored}
    with gzip.GzipFile(args.out, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {sum(len(e['states']) for e in episodes)} states, "
          f"{sum(len(e['steps']) for e in switches)} switched steps")


if __name__ == "__main__":
    main()
