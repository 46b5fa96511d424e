#!/usr/bin/env python3
"""Golden data of the scripted partner, from the unmodified reference: tests/golden/partner_ref.json.gz.

Replays tools/gen_golden.py style seeded episodes on coop_test, switch_test (scheme1 and scheme3), crowded_6x5 and dense_8x8 under
bumper / heuristic / mixed policies and stores, at chosen steps, the record (`gen_golden.world_to_record`), and what a FRESH,
unmodified `CookingAgent(recipe, name).step(obs)` (cooking_agents/cooking_agent.py) returns for every agent and a set of recipe
names; `obs` is the reference's live objects (`world.world_objects` plus the agents, what gen_golden.Heuristic hands its agent).
Per answer: [agent, recipe index in RECIPE_NAMES, action, walk calls, x, y of the last `walk_to_location` argument or -1, -1]
(the bound method is wrapped), or, where the reference raises, [agent, recipe index, the exception's class name].  Per episode:
the static lists (cells per static class in `world_objects[class]` list order, Floor included), which the record does not hold.

Every agent is asked for its own recipe and for every other name of RECIPE_NAMES whose leaf classes all have a live object in that
state, plus one name per state that does not (it pins RAISES).  A state is stored at steps 0, 1, 2 and at every step that is a
multiple of 5 or two more than a multiple of 9, at most PER_EPISODE per episode.  The tool asserts, and prints, a census (see `main`); the branches
are counted through the host model's own tags (cooking_zoo_amd/partner.py) on the same records, and the host model is asserted
against every stored answer.  Data only; runs in the build container (needs the reference), never on the test machines.

Usage: python tools/gen_partner_golden.py [--out tests/golden/partner_ref.json.gz]"""
from __future__ import annotations

import argparse
import gzip
import json
import os
import random
import sys
from collections import Counter, defaultdict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (puts the reference and the repository on sys.path)

from cooking_zoo.cooking_agents.cooking_agent import CookingAgent  # noqa: E402
from cooking_zoo.cooking_book.recipe_drawer import RECIPES as REF_RECIPES  # noqa: E402
from cooking_zoo_amd import partner, soa  # noqa: E402
from cooking_zoo_amd.cooking_book import recipe_drawer  # noqa: E402
from cooking_zoo_amd.cooking_world.layout import Layout  # noqa: E402

PER_EPISODE = 60
BRANCHES = ("on_appliance", "held_to_appliance", "held_to_counter", "drop_held", "fetch", "wait_appliance")


def leaf_classes(name):
    return {n.name for n in REF_RECIPES[name]().node_list if not n.contains}


def ask_reference(obs, recipe, agent_name):
    """(action, walk calls, last walk argument) of a fresh CookingAgent, or the exception's class name"""
    ag = CookingAgent(recipe, agent_name)
    calls = []
    walk = ag.walk_to_location

    def wrapped(location, observation):
        calls.append(location)
        return walk(location, observation)

    ag.walk_to_location = wrapped
    try:
        action = int(ag.step(obs))
    except Exception as e:                                              # noqa: BLE001 - the class name is the datum
        return type(e).__name__
    last = calls[-1] if calls else None
    return action, len(calls), (-1, -1) if last is None else (int(last[0]), int(last[1]))


def live_static_lists(world):
    out = {}
    for k, lst in world.world_objects.items():
        if k in soa.STATIC_CLASSES and lst:
            out[k] = [int(o.location[1]) * world.width + int(o.location[0]) for o in lst]
    return out


def replay(cfg, seed, policy_name, max_len, census):
    random.seed(seed)
    np.random.seed(seed)
    rng = np.random.default_rng(seed + 7919)
    env = gg.CookingEnvironment(level=cfg["level"], meta_file=cfg["meta_file"], num_agents=cfg["num_agents"], max_steps=cfg["max_steps"],
                                recipes=cfg["recipes"], obs_spaces=["feature_vector"] * cfg["num_agents"],
                                end_condition_all_dishes=cfg["end_condition_all_dishes"], action_scheme=cfg["action_scheme"],
                                reward_scheme=cfg.get("reward_scheme"))
    env.reset()
    world, A, scheme = env.world, cfg["num_agents"], cfg["action_scheme"]
    W, H = world.width, world.height
    dims = soa.Dims(W, H, cfg["max_dyn"], A, env.feature_vector_representation_length)
    slotmap = gg.SlotMap(world, cfg["max_dyn"])
    recipe_ids = [gg.RECIPE_NAMES.index(r) for r in cfg["recipes"]]
    pols = []
    for i in range(A):
        kind = policy_name if policy_name != "mixed" else ("heuristic" if i % 2 == 0 else "bumper")
        pols.append(gg.Bumper(rng, scheme) if kind == "bumper" else gg.Heuristic(rng, cfg["recipes"][i], f"agent-{i + 1}", eps=0.2))
    level = os.path.basename(cfg["level"]).replace(".json", "")
    lists = live_static_lists(world)
    layout = Layout(W, H, np.zeros(W * H, np.uint8), lists, [], [], [])
    ascending = Layout(W, H, np.zeros(W * H, np.uint8), {k: sorted(v) for k, v in lists.items()}, [], [], [])
    states = []

    def look(step):
        if len(states) >= PER_EPISODE or not (step <= 2 or step % 9 == 2 or step % 5 == 0):
            return
        assert live_static_lists(world) == lists, "a static list changed inside an episode"
        record = gg.world_to_record(env, dims, slotmap, 0, recipe_ids)
        obs = defaultdict(list)
        obs.update(world.world_objects)
        obs["Agent"] = world.agents
        alive = {k for k, v in world.world_objects.items() if v}
        full = [n for n in gg.RECIPE_NAMES if leaf_classes(n) <= alive]
        lacking = [n for n in gg.RECIPE_NAMES if n not in full]
        answers = []
        for i, ag in enumerate(world.agents):
            names = list(dict.fromkeys([cfg["recipes"][i]] + full + lacking[(step + i) % max(len(lacking), 1):][:1]))
            for name in names:
                ref = ask_reference(obs, name, ag.name)
                r = gg.RECIPE_NAMES.index(name)
                mine = partner.agent_answer(dims, layout, record, recipe_drawer.RECIPES[name](), i)
                ctx = f"{level} seed {seed} step {step} agent {i} {name}: reference {ref}, host model {mine}"
                if isinstance(ref, str):
                    assert mine.status == partner.RAISES and mine.tags[-1] == ref, ctx
                    answers.append([i, r, ref])
                    census["raise"][ref] += 1
                else:
                    action, walks, last = ref
                    assert mine.status != partner.RAISES and mine.action == action and mine.walks == walks, ctx
                    assert (mine.last_walk or (-1, -1)) == last and (mine.status != partner.WALK or mine.target == last), ctx
                    answers.append([i, r, action, walks, last[0], last[1]])
                    census["action"][action] += 1
                    census["walks"][walks] += 1
                census["status"][partner.STATUS_NAMES[mine.status]] += 1
                for t in mine.tags:
                    census["tag"][t] += 1
                if any(sorted(v) != v for v in lists.values()) and mine.status == partner.WALK:
                    other = partner.agent_answer(dims, ascending, record, recipe_drawer.RECIPES[name](), i)
                    census["list_order_decides"] += (other.action, other.target) != (mine.action, mine.target)
        states.append({"step": step, "record": record.tolist(), "answers": answers})

    look(0)
    for step in range(max_len):
        env.accumulated_step([p.act(world, i) for i, p in enumerate(pols)])
        look(step + 1)
        if any(env.terminations.values()) or any(env.truncations.values()):
            break
    return {"level": level, "seed": seed, "policy": policy_name, "scheme": scheme, "dims": list(dims.as_tuple()), "recipes": cfg["recipes"],
            "static_lists": lists, "states": states}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(gg.REPO, "tests", "golden", "partner_ref.json.gz"))
    args = ap.parse_args()
    own = lambda stem: (os.path.join(gg.REPO, "cooking_zoo_amd", "utils", "level", stem + ".json"),
                        os.path.join(gg.REPO, "cooking_zoo_amd", "utils", "meta_files", stem + ".json"))
    crowd, metac = own("crowded_6x5")
    dense, metad = own("dense_8x8")
    coop = lambda r: gg.base_cfg("coop_test", 2, r)
    plan = [
        ("coop_heuristic", coop(["TomatoLettuceSalad", "CarrotBanana"]), 11, "heuristic", 200),
        ("coop_mixed", coop(["MashedCarrotBanana", "TomatoLettuceSalad"]), 12, "mixed", 200),
        ("coop_bumper", coop(["TomatoLettuceSalad", "CarrotBanana"]), 13, "bumper", 300),
        ("coop_heuristic_mashed", coop(["CarrotBanana", "MashedCarrotBanana"]), 14, "heuristic", 200),
        ("switch_scheme1", gg.base_cfg("switch_test", 2, ["MashedCarrotBanana", "TomatoSalad"], scheme="scheme1", max_steps=300), 80, "bumper", 300),
        ("switch_scheme3", gg.base_cfg("switch_test", 2, ["TomatoLettuceSalad", "CarrotBanana"], max_steps=300), 40, "mixed", 300),
        ("switch_heuristic", gg.base_cfg("switch_test", 2, ["TomatoSalad", "CarrotBanana"], max_steps=300), 41, "heuristic", 200),
        ("crowded_mixed", gg.base_cfg(crowd, 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], max_steps=200, meta=metac),
         122, "mixed", 200),
        ("crowded_bumper", gg.base_cfg(crowd, 4, ["TomatoSalad", "TomatoLettuceSalad", "no_recipe", "MashedCarrotBanana"], max_steps=200, meta=metac),
         123, "bumper", 200),
        ("dense8_mixed", gg.base_cfg(dense, 4, ["TomatoSalad", "no_recipe", "TomatoLettuceSalad", "CarrotBanana"], max_steps=120, meta=metad),
         1200, "mixed", 120),
        ("dense8_bumper", gg.base_cfg(dense, 4, ["TomatoSalad", "no_recipe", "TomatoLettuceSalad", "CarrotBanana"], max_steps=120, meta=metad),
         1201, "bumper", 120),
    ]
    census = dict(action=Counter(), walks=Counter(), status=Counter(), tag=Counter(), list_order_decides=0)
    census["raise"] = Counter()
    episodes = []
    for name, cfg, seed, policy, steps in plan:
        ep = replay(cfg, seed, policy, steps, census)
        ep["set"] = name
        episodes.append(ep)
        print(f"{name} seed {seed} {policy}: {len(ep['states'])} states at steps {[s['step'] for s in ep['states']]}, "
              f"{sum(len(s['answers']) for s in ep['states'])} answers")
    total = sum(census["status"].values())
    print(f"{total} answers; by action code: {dict(sorted(census['action'].items()))}; by walk calls: {dict(sorted(census['walks'].items()))}; "
          f"by status: {dict(census['status'])}; raises: {dict(census['raise'])}; branches: {dict(census['tag'])}; "
          f"answers the static list order decides (they change when every list is sorted by cell): {census['list_order_decides']}")
    assert all(census["action"][c] > 0 for c in range(5)), "an action code never occurs"
    assert all(census["status"][s] > 0 for s in ("DONE", "WALK", "IDLE", "RAISES")), "a status never occurs"
    assert census["raise"]["IndexError"] > 0 and census["raise"]["TypeError"] > 0, "a raise site never occurs"
    assert all(census["tag"][t] > 0 for t in BRANCHES), f"a branch of generic_sequence never occurs: {[t for t in BRANCHES if not census['tag'][t]]}"
    assert all(census["tag"][t] > 0 for t in ("child_held", "child_in_held_plate", "on_appliance", "to_child", "to_main", "no_child")), "object places"
    assert census["list_order_decides"] > 0, "no tie decided by static list order on a list that is not ascending"
    assert 3 * sum(census["raise"].values()) <= total, "more than one third of the stored answers are raises"
    doc = {"recipe_names": gg.RECIPE_NAMES, "answer": "[agent, recipe, action, walk calls, last walk x, y] or [agent, recipe, exception]",
           "episodes": episodes}
    with gzip.GzipFile(args.out, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {sum(len(e['states']) for e in episodes)} states")


if __name__ == "__main__":
    main()
