"""User recipes (recipe_drawer.register_recipe; reference recipe_drawer.py:19-35, cooking_env.py:100-105): graphs with more
than 8 nodes (wide tables: 16 nodes, marks in record words 1 and 7) and nodes with several conditions (recipe.py:96-98),
pinned by traces captured from the reference with the same recipes registered there (tests/golden/custom_wide_*.npz;
oracle replay in test_oracle_golden.py, device replay in test_gpu_parity.py)."""
import random

import numpy as np
import pytest

from cooking_zoo_amd import soa
from cooking_zoo_amd.cooking_book import recipe_drawer as rd
from cooking_zoo_amd.cooking_book.recipe import Recipe, RecipeNode
from golden_io import GoldenSet
from host_common import register_fixture_recipes


@pytest.fixture
def user_recipes():
    assert not rd.RECIPE_STORE
    register_fixture_recipes()
    yield
    rd.RECIPE_STORE.clear()


def test_host_mirror_flattens_to_the_tables_the_reference_graphs_give(user_recipes):
    gs = GoldenSet("custom_wide_coop")
    names = list(rd.RECIPE_STORE.keys())
    assert names == gs.cfg["recipe_store"]
    graphs = [rd.RECIPE_STORE[n]() for n in names]
    assert [len(g.node_list) for g in graphs] == [10, 3, 3]
    table = np.stack([g.flatten(soa.MAX_NODES) for g in graphs])
    assert np.array_equal(table, gs.recipe_table)
    # the two-condition node: chopped and not mashed = object state 1 only (accept mask 0b0010)
    banana = graphs[1].node_list[2]
    assert banana.name == "Banana" and len(banana.conditions) == 2
    assert (int(table[1][1 + 2 * 2]) >> 8) & 0xFF == 0x10 | 0x2
    with pytest.raises(ValueError, match="10 nodes"):
        graphs[0].flatten(soa.NARROW_NODES)
    # small graphs keep the compact rows
    assert graphs[1].flatten().shape == (9,)


def test_graphs_beyond_sixteen_nodes_are_refused():
    kids = [RecipeNode("Tomato", 0, "Tomato") for _ in range(16)]
    with pytest.raises(ValueError, match="16"):
        Recipe(RecipeNode("Plate", 0, "Plate", contains=kids), 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["custom_wide_coop", "custom_wide_scheme1"])
def test_parallel_env_with_registered_recipes_follows_the_reference(user_recipes, name):
    """the drop-in facade with user recipes (wide tables on the device) against the reference's own run"""
    from cooking_zoo_amd.environment.cooking_env import parallel_env
    gs = GoldenSet(name)
    cfg = gs.cfg
    for ep in gs.episodes:
        random.seed(ep.seed)
        np.random.seed(ep.seed)
        A = cfg["num_agents"]
        env = parallel_env(level=cfg["level"], meta_file=cfg["meta_file"], num_agents=A, max_steps=cfg["max_steps"],
                           recipes=cfg["recipes"], obs_spaces=["feature_vector"] * A, action_scheme=cfg["action_scheme"],
                           end_condition_all_dishes=cfg["end_condition_all_dishes"], reward_scheme=cfg["reward_scheme"])
        assert env._vec.recipe_nodes == 16
        obs, _ = env.reset()
        for a in range(A):
            assert np.array_equal(obs[f"player_{a}"].view(np.uint64), ep.obs[0][a].view(np.uint64))
        for t, acts in enumerate(ep.actions):
            obs, rew, term, trunc, infos = env.step({f"player_{a}": int(acts[a]) for a in range(A)})
            for a in range(A):
                assert np.array_equal(obs[f"player_{a}"].view(np.uint64), ep.obs[t + 1][a].view(np.uint64)), (name, t, a)
                assert np.float64(rew[f"player_{a}"]).view(np.uint64) == ep.rewards[t][a].view(np.uint64), (name, t, a)
            marks = int(ep.states[t + 1][soa.W_MARKS]) | (int(ep.states[t + 1][soa.W_MARKS_HI]) << 32)
            for a in range(A):
                assert infos[f"player_{a}"]["recipe_done"] == bool((marks >> (16 * a)) & 1), (name, t, a)
            for r, g in enumerate(env.recipe_graphs):
                assert g.marks == (marks >> (16 * r)) & 0xFFFF, (name, t, r)
            if not env.agents:
                break
        env.close()
