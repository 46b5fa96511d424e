"""Shared by tests/test_layout_keyed.py (host) and tests/test_gpu_layout_generate.py (device): the fixture of keyed level draws
captured from the unmodified reference parser (tools/gen_golden.py layout_draws_keyed) and how a `Layout` is compared with it."""
import json
import os

from cooking_zoo_amd import soa
from cooking_zoo_amd.cooking_world.engine import load_level as ll
from cooking_zoo_amd.cooking_world.layout import feature_length

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "layouts_keyed_ref.json")))
CASE_IDS = [f"{c['level']}-A{c['num_agents']}" for c in CASES]


def case_tables(case, max_dyn=None):
    """-> (level object, meta dict, num_agents, dims) of a fixture case; max_dyn pads the slot capacity (another kernel instance)"""
    level, meta = ll.load_level_file(case["level"]), ll.load_meta_file(case["meta"])
    rows = level["LEVEL_LAYOUT"].splitlines()
    dims = soa.Dims(len(rows[-1]), len(rows), max_dyn or ll.level_max_dyn(level), case["num_agents"], feature_length(meta))
    return level, meta, case["num_agents"], dims


def assert_matches_reference(lay, ref):
    """statics in list order, dynamics in key / list order, agents - as tests/test_level_loading.py compares layouts_ref.json"""
    W = ref["width"]
    assert (lay.width, lay.height) == (ref["width"], ref["height"])
    assert lay.agents == [tuple(a) for a in ref["agents"]]
    for name, cells in ref["statics"].items():
        assert lay.static_lists.get(name, []) == [y * W + x for x, y in cells], name
    assert [soa.DYNAMIC_CLASSES[c] for c, _ in lay.dyn_classes] == [k for k, _ in ref["dynamics"]]
    assert lay.dyn_xy == [tuple(p) for _, v in ref["dynamics"] for p in v]
