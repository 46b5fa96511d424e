#!/usr/bin/env python3
"""What the host model alone goes through in the slots tests/test_gpu_layout_generate_matrix.py draws: per case the failed draws by
kind, the successful ones, layouts with a rejection streak of at least 64 / 128, far-edge positions drawn and static objects left
out by OPTIONAL.  No device.  The floors of that module are set to about half of these figures (profiles/r17/README.md).

    python tools/layout_generate_coverage.py [--padded]"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import test_gpu_layout_generate_matrix as tm                      # noqa: E402
from layout_keyed_common import KINDS, STRESS_CASES, case_files, case_tables  # noqa: E402


def coverage(files, levels, meta, A, dims, los, L, gens, first, count):
    recs, desc = np.zeros((L, dims.RW), dtype=np.uint32), np.zeros((L, dims.F), dtype=np.uint32)
    cov, slots = tm.new_coverage(), []
    for g in gens:
        tm.expect_generation(files, levels, meta, A, dims, los, g, first, count, recs, desc, [None] * L, cov, slots)
    return cov, slots


def row(name, cov, seconds):
    failed = ", ".join(f"{k} {n}" for k, n in cov["failed"].items() if n) or "-"
    print(f"| {name} | {failed} | {cov['ok']} | {cov['streak64']} | {cov['streak128']} | {cov['far_edge']} | {cov['static_optional_stops']} | {seconds:.1f} |")


def main():
    print("| case | failed draws | successful | streak >= 64 | streak >= 128 | far edge | static OPTIONAL stops | host s |")
    print("|---|---|---|---|---|---|---|---|")
    for case in STRESS_CASES:
        for max_dyn in ((65, 129) if "--padded" in sys.argv and case in tm.STRESS_A3 else (None,)):
            t = time.time()
            level, meta, A, dims = case_tables(case, max_dyn)
            L, gens, first, count = tm.pool_shape(dims)
            cov, _ = coverage([case_files(case)], [level], meta, A, dims, np.zeros(L, dtype=np.uint8), L, gens, first, count)
            row(f"{case['level']} A{A}" + (f" D{max_dyn}" if max_dyn else ""), cov, time.time() - t)
    from cooking_zoo_amd.cooking_world.engine import load_level as ll
    stress = next(c for c in STRESS_CASES if c["level"] == "stress_second_switch")
    files = [("coop_test", "example"), (case_files(stress)[0], "example"), ("coexistence_test", "example")]
    levels, meta = [ll.load_level_file(f[0]) for f in files], ll.load_meta_file("example")
    from cooking_zoo_amd import soa
    from cooking_zoo_amd.cooking_world.layout import feature_length
    dims = soa.Dims(7, 7, max(ll.level_max_dyn(l) for l in levels), 2, feature_length(meta))
    t = time.time()
    cov, slots = coverage(files, levels, meta, 2, dims, np.repeat(np.arange(3, dtype=np.uint8), 64), 192, (1, 2, 3), 24, 144)
    assert all(64 <= s < 128 for s in slots)
    row("mixed batch (coop_test, stress_second_switch, coexistence_test) A2", cov, time.time() - t)


if __name__ == "__main__":
    main()
