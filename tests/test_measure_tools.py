"""tools/measure.py without a device: the row format and its inverse over the timing tools' real leg names, the parent / change
driver's run order and what it does after a child that fails or hangs (the children are stand-in scripts), and the band rule."""
import os
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
sys.path.insert(0, TOOLS)
import measure  # noqa: E402

LEGS = [                                                 # literals of the eleven tools
    "float64 rows", "codes only", "no observation", "float64 + codes",
    "float64 trajectory", "compact trajectory", "ring run fused, float64 rows in place",
    "stay", "random", "rich",
    "pinned_outputs=False, host-array step", "pinned_outputs=True, COMPACT observation (uint8 codes)", "pinned_outputs=True, no observation copy",
    "step, float64 rows (direct launches from Python)", "step, codes + float64",
    "graph of 200 step kernels WITHOUT the policy kernel: codes only", "closed loop: float64",
    "f32 wt=auto", "closed loop f64+float() (eager launches from Python, one stream)",
    "rollout_actions f64", "f64 + convert", "codes + gather", "rollout_actions_f32",
    "one step (float64 rows)", "reset_device no rows 0 % chosen (0)", "reset_device float32 rows 10 % chosen (409)",
    "loop: step_device_f32 + reset_device(), auto_reset off", "loop: step_device_f32 alone, auto_reset on",
    "step lean", "one step generic launch", "collect all 1 % (656 found)", "collect dense 100 % (65536 found)",
    "save_device, identity", "restore_device float32 rows 100 % chosen (65536)", "fork_device no rows a permutation (2 launches)",
    "the whole batch (65536 envs) get_state + set_state + observe_device + sync",
    "1 % as one range (40 envs) save_device + restore_device (f32 rows) + sync",
    "step_device, no observation + observe_grid_device grid32", "observe_grid_device grid8 extended",
    "host route: numpy model (grid.host_bits + expand)", "host route: get_state + grid.host_bits + expand + upload",
]
US = [5.521, 5.653, 26121.414, 0.004, 5.942]


@pytest.mark.parametrize("n", [4096, 131072])
@pytest.mark.parametrize("note", ["", "4.61 G env-steps/s (0.217 ns per env-step)", "episodes of 50; 1 | 2"])
def test_row_round_trip(n, note):
    for leg in LEGS:
        for label in ("parent", "change", "f32", "a label of some length"):
            line = measure.format_row(label, leg, n, "launch", US, note)
            assert measure.parse_row(line) == (label, leg, n, "launch", US, note), line
    assert measure.parse_row(measure.format_row("change", "x" * 200, n, "live env-step", [1.0])) == ("change", "x" * 200, n, "live env-step", [1.0], "")


def test_other_lines_are_no_rows():
    for line in ("", "# run 3: parent", "  4096 envs  record: 23 words", "| 1 | step lean, 4096 envs | 1.000 / 2.000 / 3.000 | yes |",
                 "  per step: step + grid32 7.1 us  against  step_device_f32 5.5 us"):
        assert measure.parse_row(line) is None


CHILD = """import os, sys, time; sys.path.insert(0, {tools!r}); import measure
label, starts = sys.argv[sys.argv.index("--label") + 1], {starts!r}
open(starts, "a").write(" ".join(sys.argv[1:]) + "\\n"); nth = len(open(starts).readlines())
print(measure.format_row(label, "step lean", 4096, "launch", [5.0 + nth, 5.5, 6.0])); print("not a row", flush=True)
{second}
"""


def driver(tmp_path, pairs, second="pass", other=None, timeout_s=60):
    """alternate() over a stand-in child; `second` is what the child does at its second start.  -> (return value, starts, out)"""
    starts, out, script = tmp_path / "starts", tmp_path / "deep" / "er" / "out.txt", tmp_path / "child.py"
    script.write_text(CHILD.format(tools=TOOLS, starts=str(starts), second=f"if nth == 2: {second}"))
    rc = measure.alternate(str(script), str(other or tmp_path), pairs, ["--launches", "7"], timeout_s, str(out))
    return rc, starts.read_text().splitlines(), out.read_text()


@pytest.mark.parametrize("pairs", [1, 3])
def test_run_order(tmp_path, pairs):
    rc, starts, out = driver(tmp_path, pairs)
    assert rc == 0
    labels = [s.split("--label ")[1].split()[0] for s in starts]
    assert labels == ["parent", "change"] * pairs + ["change", "parent"]
    for s, label in zip(starts, labels):                                 # a directory is the other side's --tree
        assert s.startswith("--launches 7") and (f"--tree {tmp_path}" in s) == (label == "parent")
    assert [line for line in out.splitlines() if line.startswith("# run")] == [f"# run {i}: {label}" for i, label in enumerate(labels)]
    assert out.splitlines()[-1] == f"{pairs + 1} rows, 0 outside"        # one leg per child, one band row per pair
    assert "step lean | 4096 envs | change - parent (means)" in out


def test_a_library_is_the_other_sides_lib(tmp_path):
    lib = tmp_path / "libother.so"
    lib.write_bytes(b"")
    rc, starts, _ = driver(tmp_path, 1, other=lib)
    assert rc == 0 and [f"--lib {lib}" in s for s in starts] == [True, False, False, True] and not any("--tree" in s for s in starts)


def test_nothing_is_started_after_a_failed_child(tmp_path):
    rc, starts, out = driver(tmp_path, 3, "sys.stderr.write('the card fell over'); sys.exit(3)")
    assert rc != 0 and len(starts) == 2
    assert measure.parse_row(out.splitlines()[1]) == ("parent", "step lean", 4096, "launch", [6.0, 5.5, 6.0], "")
    assert "status 3" in out and "nothing more is started" in out and "the card fell over" in out and "# summary" not in out


def test_nothing_is_started_after_a_child_that_hangs(tmp_path):
    pid = tmp_path / "pid"
    rc, starts, out = driver(tmp_path, 3, f"open({str(pid)!r}, 'w').write(str(os.getpid())); time.sleep(60)", timeout_s=1)
    assert rc != 0 and len(starts) == 2
    assert measure.parse_row(out.splitlines()[1]) == ("parent", "step lean", 4096, "launch", [6.0, 5.5, 6.0], "")
    assert "timeout after 1 s" in out and "nothing more is started" in out and "# summary" not in out
    with pytest.raises(ProcessLookupError):                             # the child is gone
        os.kill(int(pid.read_text()), 0)


@pytest.mark.parametrize("parent, median, ok", [
    ([1.0, 1.5, 2.0], 1.5, True), ([1.0, 1.5, 2.0], 0.0, True), ([1.0, 1.5, 2.0], 3.0, True),       # inside, and on each edge of 0 .. 3
    ([1.0, 1.5, 2.0], -0.001, False), ([1.0, 1.5, 2.0], 3.001, False),                                # just outside each edge
    ([2.0, 2.0, 2.0], 2.0, True), ([2.0, 2.0, 2.0], 2.001, False), ([2.0, 2.0, 2.0], 1.999, False),   # a band of no width
])
def test_band_rule(parent, median, ok):
    lo, hi = min(parent), max(parent)
    assert measure.holds(parent, median) == (ok, lo - (hi - lo), hi + (hi - lo))


def test_summary_counts_the_rows_outside():
    row = lambda label, leg, us: (label, leg, 4096, "call", us, "")
    runs = [("parent", [row("parent", "a", [1.0, 1.5, 2.0]), row("parent", "b (x, y) 100 %", [4.0, 4.0, 4.1])]),
            ("change", [row("change", "a", [2.5, 2.9, 9.0]), row("change", "b (x, y) 100 %", [4.0, 4.3, 4.4])]),
            ("change", [row("change", "a", [1.0, 3.5, 4.0])]), ("parent", [row("parent", "a", [1.0, 1.5, 2.0]), row("parent", "c", [1.0])])]
    lines = measure.summary(runs)
    assert lines[-1] == "3 rows, 2 outside"
    assert "| 1 | a, 4096 envs | 1.000 / 1.500 / 2.000 | 2.500 / 2.900 / 9.000 | 0.000 .. 3.000 | yes |" in lines
    assert "| 1 | b (x, y) 100 %, 4096 envs | 4.000 / 4.000 / 4.100 | 4.000 / 4.300 / 4.400 | 3.900 .. 4.200 | **no** |" in lines
    assert "| 2 | a, 4096 envs | 1.000 / 1.500 / 2.000 | 1.000 / 3.500 / 4.000 | 0.000 .. 3.000 | **no** |" in lines
    assert "a | 4096 envs | parent  | 1.500 1.500 | spread 0.000 | mean 1.500" in lines
    assert "a | 4096 envs | change  | 2.900 3.500 | spread 0.600 | mean 3.200" in lines
    assert "a | 4096 envs | change - parent (means) | +1.700 us" in lines
