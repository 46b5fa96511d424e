"""CPU: the owner template of the C API (cooking_zoo_amd/csrc/cz_owned.h) on its own.  A stand-alone program with its own main is
built from the header alone by the host C++ compiler with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child
process: nothing is preloaded, nothing is loaded into Python, no GPU.  The owner is bound to a fake release function that logs
what it was given."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cooking_zoo_amd", "csrc")

PROGRAM = r"""
#include "cz_owned.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static std::vector<int> released;                      // what the fake release function was given, in order
static int fake_release(int *p) { released.push_back(*p); return 0; }
using Own = cz::Owned<int *, fake_release>;

static int checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond); std::exit(1); } } while (0)
static bool log_is(std::vector<int> want) { const bool ok = released == want; released.clear(); return ok; }

static int fake_alloc(int **out, int *what) { *out = what; return 0; }     // a call that creates through an out-parameter
struct Three { Own a, b, c; };

int main() {
    int v[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    { Own o; Own n(nullptr); CHECK(!o && !n.get()); }
    CHECK(log_is({}));                                     // construction from null releases nothing
    { Own o(&v[1]); CHECK(o.get() == &v[1]); int *raw = o; CHECK(raw == &v[1]); CHECK(log_is({})); }
    CHECK(log_is({1}));                                    // the destructor releases exactly once
    {
        Own a(&v[1]);
        Own b(std::move(a));                               // move-construct transfers
        CHECK(!a.get() && b.get() == &v[1] && log_is({}));
        Own c(&v[2]);
        c = std::move(b);                                  // move-assign releases the previous holding and transfers
        CHECK(!b.get() && c.get() == &v[1] && log_is({2}));
        Own &self = c;
        c = std::move(self);                               // self-move-assign is harmless
        CHECK(c.get() == &v[1] && log_is({}));
    }
    CHECK(log_is({1}));
    {
        Own o(&v[3]);
        o.reset(&v[4]);                                    // reset(x) releases the old value and holds x
        CHECK(o.get() == &v[4] && log_is({3}));
        int *raw = o.release();                            // release() hands out without releasing
        CHECK(raw == &v[4] && !o.get() && log_is({}));
        o.reset();                                         // ... and an empty owner releases nothing
        CHECK(log_is({}));
    }
    CHECK(log_is({}));
    {
        Own o(&v[5]);
        int **slot = o.out();                              // the out-parameter accessor releases before it exposes the slot
        CHECK(log_is({5}) && *slot == nullptr);
        CHECK(fake_alloc(slot, &v[6]) == 0 && o.get() == &v[6]);
        CHECK(fake_alloc(o.out(), &v[7]) == 0 && o.get() == &v[7] && log_is({6}));
    }
    CHECK(log_is({7}));
    { Three t{Own(&v[1]), Own(&v[2]), Own(&v[3])}; CHECK(log_is({})); }
    CHECK(log_is({3, 2, 1}));                              // members release in reverse declaration order
    std::printf("owned ok: %d checks\n", checks);
    return 0;
}
"""


def compilers():
    found = [shutil.which("g++"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")]
    return [c for c in found if c and os.path.exists(c)][:2]


def test_owner_releases_exactly_once(tmp_path):
    cxxs = compilers()
    if not cxxs:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "owned_main.cpp"
    src.write_text(PROGRAM)
    for k, cxx in enumerate(cxxs):
        exe = tmp_path / f"owned_main_{k}"
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                                "-o", str(exe), str(src)], capture_output=True, text=True)
        assert build.returncode == 0, f"{cxx}: {build.stderr[-2000:]}"
        run = subprocess.run([str(exe)], capture_output=True, text=True, env={"PATH": os.environ.get("PATH", "")})
        assert run.returncode == 0 and "owned ok" in run.stdout, f"{cxx}: exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
