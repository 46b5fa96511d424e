"""CPU: the one-step kernels issue every load of the constant block (Params::lut: quotient table, submask, cell-coordinate words,
recipe-row selector) before they wait for any loaded data.

A launch of the headline is bound by the latency of one wave's dependent chain, and that chain starts with memory round trips into
caches that are cold after the launch boundary.  The constant block's addresses are `P.lut + constant + 4 * lane` - they need nothing
that is loaded - so a table load that stands behind a wait is a second round trip in front of the workgroup's barrier for nothing
(k_step_lean was built that way until round 9: profiles/r09/README.md).

The check reads the device listing of cz_inst_small.hip, compiled the way `make markers` compiles it: for every k_step_lean instance
and every k_step<1,1,*,*,0>, between kernel entry and `s_barrier`, no global_load / buffer_load whose address comes from the
constant block's pointer may follow an s_waitcnt other than the one that ends the kernel-argument preload block.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cooking_zoo_amd", "csrc")
LUT_KERNARG_OFFSET = 0x10          # the step kernels' third argument (Early::lut)

KERNEL = re.compile(r"^(_ZN2cz(?:11k_step_leanILi1ELi1ELi\dELi\dEE|6k_stepILi1ELi1ELi\dELi\dELi0EE)\w*):", re.M)
REG = re.compile(r"\b([sv])(?:(\d+)|\[(\d+):(\d+)\])")
NO_DEST = ("s_waitcnt", "s_barrier", "s_branch", "s_cbranch", "s_cmp", "s_bitcmp", "s_nop", "s_endpgm", "s_setprio", "global_store",
           "buffer_store", "ds_write", "scratch_store")


def regs(text):
    out = set()
    for kind, one, lo, hi in REG.findall(text):
        out.update((kind, i) for i in (range(int(lo), int(hi) + 1) if one == "" else [int(one)]))
    return out


def late_table_loads(body):
    """the loads of the constant block that follow a wait on loaded data, in the code of one kernel up to its first s_barrier"""
    code = []
    for line in body.split("\n"):
        s = line.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            code.append(s)
            if s.startswith("s_barrier"):
                break
    assert code and code[-1].startswith("s_barrier"), "no workgroup barrier in the kernel"
    lut, preload_wait, waited, late = set(), None, False, []
    for n, ins in enumerate(code):
        mn, _, ops = ins.partition(" ")
        ops = [o.strip() for o in ops.split(",")]
        if mn == "s_waitcnt":
            if preload_wait is None:
                preload_wait = n
                assert lut, "the preload block does not fetch the table pointer"
            else:
                waited = True
            continue
        if preload_wait is None:
            # the preload block: s_load_dword* sD, s[0:1], OFFSET - which registers receive the table pointer
            if mn.startswith("s_load_dword"):
                first = min(regs(ops[0]))[1]
                off = int(ops[2], 0)
                words = {"s_load_dword": 1}.get(mn) or int(mn.rsplit("x", 1)[1])
                if off <= LUT_KERNARG_OFFSET < off + 4 * words:
                    k = first + (LUT_KERNARG_OFFSET - off) // 4
                    lut = {("s", k), ("s", k + 1)}
            continue
        if mn.startswith(NO_DEST) or (mn.startswith("v_cmp") and mn.endswith("_e32")):
            continue
        dest, srcs = regs(ops[0]), set().union(*[regs(o) for o in ops[1:]]) if len(ops) > 1 else set()
        if mn.startswith(("global_load", "buffer_load")):
            if srcs & lut and waited:
                late.append(ins)
            lut -= dest
        elif srcs & lut:
            lut |= dest                # an address made from the table pointer (a copy, pointer + offset)
        else:
            lut -= dest                # the register now holds something else
    assert preload_wait is not None
    return late


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not shutil.which("make"):
        pytest.skip("make not found")
    dry = subprocess.run(["make", "-n", "-C", CSRC, "markers"], capture_output=True, text=True, check=True).stdout
    cmd = [l for l in dry.split("\n") if " -S " in l and "--cuda-device-only" in l]
    assert len(cmd) == 1, dry
    argv = cmd[0].split()
    if not (os.path.exists(argv[0]) or shutil.which(argv[0])):
        pytest.skip("hipcc not found: " + argv[0])
    out = str(tmp_path_factory.mktemp("listing") / "cz_inst_small_mark.s")
    argv[argv.index("-o") + 1] = out
    subprocess.run(argv, cwd=CSRC, check=True, capture_output=True)
    return open(out).read()


def kernel_bodies(listing):
    heads = list(KERNEL.finditer(listing))
    for m in heads:
        end = listing.index(".Lfunc_end", m.end())
        yield m.group(1), listing[m.end():end]


def test_every_instance_is_in_the_listing(listing):
    names = [n for n, _ in kernel_bodies(listing)]
    lean = [n for n in names if "k_step_lean" in n]
    # agent counts 1..4 x schemes 1 and 3, of each kernel
    assert len(lean) == 8 and len(names) - len(lean) == 8, names


def test_table_loads_precede_the_first_wait(listing):
    bad = {name: late for name, body in kernel_bodies(listing) if (late := late_table_loads(body))}
    assert not bad, "loads of the constant block behind a wait on loaded data:\n" + "\n".join(
        "%s:\n    %s" % (n, "\n    ".join(l)) for n, l in bad.items())


def test_the_check_sees_a_late_load():
    """the check itself, on a hand-written prologue: the second table load stands behind the wait for the header words"""
    body = """
	s_load_dwordx2 s[2:3], s[0:1], 0x0
	s_load_dwordx8 s[4:11], s[0:1], 0x8
	s_waitcnt lgkmcnt(0)
	s_branch .LBB0_0
.LBB0_0:
	v_lshlrev_b32_e32 v2, 2, v0
	global_load_dword v26, v2, s[6:7] offset:2048
	v_mov_b32_e32 v3, 0
	v_lshl_add_u64 v[4:5], s[6:7], 0, v[2:3]
	s_load_dwordx4 s[28:31], s[2:3], 0x0
	s_waitcnt lgkmcnt(0)
	global_load_dword v6, v[4:5], off offset:2360
	global_load_dword v7, v2, s[2:3] offset:32
	s_barrier
"""
    assert late_table_loads(body) == ["global_load_dword v6, v[4:5], off offset:2360"]
    assert late_table_loads(body.replace("\ts_waitcnt lgkmcnt(0)\n\tglobal_load_dword v6", "\tglobal_load_dword v6")) == []
