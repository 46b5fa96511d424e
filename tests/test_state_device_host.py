"""CPU: save / restore / fork of env states on the device (cz_save_device, cz_restore_device, cz_restore_device_refused) as far as it
can be checked without a GPU: the header declares the three entry points, the built library exports them, the binding lists them, the
ABI number stayed 10, a library built before them fails at the first call and names the symbol, both Python classes have the four
methods, k_restore_where exists for all three instance sizes and every agent count behind the unchanged Params (no vector register
spilled, no scratch memory) and k_save_where exists once.

Also here: the numpy models of what the device does to a restored env's statistics (`steps_correction`, `env_steps` of
tests/host_common.py: the SU_STEPS rule), checked against a random life of 64 envs.  (cz_save_device's and
cz_restore_device's refusal of capacity < num_envs without slots is a host check, but a handle does not exist without a device: that
case is in tests/test_gpu_state_device.py.)"""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from cooking_zoo_amd import soa
from host_common import HEADER, INSTANCES, LIB, device_code, env_steps, steps_correction  # noqa: F401  (device_code: the fixture)

NEW_SYMBOLS = ["cz_save_device", "cz_restore_device", "cz_restore_device_refused"]


def test_steps_correction_keeps_env_steps_the_steps_taken():
    """a random life of 64 envs - steps, episode ends, restores of running and finished records into running and finished envs - in
    which the device's three words per env give the number of steps taken at every moment"""
    rng = np.random.default_rng(0)
    n = 64
    t, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    su, lensum, taken = np.zeros(n, np.int32), np.zeros(n, np.int64), 0
    archive_t, archive_status = rng.integers(0, 30, 16).astype(np.uint32), (rng.random(16) < 0.4).astype(np.uint32)
    kinds = set()
    for _ in range(200):
        live = status == 0
        t[live] += 1
        taken += int(live.sum())
        ends = live & (rng.random(n) < 0.1)
        lensum[ends] += t[ends]
        status[ends] = soa.STATUS_DONE
        restart = (status != 0) & (rng.random(n) < 0.3)                 # an auto-reset pass: no step, nothing counted
        t[restart], status[restart] = 0, 0
        chosen = np.nonzero(rng.random(n) < 0.2)[0]
        rows = rng.integers(0, 16, len(chosen))
        kinds |= {(int(status[e] != 0), int(archive_status[r] != 0)) for e, r in zip(chosen, rows)}
        su[chosen] += steps_correction(status[chosen], t[chosen], archive_status[rows], archive_t[rows])
        t[chosen], status[chosen] = archive_t[rows], archive_status[rows]
        assert env_steps(su, lensum, status, t) == taken
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)} and (su < 0).any() and (su > 0).any()


def test_steps_correction_wraps_like_the_devices_word():
    assert steps_correction(0, 3, 0, 10).tolist() == -7 and steps_correction(1, 3, 0, 10).tolist() == -10
    assert steps_correction(0, 3, 1, 10).tolist() == 3 and steps_correction(1, 3, 1, 10).tolist() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# declarations, exports, bindings
# ---------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    text = open(HEADER).read()
    assert re.search(r"^int cz_save_device\(cz_handle h, const int32_t \*d_slot, uint32_t \*d_records, int64_t capacity\);", text, flags=re.M)
    assert re.search(r"^int cz_restore_device\(cz_handle h, const int32_t \*d_slot, const uint32_t \*d_records, int64_t capacity,\s+"
                     r"double \*d_obs, float \*d_obs32, uint8_t \*d_codes\);", text, flags=re.M)
    assert re.search(r"^int64_t cz_restore_device_refused\(cz_handle h\);", text, flags=re.M)
    decl = text.index("int cz_save_device(")
    comment = text[text.rindex("/*", 0, decl):decl]
    for said in ("cooking_env.py:271,352-373", "cz_restore_device_refused", "DIVERGE", "NO counter", "unspecified", "descriptor row",
                 "cz_set_state", "capacity >= num_envs"):
        assert said in comment, said
    capture = text[text.index("STREAM CAPTURE"):]
    capture = capture[:capture.index("are pure kernel launches")]
    assert "cz_save_device" in capture and "cz_restore_device" in capture


def test_abi_number_stays_ten():
    from cooking_zoo_amd import _abi, _native
    assert _native.header_abi_version() == 10 == _abi.CZ_ABI_VERSION
    lib = C.CDLL(LIB)
    lib.cz_abi_version.restype = C.c_int32
    assert lib.cz_abi_version() == 10


def test_library_exports_and_binding_lists_the_entry_points():
    from cooking_zoo_amd import _native
    lib = C.CDLL(LIB)
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name + " is not exported"
        assert name in bound, name + " is not in _native.SYMBOLS"
    assert [len(bound[name][1]) for name in NEW_SYMBOLS] == [4, 7, 1]
    assert bound["cz_save_device"][1][3] is C.c_int64 and bound["cz_restore_device"][1][3] is C.c_int64
    assert bound["cz_restore_device_refused"][0] is C.c_int64


def test_a_library_without_the_entry_points_is_reported_stale_naming_the_symbol():
    """the ABI number did not move, so a library built before the three entry points still loads: what the binding puts in their place"""
    from cooking_zoo_amd import _native
    assert set(NEW_SYMBOLS) <= set(_native.ADDED_SYMBOLS)
    for name in NEW_SYMBOLS:
        with pytest.raises(_native.NativeError, match=name + r": it was built before"):
            _native._missing(name)(None)


def test_python_layer_has_the_methods():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for cls in (CookingVecEnv, ShardedVecEnv):
        assert list(inspect.signature(cls.save_device).parameters)[:3] == ["self", "d_records", "d_slot"]
        assert list(inspect.signature(cls.restore_device).parameters)[:6] == ["self", "d_records", "d_slot", "d_obs", "d_obs32", "d_codes"]
        assert list(inspect.signature(cls.fork_device).parameters) == ["self", "d_src", "d_obs", "d_obs32", "d_codes"]
        assert list(inspect.signature(cls.restore_device_refused).parameters) == ["self"]
        for f in (cls.save_device, cls.restore_device, cls.fork_device):
            assert all(p.default is None for name, p in inspect.signature(f).parameters.items() if name not in ("self", "d_records", "d_src"))
    assert "out of scope" in ShardedVecEnv.fork_device.__doc__


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels, from the compiler's metadata
# ---------------------------------------------------------------------------------------------------------------------------

def restore_where_kernels(meta):
    for inst, (opl, cpl) in INSTANCES.items():
        for na in (1, 2, 3, 4):
            prefix = f"_ZN2cz15k_restore_whereILi{opl}ELi{cpl}ELi{na}EEEvNS_6ParamsE"
            yield inst, na, [k for k in meta if k.startswith(prefix)]


def test_every_instance_has_its_restore_where_kernels(device_code):  # noqa: F811
    meta, _ = device_code
    found = list(restore_where_kernels(meta))
    assert len(found) == 12
    assert all(len(names) == 1 for _, _, names in found), [(i, na) for i, na, names in found if len(names) != 1]
    # slots, archive, capacity, recipes in the table, float64 rows, float32 rows, codes, counter: the kernel's own arguments behind
    # the unchanged Params
    assert all(names[0].endswith("NS_6ParamsEPKiPKjljPdPfPhPy") for _, _, names in found), [names for _, _, names in found]


def test_restore_where_kernels_spill_no_vector_register_and_use_no_scratch(device_code):  # noqa: F811
    meta, _ = device_code
    bad = {}
    for _, _, names in restore_where_kernels(meta):
        for k in names:
            m = meta[k]
            if int(m["vgpr_spill_count"]) != 0 or int(m["private_segment_fixed_size"]) != 0:
                bad[k] = (m["vgpr_spill_count"], m["private_segment_fixed_size"])
    assert not bad, bad


def test_save_where_is_one_kernel_without_an_instance(device_code):  # noqa: F811
    meta, _ = device_code
    names = [k for k in meta if "k_save_where" in k]
    assert len(names) == 1 and "Params" not in names[0], names
    assert int(meta[names[0]]["vgpr_spill_count"]) == 0 and int(meta[names[0]]["private_segment_fixed_size"]) == 0
