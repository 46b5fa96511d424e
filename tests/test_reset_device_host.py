"""CPU: the device-side reset of chosen envs (cz_reset_device, cz_reset_device_refused) as far as it can be checked without a GPU:
the header declares both entry points and cites the reference lines, the built library exports them, the binding lists them, the
ABI number stayed 10 (nothing but two functions was added), a library built before them fails at the first call and names the
symbol, both Python classes have the methods, and - read from the gfx950 code objects inside the built library, the compiler's own
metadata - k_reset_where exists for all three instance sizes and every agent count, spills no vector register and uses no scratch
memory."""
import ctypes as C
import inspect
import re

import pytest

from host_common import HEADER, INSTANCES, LIB, device_code  # noqa: F401  (device_code: the fixture)

NEW_SYMBOLS = ["cz_reset_device", "cz_reset_device_refused"]


def test_header_declares_the_entry_points():
    text = open(HEADER).read()
    assert re.search(r"^int cz_reset_device\(cz_handle h, const uint8_t \*d_mask, const int32_t \*d_layout_ids,\s+double \*d_obs, "
                     r"float \*d_obs32, uint8_t \*d_codes\);", text, flags=re.M)
    assert re.search(r"^int64_t cz_reset_device_refused\(cz_handle h\);", text, flags=re.M)
    decl = text.index("int cz_reset_device(")
    comment = text[text.rindex("/*", 0, decl):decl]
    assert "cooking_env.py:178-210" in comment and "cooking_env.py:271,352-373" in comment
    assert "cz_reset_device_refused" in comment
    capture = text[text.index("STREAM CAPTURE"):]
    capture = capture[:capture.index("*/")]
    assert "cz_reset_device" in capture[:capture.index("are pure kernel launches")]


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
    assert len(bound["cz_reset_device"][1]) == 6 and len(bound["cz_reset_device_refused"][1]) == 1
    assert bound["cz_reset_device_refused"][0] is C.c_int64


def test_a_library_without_the_entry_points_fails_at_the_first_call_naming_the_symbol():
    """the ABI number did not move, so a library built before the two entry points still loads: what the binding puts in their place"""
    from cooking_zoo_amd import _native
    assert set(NEW_SYMBOLS) <= set(_native.ADDED_SYMBOLS)
    for name in NEW_SYMBOLS:
        with pytest.raises(_native.NativeError, match=name + r"\b"):
            _native._missing(name)(None)


def test_python_layer_has_the_methods():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for cls in (CookingVecEnv, ShardedVecEnv):
        sig = inspect.signature(cls.reset_device)
        assert list(sig.parameters) == ["self", "d_mask", "d_layout_ids", "d_obs", "d_obs32", "d_codes"]
        assert all(p.default is None for name, p in sig.parameters.items() if name != "self")
        assert list(inspect.signature(cls.reset_device_refused).parameters) == ["self"]


def reset_where_kernels(meta):
    for inst, (opl, cpl) in INSTANCES.items():
        for na in (1, 2, 3, 4):
            prefix = f"_ZN2cz13k_reset_whereILi{opl}ELi{cpl}ELi{na}EEEvNS_6ParamsE"
            yield inst, na, [k for k in meta if k.startswith(prefix)]


def test_every_instance_has_its_reset_where_kernels(device_code):  # noqa: F811
    meta, _ = device_code
    found = list(reset_where_kernels(meta))
    assert len(found) == 12
    assert all(len(names) == 1 for _, _, names in found), [(i, na) for i, na, names in found if len(names) != 1]
    # mask, layout ids, float64 rows, float32 rows, codes, counter: the kernel's own arguments behind the unchanged Params
    assert all(names[0].endswith("NS_6ParamsEPKhPKiPdPfPhPy") for _, _, names in found)


def test_reset_where_kernels_spill_no_vector_register_and_use_no_scratch(device_code):  # noqa: F811
    meta, _ = device_code
    bad = {}
    for _, _, names in reset_where_kernels(meta):
        for k in names:
            m = meta[k]
            if int(m["vgpr_spill_count"]) != 0 or int(m["private_segment_fixed_size"]) != 0:
                bad[k] = (m["vgpr_spill_count"], m["private_segment_fixed_size"])
    assert not bad, bad
