"""CPU: the float32 observation rows (cz_step_device_f32, cz_set_f32_output, cz_observe_device_f32, cz_obs_table_f32) as far as they
can be checked without a GPU: the header declares the entry points and the built library exports them, the ABI number moved to 10
everywhere, the Python layer has the methods, and - read from the gfx950 code objects inside the built library, the compiler's own
metadata and disassembly - the k_step<..., STEP_F32> kernels exist for all three instance sizes, every agent count and both
schemes, spill no vector register and write their rows with 16-byte buffer stores."""
import ctypes as C
import re

from host_common import HEADER, INSTANCES, LIB, device_code  # noqa: F401  (device_code: the fixture)

NEW_SYMBOLS = ["cz_step_device_f32", "cz_set_f32_output", "cz_observe_device_f32", "cz_obs_table_f32"]
STEP_F32 = 6                                                    # cz::StepMode in cz_kernels.h


def test_header_declares_the_entry_points():
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(cz_handle h, " % name, text, flags=re.M), name
    assert "float *d_obs32" in text and "float table[256]" in text
    # every entry cites the reference code it stands in for
    for name in NEW_SYMBOLS:
        decl = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, decl):decl]
        assert "cooking_env.py:" in comment, name


def test_abi_number_is_ten_everywhere():
    from cooking_zoo_amd import _abi, _native
    assert _native.header_abi_version() == 10 == _abi.CZ_ABI_VERSION
    lib = C.CDLL(LIB)
    lib.cz_abi_version.restype = C.c_int32
    assert lib.cz_abi_version() == 10


def test_library_exports_and_binding_lists_the_entry_points():
    from cooking_zoo_amd import _native
    lib = C.CDLL(LIB)
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name + " is not exported"
        assert name in bound, name + " is not in _native.SYMBOLS"


def test_python_layer_has_the_methods():
    import inspect
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for cls in (CookingVecEnv, ShardedVecEnv):
        for name in ("step_device_f32", "set_f32_output", "obs_table_f32", "observe_device"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
        assert "d_obs32" in inspect.signature(cls.observe_device).parameters, cls.__name__


def f32_kernels():
    for inst, (opl, cpl) in INSTANCES.items():
        for na in (1, 2, 3, 4):
            for scheme in (1, 3):
                yield inst, f"_ZN2cz6k_stepILi{opl}ELi{cpl}ELi{na}ELi{scheme}ELi{STEP_F32}EEEvPjPKiPKdiiiiiiiNS_6ParamsE"


def test_every_instance_has_its_float32_step_kernels(device_code):  # noqa: F811
    meta, code = device_code
    missing = [(inst, k) for inst, k in f32_kernels() if k not in meta or k not in code]
    assert not missing, missing
    for opl, cpl in INSTANCES.values():
        for na in (1, 2, 3, 4):
            assert f"_ZN2cz13k_observe_f32ILi{opl}ELi{cpl}ELi{na}EEEvNS_6ParamsElPf" in meta, (opl, cpl, na)


def test_float32_kernels_spill_no_vector_register(device_code):  # noqa: F811
    meta, _ = device_code
    names = [k for _, k in f32_kernels()] + [k for k in meta if "k_observe_f32" in k]
    assert len(names) == 24 + 12
    spills = {k: meta[k]["vgpr_spill_count"] for k in names if int(meta[k]["vgpr_spill_count"]) != 0}
    assert not spills, spills


def test_float32_kernels_write_rows_with_16_byte_buffer_stores(device_code):  # noqa: F811
    _, code = device_code
    for inst, k in f32_kernels():
        na = int(re.search(r"k_stepILi\d+ELi\d+ELi(\d)E", k).group(1))
        stores = [l for l in code[k] if l.startswith("buffer_store_dwordx4")]
        # one store per observer and round of 256 features, in each of the three cache-policy flavours (plain / sc1 / nt), for
        # the two prefetched rounds and the loop behind them; and no narrower store into a row
        assert len(stores) >= 3 * na, (inst, k, len(stores))
        assert any(" sc1" in l for l in stores) and any(" nt" in l for l in stores), (inst, k)
        assert not [l for l in code[k] if re.match(r"buffer_store_(dword|dwordx2|dwordx3|short|byte)\b", l)], (inst, k)


def test_existing_step_kernels_carry_no_float32_path(device_code):  # noqa: F811
    """the one-step float64 kernel of the headline has its 16-byte stores and nothing of the new stage (same count as the lean one)"""
    _, code = device_code
    k0 = "_ZN2cz6k_stepILi1ELi1ELi2ELi3ELi0EEEvPjPKiPKdiiiiiiiNS_6ParamsE"
    k6 = k0.replace("ELi0EEEv", "ELi6EEEv")
    assert k0 in code and k6 in code
    assert "v_cvt_f32_f64" not in " ".join(code[k0]) and "v_cvt_f32_f64" in " ".join(code[k6])
