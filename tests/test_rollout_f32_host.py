"""CPU: the float32 trajectories of the fused rollouts (cz_rollout_f32, cz_rollout_actions_f32) as far as they can be checked without
a GPU: the header declares both entry points and the built library exports them, the binding lists them, the ABI number stayed 10
(nothing but two functions was added), the Python layer has the methods, and - read from the gfx950 code objects inside the built
library, the compiler's own metadata - k_step<..., ROLLOUT_F32> and k_step<..., ROLLOUT_ACTIONS_F32> exist for all three instance
sizes, every agent count and both schemes, spill no vector register and use no scratch memory."""
import ctypes as C
import inspect
import re

import pytest

from host_common import HEADER, INSTANCES, LIB, device_code  # noqa: F401  (device_code: the fixture)

NEW_SYMBOLS = ["cz_rollout_f32", "cz_rollout_actions_f32"]
ROLLOUT_F32, ROLLOUT_ACTIONS_F32 = 7, 8                           # cz::StepMode in cz_kernels.h


def test_header_declares_the_entry_points():
    text = open(HEADER).read()
    assert re.search(r"^int cz_rollout_f32\(cz_handle h, int32_t T, uint64_t seed, uint32_t step0, float \*d_obs32,\s+double \*d_rewards,"
                     r"\s+uint8_t \*d_terminations, uint8_t \*d_truncations\);", text, flags=re.M)
    assert re.search(r"^int cz_rollout_actions_f32\(cz_handle h, int32_t T, const int32_t \*d_actions, float \*d_obs32,\s+double \*d_rewards,"
                     r"\s+uint8_t \*d_terminations, uint8_t \*d_truncations\);", text, flags=re.M)
    for name in NEW_SYMBOLS:                                     # every entry cites the reference code it stands in for
        decl = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, decl):decl]
        assert "cooking_env.py:243-269" in comment and "352-373" in comment, name
    setting = text[:text.index("int cz_set_f32_output(")]
    setting = setting[setting.rindex("/*"):]
    assert "their float32-sized form is the compact trajectory" not in setting and "cz_rollout_f32" in setting


def test_abi_number_stays_ten():
    from cooking_zoo_amd import _abi, _native
    assert _native.header_abi_version() == 10 == _abi.CZ_ABI_VERSION
    lib = C.CDLL(LIB)
    lib.cz_abi_version.restype = C.c_int32
    assert lib.cz_abi_version() == 10


def test_library_exports_and_binding_lists_the_entry_points():
    from cooking_zoo_amd import _native
    lib = C.CDLL(LIB)
    bound = {name: args for name, _, args in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name + " is not exported"
        assert name in bound, name + " is not in _native.SYMBOLS"
    assert len(bound["cz_rollout_f32"]) == 8 and len(bound["cz_rollout_actions_f32"]) == 7


def test_a_library_without_the_entry_points_fails_at_the_first_call_naming_the_symbol():
    """the ABI number did not move, so a library built before the two entry points still loads: what the binding puts in their place"""
    from cooking_zoo_amd import _native
    assert set(NEW_SYMBOLS) <= set(_native.ADDED_SYMBOLS)
    for name in NEW_SYMBOLS:
        with pytest.raises(_native.NativeError, match=name + r"\b"):
            _native._missing(name)(None, 1)


def test_python_layer_has_the_methods():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    from cooking_zoo_amd.vec_env import CookingVecEnv
    for cls in (CookingVecEnv, ShardedVecEnv):
        assert list(inspect.signature(cls.rollout_f32).parameters) == ["self", "T", "seed", "step0", "d_obs32", "d_rewards", "d_term", "d_trunc"]
        assert list(inspect.signature(cls.rollout_actions_f32).parameters) == ["self", "d_actions", "T", "d_obs32", "d_rewards", "d_term", "d_trunc"]


def rollout_f32_kernels():
    for inst, (opl, cpl) in INSTANCES.items():
        for na in (1, 2, 3, 4):
            for scheme in (1, 3):
                for mode in (ROLLOUT_F32, ROLLOUT_ACTIONS_F32):
                    yield inst, f"_ZN2cz6k_stepILi{opl}ELi{cpl}ELi{na}ELi{scheme}ELi{mode}EEEvPjPKiPKdiiiiiiiNS_6ParamsE"


def test_every_instance_has_its_float32_rollout_kernels(device_code):  # noqa: F811
    meta, code = device_code
    names = list(rollout_f32_kernels())
    assert len(names) == 48
    missing = [(inst, k) for inst, k in names if k not in meta or k not in code]
    assert not missing, missing


def test_float32_rollout_kernels_spill_no_vector_register_and_use_no_scratch(device_code):  # noqa: F811
    meta, _ = device_code
    bad = {}
    for _, k in rollout_f32_kernels():
        m = meta[k]
        if int(m["vgpr_spill_count"]) != 0 or int(m["private_segment_fixed_size"]) != 0:
            bad[k] = (m["vgpr_spill_count"], m["private_segment_fixed_size"])
    assert not bad, bad


def test_float32_rollout_kernels_stage_the_rounded_table_and_write_16_byte_rows(device_code):  # noqa: F811
    _, code = device_code
    for inst, k in rollout_f32_kernels():
        text = " ".join(code[k])
        assert "v_cvt_f32_f64" in text, (inst, k)
        stores = [l for l in code[k] if l.startswith("buffer_store_dwordx4")]
        assert any(" nt" in l for l in stores) and any(" sc1" in l for l in stores), (inst, k)
