"""CPU tests of the batched fixture sets' boundary (include/b2hip.h, block J: b2hip_fixture_set_filters,
b2hip_fixture_set_sensors, b2hip_fixture_set_thicks, b2hip_fixture_set_materials): declared with their definition by
equivalence, exported, bound in Python beside the single calls they are defined by, and argument errors refused before the
world is looked at or any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_fixture_set_filters", "b2hip_fixture_set_sensors", "b2hip_fixture_set_thicks", "b2hip_fixture_set_materials")
SINGLES = ("b2hip_fixture_set_filter", "b2hip_fixture_set_sensor", "b2hip_fixture_set_thick", "b2hip_fixture_set_material")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def _err(L):
    msg = L.b2hip_last_error()
    assert msg, "no b2hip_last_error message"
    return msg.decode()


def test_header_declares_the_calls_and_defines_them_by_equivalence():
    whole = open(HDR).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    head = r"\bint\s+%s\s*\(\s*b2hip_world\s*\*\s*w\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*fixtures\s*,\s*"
    assert re.search(head % "b2hip_fixture_set_filters" + r"const\s+b2hip_fixture_filter\s*\*\s*filters\s*\)", text)
    assert re.search(head % "b2hip_fixture_set_sensors" + r"const\s+uint8_t\s*\*\s*sensor\s*\)", text)
    assert re.search(head % "b2hip_fixture_set_thicks" + r"const\s+uint8_t\s*\*\s*thick\s*\)", text)
    assert re.search(head % "b2hip_fixture_set_materials" + r"const\s+b2hip_fixture_material\s*\*\s*materials\s*,\s*int\s+mask\s*\)", text)
    assert re.search(r"uint16_t\s+category_bits\s*,\s*mask_bits\s*;\s*int16_t\s+group_index\s*;\s*uint16_t\s+pad\s*;\s*}\s*b2hip_fixture_filter\s*;", text)
    assert re.search(r"float\s+density\s*,\s*friction\s*,\s*restitution\s*;\s*}\s*b2hip_fixture_material\s*;", text)
    for name, value in (("DENSITY", 1), ("FRICTION", 2), ("RESTITUTION", 4)):
        assert re.search(r"#define\s+B2HIP_MATERIAL_%s\s+%d\b" % (name, value), text)
    block = whole[whole.index("---- J. Batched fixture sets"):]
    for word in ("Definition by equivalence", "b2hip_fixture_set_filter(w, fixtures[i]", "b2hip_fixture_set_sensor(w, fixtures[i], sensor[i] != 0)",
                 "b2hip_fixture_set_thick(w, fixtures[i], thick[i] != 0)", "b2hip_fixture_set_material(w, fixtures[i]", "move buffer",
                 "B2HIP_ERR_UNSUPPORTED", "AT MOST ONCE", "is a no-op", "always re-filters", "Out of scope", "A refused call applies nothing"):
        assert word in block, word
    # the function map at the head of the file
    assert "b2hip_fixture_set_filters / _sensors / _thicks / _materials" in whole[:whole.index("#ifndef B2HIP_H")]


def test_library_exports_the_calls():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES + SINGLES:
        assert hasattr(L, name), name


def test_python_world_has_the_methods_with_argtypes():
    for m in ("fixture_set_filters", "fixture_set_sensors", "fixture_set_thicks", "fixture_set_materials", "fixture_set_filter", "fixture_set_sensor",
              "fixture_set_thick", "fixture_set_material"):
        assert callable(getattr(b2hip.World, m, None)), m
    L = _lib()
    for name in NAMES + SINGLES:
        assert getattr(L, name).argtypes is not None, name
    assert list(L.b2hip_fixture_set_filter.argtypes) == [C.c_void_p, C.c_int, C.c_uint16, C.c_uint16, C.c_int16]
    assert list(L.b2hip_fixture_set_thick.argtypes) == [C.c_void_p, C.c_int, C.c_int]
    assert list(L.b2hip_fixture_set_material.argtypes) == [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [4, 4, 4, 5]
    assert b2hip.FIXTURE_FILTER_DTYPE.itemsize == 8 and b2hip.FIXTURE_MATERIAL_DTYPE.itemsize == 12
    assert (b2hip.MATERIAL_DENSITY, b2hip.MATERIAL_FRICTION, b2hip.MATERIAL_RESTITUTION) == (1, 2, 4)


def test_python_shapes_are_validated():
    w = b2hip.World.__new__(b2hip.World)  # (no world is needed to learn that the arguments do not fit)
    w.p = None
    with pytest.raises(ValueError):
        w.fixture_set_filters([[0, 1]], 1, 0xFFFF, 0)
    with pytest.raises(ValueError):
        w.fixture_set_filters([0, 1], [1, 2, 4], 0xFFFF, 0)
    with pytest.raises(ValueError):
        w.fixture_set_sensors([0, 1], [True, False, True])
    with pytest.raises(ValueError):
        w.fixture_set_thicks([[0, 1]], True)
    with pytest.raises(ValueError):
        w.fixture_set_materials([0, 1], friction=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        w.fixture_set_materials([0, 1])  # (nothing to set: the mask would be empty)


def test_null_world_and_bad_arguments_are_refused_in_order():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ids = np.arange(4, dtype=np.int32)
    filters = np.zeros(4, b2hip.FIXTURE_FILTER_DTYPE)
    flags = np.ones(4, np.uint8)
    materials = np.zeros(4, b2hip.FIXTURE_MATERIAL_DTYPE)
    calls = {
        "b2hip_fixture_set_filters": lambda n, f, v: L.b2hip_fixture_set_filters(None, n, f, v),
        "b2hip_fixture_set_sensors": lambda n, f, v: L.b2hip_fixture_set_sensors(None, n, f, v),
        "b2hip_fixture_set_thicks": lambda n, f, v: L.b2hip_fixture_set_thicks(None, n, f, v),
        "b2hip_fixture_set_materials": lambda n, f, v: L.b2hip_fixture_set_materials(None, n, f, v, 7),
    }
    values = {"b2hip_fixture_set_filters": filters, "b2hip_fixture_set_sensors": flags, "b2hip_fixture_set_thicks": flags,
              "b2hip_fixture_set_materials": materials}
    for name, call in calls.items():
        # valid arguments, null world: the world is what is missing (nothing to do, and still no world)
        for args in ((4, vp(ids), vp(values[name])), (0, None, None)):
            assert call(*args) == ERR_INVALID
            assert "world" in _err(L)
        # n outside [0, 2^24]: reported before the pointers, with the call's name
        for n in (-1, (1 << 24) + 1):
            for args in ((n, vp(ids), vp(values[name])), (n, None, None)):
                assert call(*args) == ERR_INVALID
                assert "n must" in _err(L) and name in _err(L)
        # null pointers with entries
        for args in ((1, None, vp(values[name])), (1, vp(ids), None)):
            assert call(*args) == ERR_INVALID
            assert "null" in _err(L) and name in _err(L)
    # (a bad mask is reported behind the world: with a null world the world is what is missing)
    assert L.b2hip_fixture_set_materials(None, 4, vp(ids), vp(materials), 0) == ERR_INVALID
    assert "world" in _err(L)
