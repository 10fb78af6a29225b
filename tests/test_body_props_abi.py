"""CPU tests of the batched body property sets' boundary (include/b2hip.h, block K: b2hip_set_types, b2hip_set_bullets,
b2hip_set_fixed_rotations, b2hip_set_sleeping_alloweds, b2hip_set_body_dampings, b2hip_set_mass_datas, b2hip_reset_mass_datas):
declared with their definition by equivalence, exported, bound in Python beside the single calls they are defined by, and
argument errors refused before the world is looked at or any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
FLAG_CALLS = ("b2hip_set_types", "b2hip_set_bullets", "b2hip_set_fixed_rotations", "b2hip_set_sleeping_alloweds")
NAMES = FLAG_CALLS + ("b2hip_set_body_dampings", "b2hip_set_mass_datas", "b2hip_reset_mass_datas")
SINGLES = ("b2hip_set_type", "b2hip_set_bullet", "b2hip_set_fixed_rotation", "b2hip_set_sleeping_allowed", "b2hip_set_body_damping",
           "b2hip_set_mass_data", "b2hip_get_mass_data")
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
    head = r"\bint\s+%s\s*\(\s*b2hip_world\s*\*\s*w\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*bodies\s*"
    for name, arg in (("b2hip_set_types", "type"), ("b2hip_set_bullets", "bullet"), ("b2hip_set_fixed_rotations", "flag"),
                      ("b2hip_set_sleeping_alloweds", "flag")):
        assert re.search(head % name + r",\s*const\s+uint8_t\s*\*\s*%s\s*\)" % arg, text), name
    assert re.search(head % "b2hip_set_body_dampings" + r",\s*const\s+b2hip_body_damping\s*\*\s*d\s*,\s*int\s+mask\s*\)", text)
    assert re.search(head % "b2hip_set_mass_datas" + r",\s*const\s+b2hip_mass_data\s*\*\s*md\s*\)", text)
    assert re.search(head % "b2hip_reset_mass_datas" + r"\)", text)
    for macro, value in (("B2HIP_DAMPING_LINEAR", 1), ("B2HIP_DAMPING_ANGULAR", 2), ("B2HIP_DAMPING_GRAVITY_SCALE", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
    assert re.search(r"typedef\s+struct\s+b2hip_body_damping\s*\{\s*float\s+linear_damping\s*,\s*angular_damping\s*,\s*gravity_scale\s*;"
                     r"\s*float\s+pad\s*;\s*\}\s*b2hip_body_damping\s*;", text)
    block = whole[whole.index("---- K. Batched body property sets"):]
    for word in ("Definition by equivalence", "b2hip_set_type(w, bodies[i], type[i])", "b2hip_set_bullet(w, bodies[i], bullet[i] != 0)",
                 "b2hip_set_fixed_rotation(w, bodies[i], flag[i] != 0)", "b2hip_set_sleeping_allowed(w, bodies[i], flag[i] != 0)",
                 "b2hip_set_body_damping(w, bodies[i], linear_damping, angular_damping, gravity_scale)",
                 "b2hip_set_mass_data(w, bodies[i], &md[i])", "b2hip_set_mass_data(w, bodies[i], NULL)", "No-ops", "Who wakes",
                 "move buffer", "B2HIP_ERR_UNSUPPORTED", "to-static refit fall-back", "believed unreachable", "AT MOST ONCE"):
        assert word in block, word
    # the function map at the head of the file
    assert "b2hip_set_types / _bullets / _fixed_rotations" in whole[:whole.index("#ifndef B2HIP_H")]
    # block J no longer calls them out of scope
    j = whole[whole.index("---- J. Batched fixture sets"):whole.index("---- K. Batched body property sets")]
    assert "live in" in j and "block K" in j


def test_library_exports_the_calls():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES + SINGLES:
        assert hasattr(L, name), name


def test_python_world_has_the_methods_with_argtypes():
    for m in ("set_types", "set_bullets", "set_fixed_rotations", "set_sleeping_alloweds", "set_body_dampings", "set_mass_datas",
              "reset_mass_datas", "set_type", "set_bullet", "set_body_damping", "set_fixed_rotation", "set_sleeping_allowed",
              "set_mass_data", "mass_data"):
        assert callable(getattr(b2hip.World, m, None)), m
    L = _lib()
    for name in NAMES + SINGLES:
        assert getattr(L, name).argtypes is not None, name
    for name in FLAG_CALLS + ("b2hip_set_mass_datas",):
        assert list(getattr(L, name).argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], name
    assert list(L.b2hip_set_body_dampings.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    assert list(L.b2hip_reset_mass_datas.argtypes) == [C.c_void_p, C.c_int, C.c_void_p]
    assert list(L.b2hip_set_type.argtypes) == [C.c_void_p, C.c_int, C.c_int]
    assert b2hip.BODY_DAMPING_DTYPE.itemsize == 16 and b2hip.MASS_DATA_DTYPE.itemsize == 24
    assert (b2hip.DAMPING_LINEAR, b2hip.DAMPING_ANGULAR, b2hip.DAMPING_GRAVITY_SCALE) == (1, 2, 4)


def test_python_shapes_are_validated():
    w = b2hip.World.__new__(b2hip.World)  # (no world is needed to learn that the arguments do not fit)
    w.p = None
    for call in (lambda: w.set_types([[0, 1]], b2hip.STATIC), lambda: w.set_types([0, 1], [0, 1, 2]), lambda: w.set_types([0, 1], 300),
                 lambda: w.set_bullets([0, 1], [True, False, True]), lambda: w.set_bullets([[0, 1]]),
                 lambda: w.set_fixed_rotations([0, 1], [True] * 3), lambda: w.set_sleeping_alloweds([0, 1], [[True, False]]),
                 lambda: w.set_body_dampings([0, 1]), lambda: w.set_body_dampings([0, 1], linear=[0.1, 0.2, 0.3]),
                 lambda: w.set_body_dampings([[0, 1]], angular=0.5),
                 lambda: w.set_mass_datas([0, 1], [1.0, 2.0, 3.0], 1.0, (0.0, 0.0)), lambda: w.set_mass_datas([0, 1], 1.0, 1.0, [[0.0, 0.0]] * 3),
                 lambda: w.set_mass_datas([0, 1], 1.0, 1.0, (0.0, 0.0, 0.0)), lambda: w.reset_mass_datas([[0, 1]])):
        with pytest.raises(ValueError):
            call()


def test_null_world_and_bad_arguments_are_refused_in_order():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bodies = np.arange(4, dtype=np.int32)
    flags = np.ones(4, np.uint8)
    bad_types = np.full(4, 3, np.uint8)
    damp = np.zeros(4, b2hip.BODY_DAMPING_DTYPE)
    mass = np.zeros(4, b2hip.MASS_DATA_DTYPE)
    with_values = [(getattr(L, name), flags) for name in FLAG_CALLS] + [(L.b2hip_set_mass_datas, mass)]
    da, re_ = L.b2hip_set_body_dampings, L.b2hip_reset_mass_datas
    # valid arguments, null world: the world is what is missing (nothing to do, and still no world) - a bad type or mask is
    # looked at after the world
    calls = [lambda f=f, v=v: f(None, 4, vp(bodies), vp(v)) for f, v in with_values] + [lambda f=f: f(None, 0, None, None) for f, _ in with_values]
    calls += [lambda: da(None, 4, vp(bodies), vp(damp), 7), lambda: da(None, 0, None, None, 1), lambda: da(None, 4, vp(bodies), vp(damp), 0),
              lambda: da(None, 4, vp(bodies), vp(damp), 8), lambda: re_(None, 4, vp(bodies)), lambda: re_(None, 0, None),
              lambda: L.b2hip_set_types(None, 4, vp(bodies), vp(bad_types))]
    for call in calls:
        assert call() == ERR_INVALID
        assert "world" in _err(L)
    # n outside [0, 2^24]: reported before the pointers
    for n in (-1, (1 << 24) + 1):
        calls = [lambda f=f, v=v: f(None, n, vp(bodies), vp(v)) for f, v in with_values] + [lambda f=f: f(None, n, None, None) for f, _ in with_values]
        calls += [lambda: da(None, n, vp(bodies), vp(damp), 7), lambda: da(None, n, None, None, 0), lambda: re_(None, n, vp(bodies)),
                  lambda: re_(None, n, None)]
        for call in calls:
            assert call() == ERR_INVALID
            assert "n must" in _err(L)
    # null pointers with entries
    calls = [lambda f=f, v=v: f(None, 1, None, vp(v)) for f, v in with_values] + [lambda f=f: f(None, 1, vp(bodies), None) for f, _ in with_values]
    calls += [lambda: da(None, 1, None, vp(damp), 7), lambda: da(None, 1, vp(bodies), None, 7), lambda: re_(None, 1, None)]
    for call in calls:
        assert call() == ERR_INVALID
        assert "null" in _err(L)
