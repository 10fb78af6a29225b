"""CPU tests of the batched destruction and activation sets' boundary (include/b2hip.h, block I: b2hip_destroy_bodies,
b2hip_set_actives): declared with their definition by equivalence, exported, bound in Python beside the single
b2hip_set_active, and argument errors refused before the world is looked at or any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_destroy_bodies", "b2hip_set_actives")
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
    assert re.search(r"\bint\s+b2hip_destroy_bodies\s*\(\s*b2hip_world\s*\*\s*w\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*bodies\s*\)", text)
    assert re.search(r"\bint\s+b2hip_set_actives\s*\(\s*b2hip_world\s*\*\s*w\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*bodies\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*active\s*\)", text)
    block = whole[whole.index("---- I. Batched destruction"):]
    for word in ("Definition by equivalence", "b2hip_destroy_body(w, bodies[i])", "b2hip_set_active(w, bodies[i], active[i] != 0)",
                 "move buffer", "B2HIP_ERR_UNSUPPORTED", "AT MOST ONCE", "live joint", "the ONE place where a refused"):
        assert word in block, word
    # the function map at the head of the file
    assert "b2hip_destroy_bodies / b2hip_set_actives" in whole[:whole.index("#ifndef B2HIP_H")]


def test_library_exports_the_calls():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES + ("b2hip_destroy_body", "b2hip_set_active"):
        assert hasattr(L, name), name


def test_python_world_has_the_methods_with_argtypes():
    for m in ("destroy_bodies", "set_actives", "set_active", "destroy_body"):
        assert callable(getattr(b2hip.World, m, None)), m
    L = _lib()
    for name in NAMES + ("b2hip_set_active",):
        assert getattr(L, name).argtypes is not None, name
    assert list(L.b2hip_set_active.argtypes) == [C.c_void_p, C.c_int, C.c_int]
    assert len(L.b2hip_destroy_bodies.argtypes) == 3 and len(L.b2hip_set_actives.argtypes) == 4


def test_python_shapes_are_validated():
    w = b2hip.World.__new__(b2hip.World)  # (no world is needed to learn that the arguments do not fit)
    w.p = None
    with pytest.raises(ValueError):
        w.destroy_bodies([[0, 1]])
    with pytest.raises(ValueError):
        w.set_actives([0, 1], [True, False, True])
    with pytest.raises(ValueError):
        w.set_actives([[0, 1]], True)


def test_null_world_and_bad_arguments_are_refused_in_order():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bodies = np.arange(4, dtype=np.int32)
    active = np.ones(4, np.uint8)
    de, ac = L.b2hip_destroy_bodies, L.b2hip_set_actives
    # valid arguments, null world: the world is what is missing (nothing to do, and still no world)
    for call in (lambda: de(None, 4, vp(bodies)), lambda: ac(None, 4, vp(bodies), vp(active)), lambda: de(None, 0, None),
                 lambda: ac(None, 0, None, None)):
        assert call() == ERR_INVALID
        assert "world" in _err(L)
    # n outside [0, 2^24]: reported before the pointers
    for n in (-1, (1 << 24) + 1):
        for call in (lambda: de(None, n, vp(bodies)), lambda: de(None, n, None), lambda: ac(None, n, vp(bodies), vp(active)),
                     lambda: ac(None, n, None, None)):
            assert call() == ERR_INVALID
            assert "n must" in _err(L)
    # null pointers with entries
    for call in (lambda: de(None, 1, None), lambda: ac(None, 1, None, vp(active)), lambda: ac(None, 1, vp(bodies), None)):
        assert call() == ERR_INVALID
        assert "null" in _err(L)
