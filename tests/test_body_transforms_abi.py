"""CPU tests of the batched teleports' and sleep / wake sets' boundary (include/b2hip.h, block H: b2hip_set_transforms,
b2hip_set_awakes): declared with their definition by equivalence, exported, bound in Python beside the single
b2hip_set_transform, and argument errors refused in the documented order before the world is looked at or any device is
needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_set_transforms", "b2hip_set_awakes")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def test_header_declares_the_calls_and_defines_them_by_equivalence():
    whole = open(HDR).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    assert re.search(r"\bint\s+b2hip_set_transforms\s*\(\s*b2hip_world\s*\*\s*w\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*bodies\s*,"
                     r"\s*const\s+float\s*\*\s*pose3\s*,\s*int\s+mask\s*\)", text)
    assert re.search(r"\bint\s+b2hip_set_awakes\s*\(\s*b2hip_world\s*\*\s*w\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*bodies\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*awake\s*\)", text)
    block = whole[whole.index("---- H. Batched teleports"):]
    assert "Definition by equivalence" in block
    for word in ("b2hip_set_transform(w, b, x', y', a')", "b2hip_set_awake(w, b, awake[i] != 0)", "move buffer", "B2HIP_ERR_UNSUPPORTED",
                 "AT MOST ONCE", "inactive body"):
        assert word in block, word
    # the function map at the head of the file
    assert "b2hip_set_transforms / _awakes" in whole[:whole.index("#ifndef B2HIP_H")]


def test_library_exports_the_calls():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES + ("b2hip_set_transform", "b2hip_set_awake"):
        assert hasattr(L, name), name


def test_python_world_has_the_methods_with_argtypes():
    for m in ("set_transforms", "set_awakes", "set_transform", "set_awake"):
        assert callable(getattr(b2hip.World, m, None)), m
    L = _lib()
    for name in NAMES + ("b2hip_set_transform",):
        assert getattr(L, name).argtypes is not None, name
    assert list(L.b2hip_set_transform.argtypes) == [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    assert len(L.b2hip_set_transforms.argtypes) == 5 and len(L.b2hip_set_awakes.argtypes) == 4


def test_python_shapes_are_validated():
    w = b2hip.World.__new__(b2hip.World)  # (no world is needed to learn that nothing was asked for)
    w.p = None
    with pytest.raises(ValueError):
        w.set_transforms([0, 1])
    with pytest.raises(ValueError):
        w.set_transforms([0, 1], position=[[1.0, 2.0]])
    with pytest.raises(ValueError):
        w.set_transforms([0, 1], angle=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        w.set_transforms([[0, 1]], position=(1.0, 0.0))
    with pytest.raises(ValueError):
        w.set_awakes([0, 1], [True, False, True])


def _err(L):
    msg = L.b2hip_last_error()
    assert msg, "no b2hip_last_error message"
    return msg.decode()


def test_null_world_and_bad_arguments_are_refused_in_order():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bodies = np.arange(4, dtype=np.int32)
    pose3 = np.zeros((4, 3), np.float32)
    awake = np.ones(4, np.uint8)
    xf, aw = L.b2hip_set_transforms, L.b2hip_set_awakes
    # valid arguments, null world: the world is what is missing
    for call in (lambda: xf(None, 4, vp(bodies), vp(pose3), 1), lambda: xf(None, 4, vp(bodies), vp(pose3), 2),
                 lambda: xf(None, 4, vp(bodies), vp(pose3), 3), lambda: aw(None, 4, vp(bodies), vp(awake)),
                 # (nothing to do, and still no world)
                 lambda: xf(None, 0, None, None, 3), lambda: aw(None, 0, None, None)):
        assert call() == ERR_INVALID
        assert "world" in _err(L)
    # n outside [0, 2^24]: reported before the pointers and the mask
    for n in (-1, (1 << 24) + 1):
        for call in (lambda: xf(None, n, vp(bodies), vp(pose3), 3), lambda: xf(None, n, None, None, 0),
                     lambda: aw(None, n, vp(bodies), vp(awake)), lambda: aw(None, n, None, None)):
            assert call() == ERR_INVALID
            assert "n must" in _err(L)
    # null pointers with n > 0: before the mask
    for call in (lambda: xf(None, 4, None, vp(pose3), 3), lambda: xf(None, 4, vp(bodies), None, 3),
                 lambda: xf(None, 4, None, vp(pose3), 0), lambda: xf(None, 4, vp(bodies), None, 4),
                 lambda: aw(None, 4, None, vp(awake)), lambda: aw(None, 4, vp(bodies), None)):
        assert call() == ERR_INVALID
        assert "null" in _err(L)
    # a mask other than 1, 2 or 3: before the world
    for mask in (0, 4, -1, 7):
        assert xf(None, 4, vp(bodies), vp(pose3), mask) == ERR_INVALID
        assert "mask" in _err(L)
        assert xf(None, 0, None, None, mask) == ERR_INVALID
        assert "mask" in _err(L)
