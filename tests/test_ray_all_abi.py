"""CPU tests of the all-hit / any-hit ray casts' boundary (include/b2hip.h: b2hip_ray_cast_all, b2hip_ray_cast_any): declared,
exported, bound in Python, and argument errors refused before the world is looked at or any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_ray_cast_all", "b2hip_ray_cast_any")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def test_header_declares_the_ray_casts():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_library_exports_the_ray_casts():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_world_has_the_ray_cast_methods():
    for m in ("ray_cast_all", "ray_cast_any"):
        assert callable(getattr(b2hip.World, m, None)), m


def _err(L):
    msg = L.b2hip_last_error()
    assert msg, "no b2hip_last_error message"
    return msg.decode()


def test_null_world_and_bad_arguments_are_refused():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rays = np.zeros((4, 4), np.float32)
    rays[:, 2] = 1.0
    offsets = np.zeros(5, np.int32)
    hits = np.zeros(16, b2hip.RAY_HIT_DTYPE)
    out = np.zeros(4, np.uint8)
    f = b2hip.QueryFilter(0xFFFF, 1)
    every, some = L.b2hip_ray_cast_all, L.b2hip_ray_cast_any
    # valid arguments, null world
    assert every(None, 4, vp(rays), C.byref(f), 16, vp(offsets), vp(hits)) == ERR_INVALID
    assert "world" in _err(L)
    assert some(None, 4, vp(rays), None, vp(out)) == ERR_INVALID
    assert "world" in _err(L)
    assert every(None, 0, None, None, 0, vp(offsets), None) == ERR_INVALID  # (nothing to do, and still no world)
    assert "world" in _err(L)
    # n outside [0, 2^24]: the argument is reported, not the world
    for n in (-1, (1 << 24) + 1):
        assert every(None, n, vp(rays), None, 16, vp(offsets), vp(hits)) == ERR_INVALID
        assert "n must" in _err(L)
        assert some(None, n, vp(rays), None, vp(out)) == ERR_INVALID
        assert "n must" in _err(L)
    # NULL rays / offsets / hits / out, a negative cap
    assert every(None, 4, None, None, 16, vp(offsets), vp(hits)) == ERR_INVALID
    assert "null" in _err(L)
    assert every(None, 4, vp(rays), None, 16, None, vp(hits)) == ERR_INVALID
    assert "null" in _err(L)
    assert every(None, 4, vp(rays), None, 16, vp(offsets), None) == ERR_INVALID
    assert "null" in _err(L)
    assert every(None, 4, vp(rays), None, -1, vp(offsets), vp(hits)) == ERR_INVALID
    assert "cap" in _err(L)
    assert some(None, 4, None, None, vp(out)) == ERR_INVALID
    assert "null" in _err(L)
    assert some(None, 4, vp(rays), None, None) == ERR_INVALID
    assert "null" in _err(L)
