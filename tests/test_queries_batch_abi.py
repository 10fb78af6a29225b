"""CPU tests of the batched device queries' boundary (include/b2hip.h: b2hip_query_aabbs, b2hip_query_points,
b2hip_ray_cast_closest): declared, exported, bound in Python, and argument errors refused before any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_query_aabbs", "b2hip_query_points", "b2hip_ray_cast_closest")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def test_header_declares_the_batched_queries():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    for typ in ("b2hip_query_filter", "b2hip_query_item", "b2hip_ray_hit"):
        assert re.search(r"}\s*%s\s*;" % typ, text), typ


def test_library_exports_the_batched_queries():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_world_has_the_query_methods():
    for m in ("query_aabbs", "query_points", "ray_cast_closest"):
        assert callable(getattr(b2hip.World, m, None)), m
    assert b2hip.RAY_HIT_DTYPE.itemsize == 32 and b2hip.QUERY_ITEM_DTYPE.itemsize == 8
    assert C.sizeof(b2hip.QueryFilter) == 8


def _err(L):
    msg = L.b2hip_last_error()
    assert msg, "no b2hip_last_error message"
    return msg.decode()


def test_null_world_and_bad_arguments_are_refused():
    L = _lib()
    boxes = np.zeros((4, 4), np.float32)
    offsets = np.zeros(5, np.int32)
    items = np.zeros(16, b2hip.QUERY_ITEM_DTYPE)
    hits = np.zeros(4, b2hip.RAY_HIT_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    f = b2hip.QueryFilter(0xFFFF, 1)
    # null world
    assert L.b2hip_query_aabbs(None, 4, vp(boxes), C.byref(f), 16, vp(offsets), vp(items)) == ERR_INVALID
    assert "world" in _err(L)
    assert L.b2hip_query_points(None, 4, vp(boxes), None, 16, vp(offsets), vp(items)) == ERR_INVALID
    assert "world" in _err(L)
    assert L.b2hip_ray_cast_closest(None, 4, vp(boxes), None, vp(hits)) == ERR_INVALID
    assert "world" in _err(L)
    # n < 0 and n > 2^24 (checked before the world is looked at)
    for n in (-1, (1 << 24) + 1):
        assert L.b2hip_query_aabbs(None, n, vp(boxes), None, 16, vp(offsets), vp(items)) == ERR_INVALID
        assert "n must" in _err(L)
        assert L.b2hip_query_points(None, n, vp(boxes), None, 16, vp(offsets), vp(items)) == ERR_INVALID
        assert "n must" in _err(L)
        assert L.b2hip_ray_cast_closest(None, n, vp(boxes), None, vp(hits)) == ERR_INVALID
        assert "n must" in _err(L)
    # NULL outputs
    assert L.b2hip_query_aabbs(None, 4, vp(boxes), None, 16, None, vp(items)) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_query_points(None, 4, vp(boxes), None, 16, vp(offsets), None) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_ray_cast_closest(None, 4, vp(boxes), None, None) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_query_aabbs(None, 4, vp(boxes), None, -1, vp(offsets), vp(items)) == ERR_INVALID
