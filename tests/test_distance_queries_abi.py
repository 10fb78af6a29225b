"""CPU tests of the batched distance queries' boundary (include/b2hip.h: b2hip_shape_distance_closest,
b2hip_query_shapes_within): declared, exported, bound in Python, laid out as the header says, and argument errors refused
before any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_shape_distance_closest", "b2hip_query_shapes_within")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def test_header_declares_the_distance_queries():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    for typ in ("b2hip_shape_range", "b2hip_distance_hit"):
        assert re.search(r"}\s*%s\s*;" % typ, text), typ


def test_library_exports_the_distance_queries():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_world_has_the_distance_query_methods():
    for m in ("shape_distance_closest", "query_shapes_within"):
        assert callable(getattr(b2hip.World, m, None)), m
    assert b2hip.SHAPE_RANGE_DTYPE.itemsize == 24
    assert b2hip.DISTANCE_HIT_DTYPE.itemsize == 32
    assert b2hip.SHAPE_RANGE_DTYPE.fields["max_distance"][1] == 16
    assert b2hip.DISTANCE_HIT_DTYPE.fields["distance"][1] == 24 and b2hip.DISTANCE_HIT_DTYPE.fields["iterations"][1] == 28


def test_struct_sizes_match_the_header():
    """sizeof(b2hip_shape_range) == 24 and sizeof(b2hip_distance_hit) == 32, as compiled by the C compiler"""
    import shutil
    import subprocess
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.fail("no C compiler to check the header's layout")
    src = ('#include "b2hip.h"\n#include <stddef.h>\n'
           "_Static_assert(sizeof(b2hip_shape_range) == 24, \"range\");\n"
           "_Static_assert(sizeof(b2hip_distance_hit) == 32, \"hit\");\n"
           "_Static_assert(offsetof(b2hip_shape_range, max_distance) == 16, \"max_distance\");\n"
           "_Static_assert(offsetof(b2hip_distance_hit, distance) == 24, \"distance\");\n"
           "int main(void) { return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sizes.c")
        open(path, "w").write(src)
        r = subprocess.run([cc, "-x", "c", "-std=c11", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _err(L):
    msg = L.b2hip_last_error()
    assert msg, "no b2hip_last_error message"
    return msg.decode()


def test_null_world_and_bad_arguments_are_refused():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    shapes = (b2hip.Shape * 2)(b2hip.circle_shape(0.5), b2hip.box_shape(0.5, 0.25))
    sp = C.cast(shapes, C.c_void_p)
    r = np.zeros(4, b2hip.SHAPE_RANGE_DTYPE)
    r["shape"] = [0, 1, 0, 1]
    r["max_distance"] = 2.0
    offsets = np.zeros(5, np.int32)
    hits = np.zeros(16, b2hip.DISTANCE_HIT_DTYPE)
    f = b2hip.QueryFilter(0xFFFF, 1)
    closest, within = L.b2hip_shape_distance_closest, L.b2hip_query_shapes_within
    # valid arguments, null world
    assert closest(None, 2, sp, 4, vp(r), C.byref(f), vp(hits)) == ERR_INVALID
    assert "world" in _err(L)
    assert within(None, 2, sp, 4, vp(r), None, 16, vp(offsets), vp(hits)) == ERR_INVALID
    assert "world" in _err(L)
    # n and n_shapes outside [0, 2^24]
    for n in (-1, (1 << 24) + 1):
        assert closest(None, 2, sp, n, vp(r), None, vp(hits)) == ERR_INVALID
        assert "n must" in _err(L)
        assert within(None, 2, sp, n, vp(r), None, 16, vp(offsets), vp(hits)) == ERR_INVALID
        assert "n must" in _err(L)
        assert closest(None, n, sp, 4, vp(r), None, vp(hits)) == ERR_INVALID
        assert "n_shapes" in _err(L)
        assert within(None, n, sp, 4, vp(r), None, 16, vp(offsets), vp(hits)) == ERR_INVALID
        assert "n_shapes" in _err(L)
    # NULL inputs and outputs, a negative cap
    assert closest(None, 2, sp, 4, vp(r), None, None) == ERR_INVALID
    assert "null" in _err(L)
    assert closest(None, 2, sp, 4, None, None, vp(hits)) == ERR_INVALID
    assert "null" in _err(L)
    assert closest(None, 2, None, 4, vp(r), None, vp(hits)) == ERR_INVALID
    assert "null" in _err(L)
    assert within(None, 2, sp, 4, vp(r), None, 16, None, vp(hits)) == ERR_INVALID
    assert "null" in _err(L)
    assert within(None, 2, sp, 4, vp(r), None, 16, vp(offsets), None) == ERR_INVALID
    assert "null" in _err(L)
    assert within(None, 2, sp, 4, None, None, 16, vp(offsets), vp(hits)) == ERR_INVALID
    assert "null" in _err(L)
    assert within(None, 2, None, 4, vp(r), None, 16, vp(offsets), vp(hits)) == ERR_INVALID
    assert "null" in _err(L)
    assert within(None, 2, sp, 4, vp(r), None, -1, vp(offsets), vp(hits)) == ERR_INVALID
    assert "cap" in _err(L)
    # an unknown shape type, too many polygon vertices, a polygon of no vertex
    for typ, count, why in ((7, 0, "unknown shape type"), (b2hip.POLYGON, 9, "too many"), (b2hip.POLYGON, 0, "at least one")):
        bad = (b2hip.Shape * 2)(b2hip.circle_shape(0.5), b2hip.box_shape(0.5, 0.25))
        bad[1].type, bad[1].count = typ, count
        bp = C.cast(bad, C.c_void_p)
        assert closest(None, 2, bp, 4, vp(r), None, vp(hits)) == ERR_INVALID
        assert why in _err(L) and "query shape 1" in _err(L)
        assert within(None, 2, bp, 4, vp(r), None, 16, vp(offsets), vp(hits)) == ERR_INVALID
        assert why in _err(L) and "query shape 1" in _err(L)
    # a shape index outside [0, n_shapes)
    for k in (-1, 2):
        r2 = r.copy()
        r2["shape"][3] = k
        assert closest(None, 2, sp, 4, vp(r2), None, vp(hits)) == ERR_INVALID
        assert "query 3" in _err(L) and "shape index" in _err(L)
        assert within(None, 2, sp, 4, vp(r2), None, 16, vp(offsets), vp(hits)) == ERR_INVALID
        assert "query 3" in _err(L) and "shape index" in _err(L)
    # no shapes while queries name one
    assert closest(None, 0, None, 4, vp(r), None, vp(hits)) == ERR_INVALID
    assert "shape index" in _err(L)
    assert within(None, 0, None, 4, vp(r), None, 16, vp(offsets), vp(hits)) == ERR_INVALID
    assert "shape index" in _err(L)


def test_python_ranges_take_a_scalar_or_one_distance_per_pose():
    poses = np.zeros((3, 3), np.float32)
    r, ns, _ = b2hip.World._ranges(b2hip.circle_shape(1.0), poses, 2.5, None)
    assert ns == 1 and r["max_distance"].tolist() == [2.5, 2.5, 2.5] and r["shape"].tolist() == [0, 0, 0]
    r, ns, _ = b2hip.World._ranges(b2hip.circle_shape(1.0), poses, [1.0, 2.0, 3.0], None)
    assert r["max_distance"].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        b2hip.World._ranges(b2hip.circle_shape(1.0), poses, [1.0, 2.0], None)
