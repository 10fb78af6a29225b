"""CPU tests of the batched shape queries' boundary (include/b2hip.h: b2hip_query_shapes, b2hip_shape_cast_closest):
declared, exported, bound in Python, laid out as the header says, and argument errors refused before any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_query_shapes", "b2hip_shape_cast_closest")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def test_header_declares_the_shape_queries():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    for typ in ("b2hip_shape_query", "b2hip_shape_cast"):
        assert re.search(r"}\s*%s\s*;" % typ, text), typ


def test_library_exports_the_shape_queries():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_world_has_the_shape_query_methods():
    for m in ("query_shapes", "shape_cast_closest"):
        assert callable(getattr(b2hip.World, m, None)), m
    assert b2hip.SHAPE_QUERY_DTYPE.itemsize == 16
    assert b2hip.SHAPE_CAST_DTYPE.itemsize == 32


def test_struct_sizes_match_the_header():
    """sizeof(b2hip_shape_query) == 16 and sizeof(b2hip_shape_cast) == 32, as compiled by the C compiler"""
    import shutil
    import subprocess
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.fail("no C compiler to check the header's layout")
    src = ('#include "b2hip.h"\n#include <stddef.h>\n'
           "_Static_assert(sizeof(b2hip_shape_query) == 16, \"query\");\n"
           "_Static_assert(sizeof(b2hip_shape_cast) == 32, \"cast\");\n"
           "_Static_assert(offsetof(b2hip_shape_cast, tx) == 16, \"tx\");\n"
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
    q = np.zeros(4, b2hip.SHAPE_QUERY_DTYPE)
    c = np.zeros(4, b2hip.SHAPE_CAST_DTYPE)
    q["shape"] = c["shape"] = [0, 1, 0, 1]
    c["tx"] = 1.0
    offsets = np.zeros(5, np.int32)
    items = np.zeros(16, b2hip.QUERY_ITEM_DTYPE)
    hits = np.zeros(4, b2hip.RAY_HIT_DTYPE)
    f = b2hip.QueryFilter(0xFFFF, 1)
    # valid arguments, null world
    assert L.b2hip_query_shapes(None, 2, sp, 4, vp(q), C.byref(f), 16, vp(offsets), vp(items)) == ERR_INVALID
    assert "world" in _err(L)
    assert L.b2hip_shape_cast_closest(None, 2, sp, 4, vp(c), None, vp(hits)) == ERR_INVALID
    assert "world" in _err(L)
    # n and n_shapes outside [0, 2^24]
    for n in (-1, (1 << 24) + 1):
        assert L.b2hip_query_shapes(None, 2, sp, n, vp(q), None, 16, vp(offsets), vp(items)) == ERR_INVALID
        assert "n must" in _err(L)
        assert L.b2hip_shape_cast_closest(None, 2, sp, n, vp(c), None, vp(hits)) == ERR_INVALID
        assert "n must" in _err(L)
        assert L.b2hip_query_shapes(None, n, sp, 4, vp(q), None, 16, vp(offsets), vp(items)) == ERR_INVALID
        assert "n_shapes" in _err(L)
        assert L.b2hip_shape_cast_closest(None, n, sp, 4, vp(c), None, vp(hits)) == ERR_INVALID
        assert "n_shapes" in _err(L)
    # NULL inputs and outputs, a negative cap
    assert L.b2hip_query_shapes(None, 2, sp, 4, vp(q), None, 16, None, vp(items)) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_query_shapes(None, 2, sp, 4, vp(q), None, 16, vp(offsets), None) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_query_shapes(None, 2, sp, 4, None, None, 16, vp(offsets), vp(items)) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_query_shapes(None, 2, None, 4, vp(q), None, 16, vp(offsets), vp(items)) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_shape_cast_closest(None, 2, sp, 4, vp(c), None, None) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_shape_cast_closest(None, 2, None, 4, vp(c), None, vp(hits)) == ERR_INVALID
    assert "null" in _err(L)
    assert L.b2hip_query_shapes(None, 2, sp, 4, vp(q), None, -1, vp(offsets), vp(items)) == ERR_INVALID
    assert "cap" in _err(L)
    # an unknown shape type, too many polygon vertices, a polygon of no vertex
    for typ, count, why in ((7, 0, "unknown shape type"), (b2hip.POLYGON, 9, "too many"), (b2hip.POLYGON, 0, "at least one")):
        bad = (b2hip.Shape * 2)(b2hip.circle_shape(0.5), b2hip.box_shape(0.5, 0.25))
        bad[1].type, bad[1].count = typ, count
        bp = C.cast(bad, C.c_void_p)
        assert L.b2hip_query_shapes(None, 2, bp, 4, vp(q), None, 16, vp(offsets), vp(items)) == ERR_INVALID
        assert why in _err(L) and "shape 1" in _err(L)
        assert L.b2hip_shape_cast_closest(None, 2, bp, 4, vp(c), None, vp(hits)) == ERR_INVALID
        assert why in _err(L)
    # a shape index outside [0, n_shapes)
    for k in (-1, 2):
        q2, c2 = q.copy(), c.copy()
        q2["shape"][3] = c2["shape"][3] = k
        assert L.b2hip_query_shapes(None, 2, sp, 4, vp(q2), None, 16, vp(offsets), vp(items)) == ERR_INVALID
        assert "query 3" in _err(L) and "shape index" in _err(L)
        assert L.b2hip_shape_cast_closest(None, 2, sp, 4, vp(c2), None, vp(hits)) == ERR_INVALID
        assert "shape index" in _err(L)
    # no shapes while queries name one
    assert L.b2hip_query_shapes(None, 0, None, 4, vp(q), None, 16, vp(offsets), vp(items)) == ERR_INVALID
    assert "shape index" in _err(L)


def test_python_shape_table_defaults():
    """one Shape serves every pose (index 0); a list of n Shapes is one per pose; a mismatch needs shape_index"""
    table, ns, idx = b2hip.World._shape_table(b2hip.circle_shape(1.0), 3, None)
    assert ns == 1 and idx.tolist() == [0, 0, 0]
    table, ns, idx = b2hip.World._shape_table([b2hip.circle_shape(1.0), b2hip.box_shape(1, 1)], 2, None)
    assert ns == 2 and idx.tolist() == [0, 1]
    with pytest.raises(ValueError):
        b2hip.World._shape_table([b2hip.circle_shape(1.0), b2hip.box_shape(1, 1)], 3, None)
    table, ns, idx = b2hip.World._shape_table([b2hip.circle_shape(1.0), b2hip.box_shape(1, 1)], 3, [1, 1, 0])
    assert idx.tolist() == [1, 1, 0] and table[1].type == b2hip.POLYGON
