"""CPU tests of the batched joint calls' boundary (include/b2hip.h, block G: b2hip_joint_count, b2hip_joint_is_destroyed,
b2hip_joint_set_motors, b2hip_get_joint_states): declared, exported, bound in Python, the records' layout, argument errors
refused in the documented order before the world is looked at or any device is needed, and Python's broadcasting."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_joint_count", "b2hip_joint_is_destroyed", "b2hip_joint_set_motors", "b2hip_get_joint_states")
SINGLE = ("b2hip_get_joint_reaction", "b2hip_get_joint_limit_state")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def test_header_declares_the_calls_and_the_records():
    whole = open(HDR).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"\}\s*b2hip_joint_motor\s*;", text)
    assert re.search(r"\}\s*b2hip_joint_state\s*;", text)
    assert "G. Batched joints" in whole


def test_library_exports_the_calls():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_binds_the_calls_and_the_records_match_the_c_layout():
    for m in ("joint_set_motors", "joint_states", "joint_reaction", "joint_limit_state", "joint_is_destroyed"):
        assert callable(getattr(b2hip.World, m, None)), m
    assert isinstance(b2hip.World.joint_count, property)
    L = _lib()
    for name in NAMES + SINGLE:
        assert getattr(L, name).argtypes is not None, name
    m, s = b2hip.JOINT_MOTOR_DTYPE, b2hip.JOINT_STATE_DTYPE
    assert m.itemsize == 16 and s.itemsize == 48
    assert m.names == ("enable_motor", "motor_speed", "max_motor", "pad")
    assert s.names == ("type", "limit_state", "coordinate", "speed", "coordinate2", "speed2", "force", "torque", "motor", "pad")
    assert [m.fields[n][1] for n in m.names] == [0, 4, 8, 12]
    assert [s.fields[n][1] for n in s.names] == [0, 4, 8, 12, 16, 20, 24, 32, 36, 40]
    assert m.fields["enable_motor"][0] == np.dtype("i4") and s.fields["type"][0] == np.dtype("i4")
    assert s.fields["limit_state"][0] == np.dtype("i4") and s.fields["force"][0].shape == (2,) and s.fields["pad"][0].shape == (2,)
    # the C records, as compiled by the C compiler: the same sizes and offsets
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.fail("no C compiler to check the header's layout")
    src = '#include "b2hip.h"\n#include <stddef.h>\n'
    for record, t in (("b2hip_joint_motor", m), ("b2hip_joint_state", s)):
        src += '_Static_assert(sizeof(%s) == %d, "size of %s");\n' % (record, t.itemsize, record)
        for name in t.names:
            src += '_Static_assert(offsetof(%s, %s) == %d, "%s.%s");\n' % (record, name, t.fields[name][1], record, name)
    src += "int main(void) { return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "joint_records.c")
        open(path, "w").write(src)
        r = subprocess.run([cc, "-x", "c", "-std=c11", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _err(L):
    msg = L.b2hip_last_error()
    assert msg, "no b2hip_last_error message"
    return msg.decode()


def test_null_world_and_bad_arguments_are_refused_in_order():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    joints = np.arange(4, dtype=np.int32)
    motors = np.zeros(4, b2hip.JOINT_MOTOR_DTYPE)
    out = np.zeros(4, b2hip.JOINT_STATE_DTYPE)
    write, read = L.b2hip_joint_set_motors, L.b2hip_get_joint_states
    assert L.b2hip_joint_count(None) == 0
    assert L.b2hip_joint_is_destroyed(None, 0) == 0
    # valid arguments, null world: the world is what is missing
    for call in [lambda mask=mask: write(None, 4, vp(joints), vp(motors), mask) for mask in range(1, 8)] + [
            lambda: read(None, 4, vp(joints), 60.0, vp(out)),
            # (nothing to do, and still no world)
            lambda: write(None, 0, None, None, 7), lambda: read(None, 0, None, 60.0, vp(out))]:
        assert call() == ERR_INVALID
        assert "world" in _err(L)
    # 1. n outside [0, 2^24]: reported before the pointers and the mask
    for n in (-1, (1 << 24) + 1):
        for call in (lambda: write(None, n, vp(joints), vp(motors), 2), lambda: write(None, n, None, None, 0),
                     lambda: read(None, n, vp(joints), 60.0, vp(out)), lambda: read(None, n, None, 60.0, None)):
            assert call() == ERR_INVALID
            assert "n must" in _err(L)
    # 2. null pointers (inputs when n > 0, the output always): before the mask
    for call in (lambda: write(None, 4, None, vp(motors), 2), lambda: write(None, 4, vp(joints), None, 2),
                 lambda: write(None, 4, None, vp(motors), 0), lambda: write(None, 4, vp(joints), None, 8),
                 lambda: read(None, 4, None, 60.0, vp(out)), lambda: read(None, 4, vp(joints), 60.0, None),
                 lambda: read(None, 0, None, 60.0, None)):
        assert call() == ERR_INVALID
        assert "null" in _err(L)
    # 3. a mask outside 1..7: before the world
    for mask in (0, 8, -1, 15):
        assert write(None, 4, vp(joints), vp(motors), mask) == ERR_INVALID
        assert "mask" in _err(L)
        assert write(None, 0, None, None, mask) == ERR_INVALID
        assert "mask" in _err(L)


def test_python_broadcasts_scalars_and_derives_the_mask():
    W = b2hip.World
    m, mask = W._joint_motors(3, 1.5, None, None)
    assert m.dtype == b2hip.JOINT_MOTOR_DTYPE and m.shape == (3,) and mask == 2
    assert np.all(m["motor_speed"] == 1.5) and not m["enable_motor"].any() and not m["max_motor"].any()
    m, mask = W._joint_motors(3, [1.0, 2.0, 3.0], 40.0, None)
    assert mask == 6 and m["motor_speed"].tolist() == [1.0, 2.0, 3.0] and np.all(m["max_motor"] == 40.0)
    m, mask = W._joint_motors(2, None, None, [True, False])
    assert mask == 1 and m["enable_motor"].tolist() == [1, 0]
    m, mask = W._joint_motors(2, 0.0, [5.0, 6.0], True)
    assert mask == 7 and m["enable_motor"].tolist() == [1, 1] and m["max_motor"].tolist() == [5.0, 6.0]
    m, mask = W._joint_motors(2, None, 9.0, 5)  # (any non-zero enable is 1)
    assert mask == 5 and m["enable_motor"].tolist() == [1, 1]
    with pytest.raises(ValueError):
        W._joint_motors(3, None, None, None)
    with pytest.raises(ValueError):
        W._joint_motors(3, [1.0, 2.0], None, None)
    with pytest.raises(ValueError):
        W._joint_motors(3, 1.0, [[1.0, 2.0, 3.0]], None)
    w = W.__new__(W)  # (no world is needed to learn that the arguments do not go together)
    w.p = None
    records = np.zeros(2, b2hip.JOINT_MOTOR_DTYPE)
    with pytest.raises(ValueError):
        w.joint_set_motors([0, 1], records)  # a record array needs mask=
    with pytest.raises(ValueError):
        w.joint_set_motors([0, 1], records, max_motor=1.0, mask=2)
    with pytest.raises(ValueError):
        w.joint_set_motors([0, 1, 2], records, mask=2)
    with pytest.raises(ValueError):
        w.joint_set_motors([0, 1], 1.0, mask=2)  # mask= goes with records only
    with pytest.raises(ValueError):
        w.joint_set_motors([[0, 1]], 1.0)
    with pytest.raises(ValueError):
        w.joint_set_motors([0, 1])
