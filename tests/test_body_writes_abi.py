"""CPU tests of the batched body writes' boundary (include/b2hip.h, block F: b2hip_apply_forces, b2hip_apply_impulses,
b2hip_set_velocities, b2hip_get_body_states_of): declared, exported, bound in Python, the record's layout, and argument
errors refused in the documented order before the world is looked at or any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_apply_forces", "b2hip_apply_impulses", "b2hip_set_velocities", "b2hip_get_body_states_of")
SINGLE = ("b2hip_apply_linear_impulse", "b2hip_apply_linear_impulse_to_center", "b2hip_apply_angular_impulse")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def test_header_declares_the_calls_and_the_record():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"\}\s*b2hip_body_push\s*;", text)
    assert "Definition by equivalence" in open(HDR).read()


def test_library_exports_the_calls():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_world_has_the_methods_and_the_record_is_32_bytes():
    for m in ("apply_forces", "apply_impulses", "set_velocities", "body_states_of", "apply_linear_impulse",
              "apply_linear_impulse_to_center", "apply_angular_impulse"):
        assert callable(getattr(b2hip.World, m, None)), m
    L = _lib()
    for name in NAMES + SINGLE:
        assert getattr(L, name).argtypes is not None, name
    t = b2hip.BODY_PUSH_DTYPE
    assert t.itemsize == 32
    assert t.names == ("x", "y", "angular", "at_point", "px", "py", "pad")
    assert [t.fields[n][1] for n in t.names] == [0, 4, 8, 12, 16, 20, 24]
    assert t.fields["at_point"][0] == np.dtype("i4") and t.fields["pad"][0].shape == (2,)
    # the C record, as compiled by the C compiler: the same size and offsets
    import shutil
    import subprocess
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.fail("no C compiler to check the header's layout")
    src = '#include "b2hip.h"\n#include <stddef.h>\n_Static_assert(sizeof(b2hip_body_push) == 32, "size");\n'
    for name in t.names:
        src += '_Static_assert(offsetof(b2hip_body_push, %s) == %d, "%s");\n' % (name, t.fields[name][1], name)
    src += "int main(void) { return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "push.c")
        open(path, "w").write(src)
        r = subprocess.run([cc, "-x", "c", "-std=c11", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_python_shapes_are_validated_and_scalars_broadcast():
    p = b2hip.World._pushes(3, (1.0, 2.0), 0.5, None, "force")
    assert p.dtype == b2hip.BODY_PUSH_DTYPE and p.shape == (3,)
    assert np.all(p["x"] == 1.0) and np.all(p["y"] == 2.0) and np.all(p["angular"] == 0.5) and not p["at_point"].any()
    p = b2hip.World._pushes(2, [[1.0, 2.0], [3.0, 4.0]], [5.0, 6.0], (7.0, 8.0), "impulse")
    assert p["x"].tolist() == [1.0, 3.0] and p["angular"].tolist() == [5.0, 6.0]
    assert p["at_point"].tolist() == [1, 1] and p["px"].tolist() == [7.0, 7.0] and p["py"].tolist() == [8.0, 8.0]
    with pytest.raises(ValueError):
        b2hip.World._pushes(3, [[1.0, 2.0]], 0.0, None, "force")
    with pytest.raises(ValueError):
        b2hip.World._pushes(3, (1.0, 2.0), [1.0, 2.0], None, "force")
    with pytest.raises(ValueError):
        b2hip.World._pushes(3, (1.0, 2.0), 0.0, [[1.0, 2.0, 3.0]] * 3, "force")
    w = b2hip.World.__new__(b2hip.World)  # (no world is needed to learn that nothing was asked for)
    w.p = None
    with pytest.raises(ValueError):
        w.set_velocities([0, 1])
    with pytest.raises(ValueError):
        w.set_velocities([[0, 1]], velocity=(1.0, 0.0))


def _err(L):
    msg = L.b2hip_last_error()
    assert msg, "no b2hip_last_error message"
    return msg.decode()


def test_null_world_and_bad_arguments_are_refused():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bodies = np.arange(4, dtype=np.int32)
    push = np.zeros(4, b2hip.BODY_PUSH_DTYPE)
    v3 = np.zeros((4, 3), np.float32)
    out = np.zeros(4, b2hip.BODY_STATE_DTYPE)
    forces, impulses, vels, states = L.b2hip_apply_forces, L.b2hip_apply_impulses, L.b2hip_set_velocities, L.b2hip_get_body_states_of
    # valid arguments, null world: the world is what is missing
    for call in (lambda: forces(None, 4, vp(bodies), vp(push), 1), lambda: impulses(None, 4, vp(bodies), vp(push), 0),
                 lambda: vels(None, 4, vp(bodies), vp(v3), 3), lambda: vels(None, 4, vp(bodies), vp(v3), 1),
                 lambda: vels(None, 4, vp(bodies), vp(v3), 2), lambda: states(None, 4, vp(bodies), vp(out)),
                 # (nothing to do, and still no world)
                 lambda: forces(None, 0, None, None, 1), lambda: impulses(None, 0, None, None, 1),
                 lambda: vels(None, 0, None, None, 3), lambda: states(None, 0, None, vp(out))):
        assert call() == ERR_INVALID
        assert "world" in _err(L)
    # n outside [0, 2^24]: reported before the pointers and the mask
    for n in (-1, (1 << 24) + 1):
        for call in (lambda: forces(None, n, vp(bodies), vp(push), 1), lambda: forces(None, n, None, None, 1),
                     lambda: impulses(None, n, vp(bodies), vp(push), 1), lambda: impulses(None, n, None, None, 1),
                     lambda: vels(None, n, vp(bodies), vp(v3), 3), lambda: vels(None, n, None, None, 0),
                     lambda: states(None, n, vp(bodies), vp(out)), lambda: states(None, n, None, None)):
            assert call() == ERR_INVALID
            assert "n must" in _err(L)
    # null pointers: before the mask
    for call in (lambda: forces(None, 4, None, vp(push), 1), lambda: forces(None, 4, vp(bodies), None, 1),
                 lambda: impulses(None, 4, None, vp(push), 1), lambda: impulses(None, 4, vp(bodies), None, 1),
                 lambda: vels(None, 4, None, vp(v3), 3), lambda: vels(None, 4, vp(bodies), None, 3),
                 lambda: vels(None, 4, None, vp(v3), 0), lambda: vels(None, 4, vp(bodies), None, 4),
                 lambda: states(None, 4, None, vp(out)), lambda: states(None, 4, vp(bodies), None),
                 lambda: states(None, 0, None, None)):
        assert call() == ERR_INVALID
        assert "null" in _err(L)
    # a mask other than 1, 2 or 3: before the world
    for mask in (0, 4, -1, 7):
        assert vels(None, 4, vp(bodies), vp(v3), mask) == ERR_INVALID
        assert "mask" in _err(L)
        assert vels(None, 0, None, None, mask) == ERR_INVALID
        assert "mask" in _err(L)
