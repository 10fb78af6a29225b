"""CPU tests of the per-body contact calls' boundary (include/b2hip.h: b2hip_body_contacts, b2hip_body_contact_totals):
declared, exported, bound in Python, the records' layouts, and argument errors refused before the world is looked at or any
device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import b2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "b2hip.h")
NAMES = ("b2hip_body_contacts", "b2hip_body_contact_totals")
ERR_INVALID = -1


def _lib():
    if not os.path.exists(b2hip.LIB_PATH):
        pytest.fail("libb2hip.so missing: run __graft_entry__.build()")
    return b2hip.lib()


def test_header_declares_the_calls_and_their_records():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    for name in ("b2hip_body_contact", "b2hip_body_contact_total"):
        assert re.search(r"\}\s*%s\s*;" % name, text), name


def test_library_exports_the_calls():
    L = C.CDLL(b2hip.LIB_PATH) if os.path.exists(b2hip.LIB_PATH) else _lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_world_has_the_methods_and_the_records_are_32_bytes():
    for m in ("body_contacts", "body_contact_totals"):
        assert callable(getattr(b2hip.World, m, None)), m
    assert b2hip.BODY_CONTACT_DTYPE.itemsize == 32 and b2hip.BODY_CONTACT_TOTAL_DTYPE.itemsize == 32
    assert b2hip.BODY_CONTACT_DTYPE.names == ("contact_index", "other_body", "fixture", "other_fixture", "normal",
                                              "normal_impulse", "tangent_impulse")
    assert b2hip.BODY_CONTACT_TOTAL_DTYPE.names == ("contacts", "touching", "impulse", "normal_impulse", "max_normal_impulse",
                                                    "points", "pad")
    assert b2hip.BODY_CONTACT_DTYPE.fields["normal"][1] == 16 and b2hip.BODY_CONTACT_TOTAL_DTYPE.fields["points"][1] == 24


def _err(L):
    msg = L.b2hip_last_error()
    assert msg, "no b2hip_last_error message"
    return msg.decode()


def test_null_world_and_bad_arguments_are_refused():
    L = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bodies = np.arange(4, dtype=np.int32)
    offsets = np.zeros(5, np.int32)
    records = np.zeros(16, b2hip.BODY_CONTACT_DTYPE)
    out = np.zeros(4, b2hip.BODY_CONTACT_TOTAL_DTYPE)
    lists, totals = L.b2hip_body_contacts, L.b2hip_body_contact_totals
    # valid arguments, null world
    assert lists(None, 4, vp(bodies), 1, 16, vp(offsets), vp(records)) == ERR_INVALID
    assert "world" in _err(L)
    assert totals(None, 4, vp(bodies), vp(out)) == ERR_INVALID
    assert "world" in _err(L)
    assert lists(None, 0, None, 0, 0, vp(offsets), None) == ERR_INVALID  # (nothing to do, and still no world)
    assert "world" in _err(L)
    assert totals(None, 0, None, vp(out)) == ERR_INVALID
    assert "world" in _err(L)
    # n outside [0, 2^24]: the argument is reported, not the world - and before the cap and the pointers
    for n in (-1, (1 << 24) + 1):
        assert lists(None, n, vp(bodies), 1, 16, vp(offsets), vp(records)) == ERR_INVALID
        assert "n must" in _err(L)
        assert lists(None, n, None, 1, -1, None, None) == ERR_INVALID
        assert "n must" in _err(L)
        assert totals(None, n, vp(bodies), vp(out)) == ERR_INVALID
        assert "n must" in _err(L)
    # a negative cap, before the pointers
    assert lists(None, 4, vp(bodies), 1, -1, vp(offsets), vp(records)) == ERR_INVALID
    assert "cap" in _err(L)
    assert lists(None, 4, None, 1, -1, None, None) == ERR_INVALID
    assert "cap" in _err(L)
    # NULL bodies / offsets / records / out
    assert lists(None, 4, None, 1, 16, vp(offsets), vp(records)) == ERR_INVALID
    assert "null" in _err(L)
    assert lists(None, 4, vp(bodies), 1, 16, None, vp(records)) == ERR_INVALID
    assert "null" in _err(L)
    assert lists(None, 4, vp(bodies), 1, 16, vp(offsets), None) == ERR_INVALID
    assert "null" in _err(L)
    assert totals(None, 4, None, vp(out)) == ERR_INVALID
    assert "null" in _err(L)
    assert totals(None, 4, vp(bodies), None) == ERR_INVALID
    assert "null" in _err(L)
    # ... while NULL records with cap == 0 is a valid way to ask for the offsets alone: only the world is missing
    assert lists(None, 4, vp(bodies), 0, 0, vp(offsets), None) == ERR_INVALID
    assert "world" in _err(L)
