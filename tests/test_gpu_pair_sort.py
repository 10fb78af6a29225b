"""GPU: the pair update's stable LSD radix sort with one launch per pass (box2d-mt_amd/csrc/b2d_scan.h: k_radix_prepare +
k_radix_onepass) against numpy's stable argsort on the same bits, through b2hip_test_radix_sort, and against the three-launch
passes (B2HIP_SORT_ONEPASS=0) in whole steps. A stable LSD sort has one correct output: keys and payloads are compared exactly.

Counts: the edges of a tile, several tiles, 70 tiles (the last tile reads group sums of four groups and 5 counts of its own
group), and the two sides of RADIX_ONEPASS_MAX_TILES, where the sort falls back to the three-launch form."""
import ctypes as C
import os

import numpy as np
import pytest

import b2harness as bh
import b2hip

pytestmark = pytest.mark.gpu

RADIX_TILE = 2048
RADIX_BITS = 11
RADIX_MAX_PASSES = 6
ONEPASS_MAX_TILES = 1024


def radix_passes(first, bits):
    """radixPasses of b2hip_host_phases.h"""
    passes = (bits + RADIX_BITS - 1) // RADIX_BITS
    out, at = [], 0
    for p in range(passes):
        width = (bits - at + (passes - p) - 1) // (passes - p)
        out.append((first + at, width))
        at += width
    return out


LAYOUTS = {"width1": [(0, 1), (1, 1), (2, 1)],
           "width11": [(0, RADIX_BITS), (RADIX_BITS, RADIX_BITS)],
           "halves17": radix_passes(0, 17) + radix_passes(32, 17),
           "halves21": radix_passes(0, 21) + radix_passes(32, 21)}
COUNTS = [0, 1, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1, 3 * RADIX_TILE + 7, 70 * RADIX_TILE,
          (ONEPASS_MAX_TILES - 1) * RADIX_TILE + 5, ONEPASS_MAX_TILES * RADIX_TILE + 5]
PATTERNS = ("random", "equal", "two_digits", "sorted", "reversed", "duplicates")


def make_keys(pattern, n, layout, rng):
    used = np.uint64(0)
    for shift, width in layout:
        used |= np.uint64(((1 << width) - 1) << shift)
    if pattern == "random":
        return rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    if pattern == "equal":
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if pattern == "two_digits":
        # two values that differ in the lowest bit of every pass: two distinct digits per pass
        low = np.uint64(0)
        for shift, _ in layout:
            low |= np.uint64(1 << shift)
        return np.where(rng.integers(0, 2, n) == 1, low, np.uint64(0)).astype(np.uint64)
    if pattern == "duplicates":
        return rng.integers(0, 7, n, dtype=np.uint64) * np.uint64(0x0000020100000201)
    # sorted / reversed by the bits the passes look at, most significant pass last
    k = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    order = reference_order(k, layout)
    k = k[order]
    return k[::-1].copy() if pattern == "reversed" else k


def reference_order(keys, layout):
    order = np.arange(len(keys))
    for shift, width in layout:
        digit = ((keys[order] >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int32)
        order = order[np.argsort(digit, kind="stable")]
    return order


def _stats(w):
    out = (C.c_longlong * 2)()
    assert w.L.b2hip_debug_read(w.p, 22, 0, 2, out) == 0
    return out[0], out[1]


@pytest.fixture(scope="module")
def worlds():
    L = b2hip.lib()
    L.b2hip_test_radix_sort.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.b2hip_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    saved = os.environ.pop("B2HIP_SORT_ONEPASS", None)
    try:
        on = b2hip.World()
        os.environ["B2HIP_SORT_ONEPASS"] = "0"
        off = b2hip.World()
    finally:
        os.environ.pop("B2HIP_SORT_ONEPASS", None)
        if saved is not None:
            os.environ["B2HIP_SORT_ONEPASS"] = saved
    yield {"on": on, "off": off}
    on.close()
    off.close()


def device_sort(w, keys, vals, layout):
    k, v = keys.copy(), vals.copy()
    shifts = np.array([s for s, _ in layout], np.int32)
    widths = np.array([x for _, x in layout], np.int32)
    rc = w.L.b2hip_test_radix_sort(w.p, len(k), k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), len(layout),
                                   shifts.ctypes.data_as(C.c_void_p), widths.ctypes.data_as(C.c_void_p))
    assert rc == 0, w.L.b2hip_last_error()
    return k, v


@pytest.mark.parametrize("layout_name", sorted(LAYOUTS))
@pytest.mark.parametrize("n", COUNTS)
def test_sort_matches_a_stable_argsort(worlds, n, layout_name):
    layout = LAYOUTS[layout_name]
    rng = np.random.default_rng(1000 + n % 9973)
    fits = n // RADIX_TILE + 1 <= ONEPASS_MAX_TILES and len(layout) <= RADIX_MAX_PASSES
    for pattern in PATTERNS:
        keys = make_keys(pattern, n, layout, rng)
        vals = np.stack([np.arange(n, dtype=np.int32), rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32)], axis=1)
        vals = np.ascontiguousarray(vals)
        order = reference_order(keys, layout)
        want_k, want_v = keys[order], vals[order]
        for switch in ("on", "off"):
            w = worlds[switch]
            sorts0, one0 = _stats(w)
            got_k, got_v = device_sort(w, keys, vals, layout)
            sorts1, one1 = _stats(w)
            assert sorts1 == sorts0 + 1
            assert one1 - one0 == (1 if (switch == "on" and fits) else 0), (switch, n, layout_name)
            assert np.array_equal(got_k, want_k), (switch, pattern, n, layout_name)
            assert np.array_equal(got_v, want_v), (switch, pattern, n, layout_name)


def _hashes(hw):
    dw = hw.device_world()
    L = b2hip.lib()
    L.b2hip_debug_hash.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    out = []
    for which in (0, 1, 2):
        h = C.c_uint64()
        assert L.b2hip_debug_hash(dw, which, C.byref(h)) == 0
        out.append(h.value)
    return out


def _device_stats(hw):
    L = b2hip.lib()
    L.b2hip_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out = (C.c_longlong * 2)()
    assert L.b2hip_debug_read(hw.device_world(), 22, 0, 2, out) == 0
    return out[0], out[1]


def test_whole_steps_equal_the_three_launch_passes(amd, monkeypatch):
    """Tumbler 60 x 60 from its start grid: every proxy moves at the start, so the pair update sorts with the radix passes."""
    monkeypatch.delenv("B2HIP_SORT_ONEPASS", raising=False)
    a = amd.world(bh.TUMBLER, p0=60)
    monkeypatch.setenv("B2HIP_SORT_ONEPASS", "0")
    b = amd.world(bh.TUMBLER, p0=60)
    monkeypatch.delenv("B2HIP_SORT_ONEPASS", raising=False)
    for k in range(12):
        a.step(10)
        b.step(10)
        assert _hashes(a) == _hashes(b), "after %d steps" % (10 * (k + 1))
    sorts_a, one_a = _device_stats(a)
    sorts_b, one_b = _device_stats(b)
    assert one_a > 0, "no one-launch sort ran in %d sorts" % sorts_a
    assert sorts_b == sorts_a and one_b == 0
    a.close()
    b.close()
