"""GPU tests of the device-wide exclusive scan (box2d-mt_amd/csrc/b2d_scan.h: deviceExclusiveScan<int> and <int4>) against
np.cumsum in int64 (tests/prims_ref.py), through tests/probe/prims_probe.hip, which calls it exactly as the product does - the
live count in device memory, a ScanFlags that lives across calls - in all three forms: the single-pass look-back at 4 and at
16 items per thread and the three kernels, chosen by capacity alone.

Every case asserts three things: out[0 .. n] equals the reference exactly; every element beyond out[n] still holds the byte
0x5A the probe filled the array with; the epoch moved by 1 for a single-pass form and by 0 for the three kernels, which is
what proves that the case ran the form it was written for (tests/test_prims_ref_cpu.py labels the table)."""
import ctypes as C
import os

import numpy as np
import pytest

import b2hip
import prims_ref as pr
import probe_util as pu

pytestmark = pytest.mark.gpu

GUARD = 64  # elements of the output array beyond capN + 1


@pytest.fixture(scope="module")
def lib():
    """The probe of the integer primitives. No fallback: a missing library is a failure."""
    b2hip.use_torch_hip_runtime()  # one HIP runtime in the process, before anything that links libamdhip64 is loaded
    if not os.path.exists(pu.PRIMS_PROBE_LIB):
        pytest.fail("tests/probe/libprims_probe.so missing: run __graft_entry__.build() (make -C box2d-mt_amd all builds it "
                    "with the product's HIPFLAGS); there is no CPU stand-in for the device build")
    return pu.load_prims_probe()


class Scan:
    """One scan context, as a world has one scanCtx."""

    def __init__(self, lib, max_cap):
        self.lib = lib
        self.h = C.c_void_p()
        rc = lib.pprobe_scan_open(max_cap, C.byref(self.h))
        assert rc == 0, "pprobe_scan_open: HIP error %d" % rc

    @property
    def epoch(self):
        return self.lib.pprobe_scan_epoch(self.h)

    def set_epoch(self, value):
        assert self.lib.pprobe_scan_set_epoch(self.h, value) == 0

    def close(self):
        h, self.h = self.h, None
        if h:
            assert self.lib.pprobe_scan_close(h) == 0

    def check(self, cap_n, a, what, want=None):
        """Scans `a` with capacity cap_n and asserts the three things. `want`: the reference, where the caller shares one."""
        a = np.ascontiguousarray(a, np.int32)
        n = a.shape[0]
        elem_ints = 1 if a.ndim == 1 else 4
        out = np.zeros((cap_n + 1 + GUARD,) + a.shape[1:], np.int32)
        before = self.epoch
        rc = self.lib.pprobe_scan_run(self.h, elem_ints, cap_n, n, a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), GUARD)
        assert rc != self.lib.pprobe_scan_aborted_code(), "%s: a look-back gave up (SCAN_ABORT_BIT)" % what
        assert rc == 0, "%s: HIP error %d" % (what, rc)
        if want is None:
            want = pr.exclusive_scan(a)
        if not np.array_equal(out[:n + 1], want):
            bad = np.flatnonzero((out[:n + 1] != want).reshape(n + 1, -1).any(axis=1))
            pytest.fail("%s: %d of %d outputs differ, the first at %d (tile %d of 1 024): got %s, want %s" % (
                what, len(bad), n + 1, bad[0], bad[0] // 1024, out[bad[0]], want[bad[0]]))
        assert (out[n + 1:].view(np.uint32) == pr.FILL_WORD).all(), "%s: written beyond out[n]" % what
        after = before + pr.epoch_step(cap_n)
        if pr.epoch_step(cap_n) and before >= pr.EPOCH_LAST:
            after = 1  # (the flag words were zeroed and the count starts again)
        assert self.epoch == after, "%s: not the form the capacity asks for" % what


@pytest.fixture(scope="module")
def shared(lib):
    s = Scan(lib, max(c for c, _, _ in pr.SCAN_TABLE))
    yield s
    s.close()
    _inputs.clear()


_inputs = {}


def _input(pattern, n, elem_ints):
    """(input, reference), generated once per pattern and type at the largest count and cut: a prefix of a pattern is the
    pattern, and the scan of a prefix is a prefix of the scan"""
    key = (pattern, elem_ints)
    if key not in _inputs:
        a = pr.scan_input(pattern, max(n for _, n, _ in pr.SCAN_TABLE), elem_ints)
        want = pr.exclusive_scan(a)
        a.setflags(write=False)
        want.setflags(write=False)
        _inputs[key] = (a, want)
    a, want = _inputs[key]
    return a[:n], want[:n + 1]


@pytest.mark.parametrize("pattern", pr.SCAN_PATTERNS)
@pytest.mark.parametrize("elem_ints", [1, 4], ids=["int", "int4"])
@pytest.mark.parametrize("cap_n,n,form", pr.SCAN_TABLE, ids=["cap%d-n%d-%s" % row for row in pr.SCAN_TABLE])
def test_scan(shared, cap_n, n, form, elem_ints, pattern):
    a, want = _input(pattern, n, elem_ints)
    shared.check(cap_n, a, "%s %s capN %d n %d %s" % (form, "int4" if elem_ints == 4 else "int", cap_n, n, pattern), want)


def test_scan_probe_refuses_bad_arguments(lib):
    """n > capN, a capacity beyond the handle's, an element type that is neither: hipErrorInvalidValue (1), nothing launched."""
    s = Scan(lib, 4096)
    try:
        a = np.zeros(8192, np.int32)
        out = np.zeros(8192 + 1 + GUARD, np.int32)
        p, q = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        for elem_ints, cap_n, n, guard in ((1, 100, 101, GUARD), (1, 4097, 10, GUARD), (2, 100, 10, GUARD), (1, 0, 0, GUARD),
                                           (1, 100, -1, GUARD), (1, 100, 10, -1)):
            assert lib.pprobe_scan_run(s.h, elem_ints, cap_n, n, p, q, guard) == 1
        assert s.epoch == 0
    finally:
        s.close()


def test_scan_reuse_of_one_context(lib):
    """One handle: a 200-tile int scan, a 3-tile one, a 200-tile int4 scan, a 200-tile int scan of other data. The words an
    earlier, larger scan and the other element type left behind must not read as published."""
    s = Scan(lib, pr.STATE_N)
    try:
        for step, (elem_ints, tiles, pattern, seed) in enumerate(pr.REUSE_SEQUENCE):
            n = tiles * pr.SCAN_TILE
            s.check(n, pr.scan_input(pattern, n, elem_ints, seed), "reuse step %d (%s, %d tiles)" % (step, pattern, tiles))
        assert s.epoch == len(pr.REUSE_SEQUENCE)
    finally:
        s.close()


def test_scan_epoch_wrap(lib):
    """Three scans at epochs 1, 2, 3; the epoch set to 0x3ffffffd; three more, at 0x3ffffffe, at 0x3fffffff and - after the flag
    words were zeroed on the stream - at 1 again. Without the zeroing the last scan would meet the first one's status words."""
    s = Scan(lib, pr.STATE_N)
    try:
        for want, (pattern, seed) in zip((1, 2, 3), pr.WRAP_BEFORE):
            s.check(pr.STATE_N, pr.scan_input(pattern, pr.STATE_N, 1, seed), "before the wrap, epoch %d (%s)" % (want, pattern))
            assert s.epoch == want
        s.set_epoch(pr.EPOCH_LAST - 2)
        for want, (pattern, seed) in zip((pr.EPOCH_LAST - 1, pr.EPOCH_LAST, 1), pr.WRAP_AFTER):
            s.check(pr.STATE_N, pr.scan_input(pattern, pr.STATE_N, 1, seed), "around the wrap, epoch %#x (%s)" % (want, pattern))
            assert s.epoch == want
        assert s.epoch == 1
    finally:
        s.close()


def test_scan_epoch_wrap_over_rarely_used_tiles(lib):
    """The wrap as a world meets it: a large scan at epoch 1 (X, 200 tiles), then only small ones - epochs 2, 3, the epoch set
    to 0x3ffffffd, 0x3ffffffe, 0x3fffffff - and a large scan again (W), at epoch 1 after the wrap. The small scans rewrite the
    status words of their three tiles only, so tiles 3 .. 199 still say "prefix published at epoch 1" with X's prefixes behind
    them: only the zeroing of the flag words keeps W from taking them (in test_scan_epoch_wrap every scan in between rewrites
    every word with its own epoch, and nothing of epoch 1 is left to meet)."""
    s = Scan(lib, pr.STATE_N)
    small = pr.WRAP_SMALL_TILES * pr.SCAN_TILE
    try:
        s.check(pr.STATE_N, pr.scan_input(*pr.WRAP_BEFORE[0][:1], pr.STATE_N, 1, pr.WRAP_BEFORE[0][1]), "X at epoch 1")
        for want, (pattern, seed) in zip((2, 3), pr.WRAP_BEFORE[1:]):
            s.check(small, pr.scan_input(pattern, small, 1, seed), "small scan at epoch %d" % want)
            assert s.epoch == want
        s.set_epoch(pr.EPOCH_LAST - 2)
        for want, (pattern, seed) in zip((pr.EPOCH_LAST - 1, pr.EPOCH_LAST), pr.WRAP_AFTER[:2]):
            s.check(small, pr.scan_input(pattern, small, 1, seed), "small scan at epoch %#x" % want)
            assert s.epoch == want
        s.check(pr.STATE_N, pr.scan_input(*pr.WRAP_AFTER[2][:1], pr.STATE_N, 1, pr.WRAP_AFTER[2][1]), "W at epoch 1 after the wrap")
        assert s.epoch == 1
    finally:
        s.close()
