"""GPU tests of the wave64 and workgroup aggregation helpers of box2d-mt_amd/csrc/b2d_wave.h, one kernel per helper in
tests/probe/prims_probe.hip, against the numpy references of tests/prims_ref.py: the five waveAtomic*, blockMaxU32Offer /
Flush, blockAtomicMaxIfAbove, blockHot*, blockAlloc, waveKeyedAlloc, waveRunAlloc, waveKeyedAllocOnce, blockKeyedAlloc65.

Every helper runs with 64, 192, 256 and 1024 threads per workgroup (blockKeyedAlloc65, which needs 65 threads: 128, 256,
1024), one and seven workgroups, and element counts that are a multiple of the block size, n % 64 == 1 and n % 64 == 63
(threads beyond n call with valid = false), over the key patterns of prims_ref.WAVE_PATTERNS - what each holds is checked on
the CPU by tests/test_prims_ref_cpu.py. Every assertion is exact: the final array against np.add.at / minimum.at /
maximum.at in the right signedness, and for the allocators the three properties of prims_ref.check_alloc."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import b2hip
import prims_ref as pr
import probe_util as pu

pytestmark = pytest.mark.gpu

ip = C.POINTER(C.c_int)
up = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    """The probe of the integer primitives. No fallback: a missing library is a failure."""
    b2hip.use_torch_hip_runtime()  # one HIP runtime in the process, before anything that links libamdhip64 is loaded
    if not os.path.exists(pu.PRIMS_PROBE_LIB):
        pytest.fail("tests/probe/libprims_probe.so missing: run __graft_entry__.build() (make -C box2d-mt_amd all builds it "
                    "with the product's HIPFLAGS); there is no CPU stand-in for the device build")
    return pu.load_prims_probe()


@functools.lru_cache(maxsize=None)
def _pattern(name, n, rounds, nkeys=pr.NKEYS, block=64):
    """prims_ref.wave_pattern, made once per case and shared by the helpers (read-only)"""
    key, valid = pr.wave_pattern(name, n, rounds, nkeys=nkeys, block=block)
    key.setflags(write=False)
    valid.setflags(write=False)
    return key, valid


def _call(lib, helper, block, grid, key, val, valid, base0, p0=0, p1=0):
    """-> (return code, final array in base0's type, slots [rounds, n])"""
    rounds, n = key.shape
    key = np.ascontiguousarray(key, np.int32)
    valid = np.ascontiguousarray(valid, np.int32)
    bits = np.ascontiguousarray(val).view(np.uint32).reshape(rounds, n)
    base = np.ascontiguousarray(base0).view(np.uint32).copy()
    slots = np.full((rounds, n), -1, np.int32)
    rc = lib.pprobe_wave(pr.OPS[helper], block, grid, rounds, n, key.ctypes.data_as(ip), bits.ctypes.data_as(up),
                         valid.ctypes.data_as(ip), base.ctypes.data_as(up), len(base), slots.ctypes.data_as(ip), p0, p1)
    return rc, base.view(base0.dtype), slots


def _run(lib, helper, block, grid, key, val, valid, base0, p0=0, p1=0):
    rc, base1, slots = _call(lib, helper, block, grid, key, val, valid, base0, p0, p1)
    assert rc == 0, "%s: HIP error %d" % (helper, rc)
    return base1, slots


# helper -> (rounds, kind of value, kind of initial contents, how the offers combine)
AGGREGATES = {
    "waveAtomicAddInt": (2, "sum", "count", "add"),
    "waveAtomicMinInt": (2, "i32", "i32", "min"),
    "waveAtomicMaxU32": (2, "u32", "u32", "max"),
    "waveAtomicMaxU32Guarded": (2, "u32", "u32", "max"),
    "waveAtomicMinU32": (2, "u32", "u32", "min"),
    "blockMaxU32": (3, "u32", "u32", "max"),
    "blockHot": (4, "sum", "count", "add"),
}
EXTRA_PATTERNS = {"blockMaxU32": pr.BLOCK_PATTERNS[:5], "blockHot": pr.BLOCK_PATTERNS[5:]}
SHAPES = [(b, g) for b in pr.BLOCKS for g in pr.GRIDS]
SHAPE_IDS = ["block%d-grid%d" % s for s in SHAPES]


def _aggregate_cases():
    for helper in AGGREGATES:
        for name in pr.WAVE_PATTERNS + EXTRA_PATTERNS.get(helper, ()):
            yield helper, name


@pytest.mark.parametrize("block,grid", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("helper,pattern", list(_aggregate_cases()))
def test_aggregate(lib, helper, pattern, block, grid):
    rounds, vkind, bkind, how = AGGREGATES[helper]
    for seed, n in enumerate(pr.launch_counts(block, grid)):
        key, valid = _pattern(pattern, n, rounds, block=block)
        val = pr.wave_values(vkind, (rounds, n), seed)
        base0 = pr.initial_base(bkind, pr.NKEYS, seed)
        base1, _ = _run(lib, helper, block, grid, key, val, valid, base0)
        want = pr.ref_aggregate(how, base0, key, val, valid)
        bad = np.flatnonzero(base1 != want)
        assert not len(bad), "%s %s n %d: keys %s hold %s, want %s (from %s)" % (
            helper, pattern, n, bad[:6], base1[bad[:6]], want[bad[:6]], base0[bad[:6]])


@pytest.mark.parametrize("block,grid", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("case", pr.MAX_IF_ABOVE_CASES)
def test_block_atomic_max_if_above(lib, case, block, grid):
    """Two calls on one word (the scratch of the first is reused by the second: the trailing barrier). The stored value lies
    below, among and above the offers."""
    for n in pr.launch_counts(block, grid):
        val = pr.max_if_above_values(case, n, 2, block)
        key = np.zeros((2, n), np.int32)
        for pattern in ("all_same", "holes", "only_lane63", "none_valid"):
            _, valid = _pattern(pattern, n, 2, block=block)
            for start in (0, 500000, pr.MAX_IF_ABOVE_TOP + 1, -7):
                base0 = np.array([start], np.int32)
                base1, _ = _run(lib, "blockAtomicMaxIfAbove", block, grid, key, val, valid, base0)
                want = pr.ref_max_if_above(base0, val, valid)
                assert base1[0] == want[0], "%s %s n %d from %d: %d, want %d" % (case, pattern, n, start, base1[0], want[0])
                if case == "all_nonpositive":
                    assert base1[0] == start


def _check_alloc(lib, helper, block, grid, key, valid, word, base0, what, p0=0, p1=0, fetch=True):
    val = np.zeros(key.shape, np.uint32)
    base1, slots = _run(lib, helper, block, grid, key, val, valid, base0, p0, p1)
    try:
        pr.check_alloc(helper, base0, base1, word, key, valid, slots, block, fetch=fetch)
    except AssertionError as e:
        raise AssertionError("%s %s: %s" % (helper, what, e)) from None


@pytest.mark.parametrize("block,grid", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("pattern", pr.WAVE_PATTERNS)
def test_block_alloc(lib, pattern, block, grid):
    """Three calls on one cursor that does not start at 0: slots in thread order within a workgroup and a call."""
    for n in pr.launch_counts(block, grid):
        key, valid = _pattern(pattern, n, 3, block=block)
        _check_alloc(lib, "blockAlloc", block, grid, np.zeros_like(key), valid, np.zeros_like(key), np.array([37], np.int32),
                     "%s n %d" % (pattern, n))


@pytest.mark.parametrize("block,grid", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("pattern", pr.WAVE_PATTERNS)
@pytest.mark.parametrize("helper", ["waveKeyedAlloc", "waveRunAlloc"])
def test_wave_alloc(lib, helper, pattern, block, grid):
    for seed, n in enumerate(pr.launch_counts(block, grid)):
        key, valid = _pattern(pattern, n, 2, block=block)
        _check_alloc(lib, helper, block, grid, key, valid, key, pr.initial_base("count", pr.NKEYS, seed), "%s n %d" % (pattern, n))


# (keyBits, stride, keys): keys up to 1024 need all 11 bits (prims_ref.spread_keys takes the patterns' keys there)
ONCE = {"bits11": (11, 1, 1025), "bits11-stride32": (11, 32, 1025), "bits1": (1, 1, 2)}


@pytest.mark.parametrize("block,grid", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("pattern", pr.WAVE_PATTERNS)
@pytest.mark.parametrize("config", list(ONCE))
def test_wave_keyed_alloc_once(lib, config, pattern, block, grid):
    key_bits, stride, nkeys = ONCE[config]
    for seed, n in enumerate(pr.launch_counts(block, grid)):
        key, valid = _pattern(pattern, n, 2, block=block)
        key = pr.spread_keys(key, nkeys)
        assert key.max(initial=0) < (1 << key_bits)
        base0 = pr.initial_base("count", (nkeys - 1) * stride + 1, seed)
        _check_alloc(lib, "waveKeyedAllocOnce", block, grid, key, valid, key.astype(np.int64) * stride, base0,
                     "%s %s n %d" % (config, pattern, n), key_bits, stride)


@pytest.mark.parametrize("block,grid", [(b, g) for b in (128, 256, 1024) for g in pr.GRIDS])
@pytest.mark.parametrize("pattern", pr.WAVE_PATTERNS)
@pytest.mark.parametrize("fetch", [True, False], ids=["fetch", "count"])
@pytest.mark.parametrize("slotted", [False, True], ids=["dense", "slotted"])
def test_block_keyed_alloc65(lib, slotted, fetch, pattern, block, grid):
    """Keys 0 .. 64, 64 included; the word of key k is colorSlot(k) when slotted. No order is promised."""
    for seed, n in enumerate(pr.launch_counts(block, grid)):
        key, valid = _pattern(pattern, n, 2, nkeys=65, block=block)
        word = pr.color_slot(key) if slotted else key
        base0 = pr.initial_base("count", int(pr.color_slot(64)) + 1 if slotted else 65, seed)
        _check_alloc(lib, "blockKeyedAlloc65", block, grid, key, valid, word, base0, "%s n %d" % (pattern, n), int(fetch), int(slotted),
                     fetch=fetch)


def test_wave_probe_refuses_bad_arguments(lib):
    """A block size that is no multiple of 64 in 64 .. 1024, more elements than threads, a key outside the counter array, a
    64-thread workgroup for blockKeyedAlloc65: hipErrorInvalidValue (1), and the array comes back untouched."""
    key, valid = pr.wave_pattern("all_same", 128, 1, nkeys=8)
    val = np.ones((1, 128), np.uint32)
    base0 = np.arange(8, dtype=np.int32)

    def refused(helper, block, grid, key=key, base0=base0, p0=0, p1=0):
        rc, base1, _ = _call(lib, helper, block, grid, key, val, valid, base0, p0, p1)
        return rc == 1 and np.array_equal(base1, base0)

    assert refused("waveAtomicAddInt", 96, 2) and refused("waveAtomicAddInt", 32, 4) and refused("waveAtomicAddInt", 1088, 1)
    assert refused("waveAtomicAddInt", 64, 1)  # 128 elements, 64 threads
    bad = key.copy()
    bad[0, 77] = 8
    assert refused("waveKeyedAlloc", 128, 1, key=bad) and refused("waveRunAlloc", 128, 1, key=-key - 1)
    assert refused("waveKeyedAllocOnce", 128, 1, key=np.full_like(key, 2), p0=1, p1=1)  # a key of two bits with keyBits = 1
    assert refused("waveKeyedAllocOnce", 128, 1, key=np.full_like(key, 1), p0=3, p1=8)  # word 8 of 8
    assert refused("blockKeyedAlloc65", 64, 2, base0=np.zeros(65, np.int32), p0=1)
    assert refused("blockKeyedAlloc65", 128, 1, key=np.full_like(key, 65), base0=np.zeros(80, np.int32), p0=1)
    assert refused("blockKeyedAlloc65", 128, 1, key=np.full_like(key, 64), base0=np.zeros(65, np.int32), p0=1, p1=1)  # colorSlot(64) = 2048
    assert refused("waveAtomicAddInt", 128, 1, p0=1)
    rc, base1, _ = _call(lib, "waveAtomicAddInt", 128, 1, key, val, valid, base0)
    assert rc == 0 and base1.sum() == base0.sum() + 128
