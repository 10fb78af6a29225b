"""GPU tests of the product's device math headers AS THE DEVICE COMPILER BUILDS THEM (tests/probe/device_probe.hip: the cases of
tests/probe/probe_cases.h, one test vector per thread, hipcc with the product's own flags): sin / cos, manifolds, GJK, time of
impact, shape cast, ray cast, point test, AABB, mass, polygon build and ownIdBlock, bitwise against the vectors recorded from
the reference build (tests/golden/*_vectors.npz) - the same files tests/test_device_math_cpu.py holds the g++ build to.

Every batch runs twice: in file order with 256-thread blocks, and in a fixed permuted order with 64-thread blocks and a vector
count that is no multiple of 64 (a partial last wave); the two runs must give the same bytes per vector (_both)."""
import ctypes as C
import os

import numpy as np
import pytest

import b2hip
import probe_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def dev():
    """The device probe. No fallback: a missing library is a failure (it is built by `make -C box2d-mt_amd all`)."""
    b2hip.use_torch_hip_runtime()  # one HIP runtime in the process, before anything that links libamdhip64 is loaded
    if not os.path.exists(pu.DEVICE_PROBE_LIB):
        pytest.fail("tests/probe/libdevice_probe.so missing: run __graft_entry__.build() (make -C box2d-mt_amd all builds it "
                    "with the product's HIPFLAGS); there is no CPU stand-in for the device build")
    return C.CDLL(pu.DEVICE_PROBE_LIB)


def _f(a):
    return a.ctypes.data_as(fp)


def _i(a):
    return a.ctypes.data_as(ip)


def _v(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _both(run, *ins):
    """run(block, *arrays) -> tuple of per-vector output arrays. File order with 256-thread blocks, then a fixed permutation
    with 64-thread blocks and a count that is no multiple of 64: the same bytes per vector. Returns the first run's outputs."""
    ins = [np.ascontiguousarray(a) for a in ins]
    n = len(ins[0])
    first = run(256, *ins)
    perm = np.random.default_rng(64).permutation(n)
    if n % 64 == 0:
        perm = np.append(perm, perm[0])
    assert len(perm) % 64 != 0
    second = run(64, *[np.ascontiguousarray(a[perm]) for a in ins])
    for a, b in zip(first, second):
        assert a.dtype.itemsize == 4 and np.array_equal(_bits(a[perm]), _bits(b)), "the two launch shapes disagree"
    return first


def _ok(rc):
    assert rc == 0, "device probe: HIP error %d" % rc


# ---- the entry points as run(block, *arrays) ------------------------------------------------------------------------------
def _sincos(L):
    def run(block, a):
        out = np.zeros((len(a), 8), np.float32)
        _ok(L.dprobe_sincos(len(a), _f(a), _f(out), block))
        return (out,)
    return run


def _collide(L):
    def run(block, sa, xa, sb, xb):
        out = np.zeros((len(sa), 16), np.float32)
        _ok(L.dprobe_collide(len(sa), _v(sa), _f(xa), _v(sb), _f(xb), _f(out), block))
        return (out,)
    return run


def _shape_fn(entry, width, dtype=np.float32):
    """dprobe_shape_aabb / _shape_raycast / _test_point / _shape_mass: shapes, then the per-vector inputs, then one output"""
    def run(block, shapes, *ins):
        out = np.zeros((len(shapes), width) if width > 1 else len(shapes), dtype)
        _ok(entry(len(shapes), _v(shapes), *[_f(a) for a in ins], _v(out), block))
        return (out,)
    return run


def _proxy_fn(entry, width, tail):
    """dprobe_distance / _toi / _shape_cast: count, verts, radius, placement per side, then `tail(arrays)` -> extra arguments"""
    def run(block, ca, va, ra, pa, cb, vb, rb, pb, *rest):
        out = np.zeros((len(ca), width), np.float32)
        _ok(entry(len(ca), _i(ca), _f(va), _f(ra), _f(pa), _i(cb), _f(vb), _f(rb), _f(pb), *tail(*rest), _f(out), block))
        return (out,)
    return run


def _polygon(L):
    def run(block, inp, density):
        out = np.zeros((len(inp), 39), np.float32)
        _ok(L.dprobe_polygon(len(inp), _f(inp), _f(density), _f(out), block))
        return (out,)
    return run


def _own_id_block(L, nb_max):
    def run(block, ids):
        out = np.zeros((nb_max, len(ids)), np.int32)
        _ok(L.dprobe_own_id_block(len(ids), _i(ids), nb_max, _i(out), block))
        return (np.ascontiguousarray(out.T),)  # per id, like every other family: [ids][nb]
    return run


def _mismatches(got, want, defined=None):
    """rows whose bits differ (in the columns `defined` marks, when given)"""
    diff = _bits(got) != _bits(want)
    if defined is not None:
        diff &= defined
    return int(diff.reshape(len(got), -1).any(1).sum())


# ---- golden vectors ---------------------------------------------------------------------------------------------------------
def test_device_build_sincos_matches_golden(dev):
    """All five entry points - b2dSin, b2dCos, b2dSinCos, b2dRot (on the device the out-of-line copy), b2dRotInline - on the
    42 011 recorded angles: the reference's b2Rot::Set bits."""
    v = np.load(os.path.join(GOLD, "sincos_vectors.npz"))
    assert len(v["angle"]) == 42011
    out, = _both(_sincos(dev), v["angle"])
    for k in range(4):
        assert _mismatches(out[:, 2 * k], v["sin"]) == 0, "sin, entry point %d" % k
        assert _mismatches(out[:, 2 * k + 1], v["cos"]) == 0, "cos, entry point %d" % k


def test_device_build_collide_matches_golden(dev):
    v = np.load(os.path.join(GOLD, "collide_vectors.npz"))
    assert len(v["manifold"]) == 1500 and (v["manifold"][:, 1] > 0).sum() > 300
    out, = _both(_collide(dev), v["shapeA"], v["xfA"], v["shapeB"], v["xfB"])
    assert _mismatches(out, v["manifold"]) == 0


def test_device_build_distance_matches_golden(dev):
    v = np.load(os.path.join(GOLD, "toi_vectors.npz"))
    assert len(v["d_out"]) == 1200
    run = _proxy_fn(dev.dprobe_distance, 6, lambda use: (_i(use),))
    out, = _both(run, v["d_countA"], v["d_vertsA"], v["d_radiusA"], v["d_xfA"], v["d_countB"], v["d_vertsB"], v["d_radiusB"],
                 v["d_xfB"], v["d_useRadii"])
    assert _mismatches(out, v["d_out"]) == 0


def test_device_build_toi_matches_golden(dev):
    v = np.load(os.path.join(GOLD, "toi_vectors.npz"))
    assert len(v["t_out"]) == 2000
    run = _proxy_fn(dev.dprobe_toi, 2, lambda: (C.c_float(1.0),))
    out, = _both(run, v["t_countA"], v["t_vertsA"], v["t_radiusA"], v["t_sweepA"], v["t_countB"], v["t_vertsB"], v["t_radiusB"],
                 v["t_sweepB"])
    assert _mismatches(out, v["t_out"]) == 0


def test_device_build_polygon_matches_golden(dev):
    """b2dPolygonFromPoints with b2dPolygonFinish, then b2dShapeMass (vector i has the density 1 + 0.01 i)"""
    v = np.load(os.path.join(GOLD, "polygon_vectors.npz"))
    assert len(v["inp"]) == 200
    density = np.array([1.0 + 0.01 * i for i in range(len(v["inp"]))]).astype(np.float32)
    out, = _both(_polygon(dev), v["inp"], density)
    assert _mismatches(out, v["out"]) == 0


@pytest.fixture(scope="module")
def geom():
    import sys
    sys.path.insert(0, GOLD)
    import make_golden_geom as mg
    v = np.load(os.path.join(GOLD, "geom_vectors.npz"))
    mg.check_coverage(v)  # (the conditions that keep the comparisons below from being vacuous, from the reference's outputs)
    return v


def test_device_build_shape_raycast_matches_golden(dev, geom):
    """A hit compares flag, fraction and normal bitwise; a miss the flag."""
    want = geom["ray_out"]
    out, = _both(_shape_fn(dev.dprobe_shape_raycast, 4), geom["shapes"][geom["ray_shape"]], geom["ray_xf"], geom["ray_in"])
    defined = np.ones(want.shape, bool)
    defined[want[:, 0] == 0, 1:] = False
    assert (want[:, 0] > 0).sum() > 500
    assert _mismatches(out, want, defined) == 0


def test_device_build_test_point_matches_golden(dev, geom):
    out, = _both(_shape_fn(dev.dprobe_test_point, 1, np.int32), geom["shapes"][geom["pt_shape"]], geom["pt_xf"], geom["pt_in"])
    assert int((out != geom["pt_out"]).sum()) == 0


def test_device_build_shape_aabb_matches_golden(dev, geom):
    out, = _both(_shape_fn(dev.dprobe_shape_aabb, 4), geom["shapes"][geom["aabb_shape"]], geom["aabb_xf"])
    assert _mismatches(out, geom["aabb_out"]) == 0


def test_device_build_shape_mass_matches_golden(dev, geom):
    out, = _both(_shape_fn(dev.dprobe_shape_mass, 4), geom["shapes"][geom["mass_shape"]], geom["mass_density"])
    assert _mismatches(out, geom["mass_out"]) == 0


def test_device_build_shape_cast_matches_golden(dev, geom):
    """A hit compares point, normal, lambda and iterations bitwise, a miss the flag (pu.cast_fields: what the reference defines)."""
    proxies = [pu.proxy_of(r) for r in geom["shapes"]]
    side = {}
    for name in ("A", "B"):
        idx = geom["cast_shape" + name]
        side[name] = (np.array([proxies[s][0] for s in idx], np.int32), np.array([proxies[s][1] for s in idx], np.float32),
                      np.array([proxies[s][2] for s in idx], np.float32), geom["cast_xf" + name])
    run = _proxy_fn(dev.dprobe_shape_cast, 7, lambda t: (_f(t),))
    out, = _both(run, *side["A"], *side["B"], geom["cast_t"])
    want = geom["cast_out"]
    defined = np.zeros(want.shape, bool)
    for row, w in zip(defined, want):
        row[pu.cast_fields(w)] = True
    assert defined.all(1).sum() > 300
    assert _mismatches(out, want, defined) == 0


# ---- sin / cos over the whole float range ---------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 2049])
def test_device_build_sincos_sweep_equals_the_host_build(dev, offset):
    """Every 4099th bit pattern of the float range (the stride of the CPU test that ties the host build to libm and to the
    reference), and the same again 2049 further on: the device's five entry points equal the host build's b2dSin / b2dCos bit
    for bit on every finite input, and are NaN where it is NaN."""
    a = np.arange(offset, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32).view(np.float32)
    finite = np.isfinite(a)
    mag = np.abs(a[finite].astype(np.float64))
    for lo, hi in ((0.0, 2.0 ** -12), (2.0 ** -12, np.pi / 4), (np.pi / 4, 120.0), (120.0, np.inf)):  # the ranges of b2dSinCosImpl
        assert ((mag >= lo) & (mag < hi)).sum() >= 1000
    assert (~finite).sum() >= 1000
    P = pu.build_probe()
    s, c = np.empty_like(a), np.empty_like(a)
    P.probe_sincos(a.size, _f(a), _f(s), _f(c))
    out, = _both(_sincos(dev), a)
    for k in range(4):
        for got, want, name in ((out[:, 2 * k], s, "sin"), (out[:, 2 * k + 1], c, "cos")):
            assert _mismatches(got[finite], want[finite]) == 0, "%s, entry point %d" % (name, k)
            assert np.array_equal(np.isnan(got[~finite]), np.isnan(want[~finite])) and np.isnan(want[~finite]).all()


# ---- ownIdBlock ---------------------------------------------------------------------------------------------------------------
def _own_id_block_expected(ids, nb_max):
    """1 + (id * 2654435761u >> 8) % nb for nb = 1 .. nb_max, in 64-bit integers on the host: [ids][nb]"""
    x = ((ids.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)
    return (1 + x.astype(np.int64)[:, None] % np.arange(1, nb_max + 1, dtype=np.int64)[None, :]).astype(np.int32)


def test_device_build_own_id_block_strided_ids(dev):
    """ownIdBlock on the device (whose own lowering of `%` it replaces) against the integer remainder: every block count up to
    1 024 over every 257th body id below 2 000 000 - the first half of the CPU check's domain."""
    ids = np.arange(0, 2000000, 257, dtype=np.int32)
    out, = _both(_own_id_block(dev, 1024), ids)
    assert int((out != _own_id_block_expected(ids, 1024)).sum()) == 0


@pytest.mark.parametrize("half", [0, 1])
def test_device_build_own_id_block_top_of_the_hash(dev, half):
    """... and every id below 2 000 000 whose hash lies in the top sixteenth of its 24 bits (where the float quotient rounds up
    past an integer), again for every block count up to 1 024 (the ids in two halves, to keep each case short)."""
    every = np.arange(2000000, dtype=np.int64)
    ids = every[(((every * 2654435761) & 0xffffffff) >> 8) >= 0xf00000].astype(np.int32)
    assert len(ids) > 100000
    ids = ids[:len(ids) // 2] if half == 0 else ids[len(ids) // 2:]
    bad = 0
    for at in range(0, len(ids), 16001):  # (64 MB of answers a call; 16 001: no chunk is a multiple of 64)
        part = ids[at:at + 16001]
        out, = _both(_own_id_block(dev, 1024), part)
        bad += int((out != _own_id_block_expected(part, 1024)).sum())
    assert bad == 0
