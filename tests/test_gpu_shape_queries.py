"""GPU: batched shape overlap and closest shape cast queries on the device (include/b2hip.h: b2hip_query_shapes,
b2hip_shape_cast_closest) against the answers composed from the drop-in on the SAME world (the device world behind the
drop-in, Harness.device_world()): b2World::QueryAABB, then b2TestOverlap / b2ShapeCast per reported proxy
(box2d-mt_amd/harness/harness.cpp: b2h_query_shape, b2h_shape_cast_all). Overlap lists equal exactly, in ascending id; a cast
equals the minimum (lambda, fixture id) of every drop-in hit in all bits."""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
from test_gpu_queries_batch import SCENES, _bind, _hashes, fixture_filters, fixture_rows

CHAIN = 3


def _bind_shapes(hw):
    L = _bind(hw)
    L.b2h_query_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p]
    L.b2h_query_shape.restype = C.c_int
    L.b2h_shape_cast_all.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
    L.b2h_shape_cast_all.restype = C.c_int
    return L


def octagon(r):
    a = np.arange(8) * (np.pi / 4.0)
    v = np.stack([r * np.cos(a), r * np.sin(a)], 1).astype(np.float32)
    e = np.roll(v, -1, axis=0) - v
    n = np.stack([e[:, 1], -e[:, 0]], 1)
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    s = b2hip.Shape()
    s.type, s.count, s.radius = b2hip.POLYGON, 8, b2hip.POLYGON_RADIUS
    for i in range(8):
        s.verts[2 * i], s.verts[2 * i + 1] = v[i]
        s.normals[2 * i], s.normals[2 * i + 1] = n[i]
    return s


def chain_link(v1, v2):
    s = b2hip.Shape()
    s.type, s.count, s.radius = CHAIN, 0, b2hip.POLYGON_RADIUS
    s.verts[0], s.verts[1], s.verts[2], s.verts[3] = v1[0], v1[1], v2[0], v2[1]
    return s


def probe_shapes(rng):
    """circles of 0.05 - 3 m, boxes (rotated by the poses), 8-gons, an edge and a chain link"""
    shapes = [b2hip.circle_shape(float(r)) for r in rng.uniform(0.05, 3.0, 4)]
    shapes += [b2hip.circle_shape(0.4, 0.3, -0.2), b2hip.box_shape(0.5, 0.25), b2hip.box_shape(2.0, 0.1), octagon(0.7),
               octagon(2.5), b2hip.edge_shape((-1.5, 0.2), (1.0, -0.4)), chain_link((-0.8, 0.0), (0.9, 0.3))]
    return shapes


def poses_near(hw, n, rng):
    b = hw.bodies()
    pos = b[b[:, 7] >= 0][:, :2]
    lo, hi = pos.min(axis=0) - 2.0, pos.max(axis=0) + 2.0
    xy = np.concatenate([rng.uniform(lo, hi, (n // 2, 2)), pos[rng.integers(0, len(pos), n - n // 2)]])
    return np.concatenate([xy, rng.uniform(0.0, 2.0 * np.pi, (n, 1))], 1).astype(np.float32)


def translations(n, rng, lo=0.0, hi=40.0):
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    ln = rng.uniform(lo, hi, n)
    ln[::17] = 0.0  # (zero translations among them)
    return np.stack([np.cos(ang) * ln, np.sin(ang) * ln], 1).astype(np.float32)


def host_overlaps(hw, shape, pose, cap=1 << 18):
    L = _bind_shapes(hw)
    out = np.zeros(cap, np.int32)
    k = L.b2h_query_shape(hw.ptr, C.byref(shape), float(pose[0]), float(pose[1]), float(pose[2]), cap,
                          out.ctypes.data_as(C.c_void_p))
    assert k <= cap
    return out[:k]


def host_casts(hw, shape, pose, t, cap=4096):
    """every drop-in hit: (ids (n, 2) fixture / body, values (n, 5) lambda, point, normal)"""
    L = _bind_shapes(hw)
    ids = np.zeros((cap, 2), np.int32)
    vals = np.zeros((cap, 5), np.float32)
    k = L.b2h_shape_cast_all(hw.ptr, C.byref(shape), float(pose[0]), float(pose[1]), float(pose[2]), float(t[0]), float(t[1]),
                             cap, ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p))
    assert k <= cap
    return ids[:k], vals[:k]


def closest_of(ids, vals):
    """the drop-in's hits reduced as the header says: the smallest (lambda bits, fixture id), a -0.0 lambda counting as 0"""
    if len(ids) == 0:
        return None
    key = ((vals[:, 0] + np.float32(0.0)).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[:, 0].astype(np.uint64)
    return int(np.argmin(key))


def cast_matches(h, ids, vals):
    k = closest_of(ids, vals)
    if k is None:
        assert h["fixture"] == -1 and h["body"] == -1 and h["fraction"] == np.float32(1.0), "the device hits, the drop-in does not"
        return False
    mine = np.array([h["fraction"], h["point"][0], h["point"][1], h["normal"][0], h["normal"][1]], np.float32)
    assert (int(h["fixture"]), int(h["body"])) == (int(ids[k, 0]), int(ids[k, 1])), "another fixture: %s vs %s" % (h, ids[k])
    assert np.array_equal(mine.view(np.uint32), vals[k].view(np.uint32)), "hit differs: %s vs %s" % (mine, vals[k])
    return True


def check_against_dropin(hw, n, seed, mask=0xFFFF, sensors=True, tlo=0.0, thi=40.0):
    """overlaps and casts of every probe shape against the drop-in composition; returns (items reported, cast hits)"""
    rng = np.random.default_rng(seed)
    dw = b2hip.World.borrow(hw.device_world())
    shapes = probe_shapes(rng)
    poses = poses_near(hw, n, rng)
    idx = rng.integers(0, len(shapes), n).astype(np.int32)
    offs, items = dw.query_shapes(shapes, poses, shape_index=idx, mask=mask, sensors=sensors)
    flt = fixture_filters(hw)

    def passes(fid):
        return (flt[fid, 0] & mask) != 0 and (sensors or flt[fid, 1] == 0)

    reported = 0
    for i in range(n):
        seg = items["fixture"][offs[i]:offs[i + 1]]
        want = [int(f) for f in host_overlaps(hw, shapes[idx[i]], poses[i]) if passes(f)]
        assert seg.tolist() == want, "query %d (shape %d, pose %s) reports another list" % (i, idx[i], poses[i])
        reported += len(seg)
    t = translations(n, rng, tlo, thi)
    hits = dw.shape_cast_closest(shapes, poses, t, shape_index=idx, mask=mask, sensors=sensors)
    nhit = 0
    for i in range(n):
        ids, vals = host_casts(hw, shapes[idx[i]], poses[i], t[i])
        keep = np.array([passes(f) for f in ids[:, 0]], bool) if len(ids) else np.zeros(0, bool)
        nhit += cast_matches(hits[i], ids[keep], vals[keep])
    dw.close()
    return reported, nhit


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene,kw,steps", SCENES)
def test_shape_queries_match_the_dropin(amd, name, scene, kw, steps):
    hw = amd.world(scene, **kw)
    hw.step(steps)
    reported, nhit = check_against_dropin(hw, n=300 if name != "field200k" else 200, seed=17)
    assert reported > 0 and nhit > 0, (reported, nhit)
    if name == "field200k":
        # a large circle: a list longer than 4096 items (k_query_mark / k_query_compact_big), exactly the drop-in's
        b = hw.bodies()
        pos = b[b[:, 7] >= 0][:, :2]
        c = np.median(pos, axis=0)
        area = float(np.prod(pos.max(axis=0) - pos.min(axis=0)))
        dw = b2hip.World.borrow(hw.device_world())
        big = b2hip.circle_shape(float(np.sqrt(12000.0 * area / len(pos) / np.pi)))  # (about 12 000 bodies' share of the field)
        pose = np.array([[c[0], c[1], 0.0]], np.float32)
        offs, items = dw.query_shapes(big, pose)
        want = host_overlaps(hw, big, pose[0])
        assert len(want) > 4096, len(want)
        assert items["fixture"].tolist() == want.tolist()
        dw.close()
    hw.close()


@pytest.mark.gpu
def test_long_casts_take_every_path(amd):
    """casts of 20 - 40 m on the 200k field (pieces) and of 10^4 m (more than 4096 pieces: every proxy scanned)"""
    hw = amd.world(bh.FIELD, p0=200000, p1=2000, flags=bh.F_CONTINUOUS | bh.F_SLEEP | bh.F_WARM, seed=3)
    hw.step(4)
    _, nhit = check_against_dropin(hw, n=120, seed=23, tlo=20.0, thi=40.0)
    assert nhit > 0
    rng = np.random.default_rng(29)
    dw = b2hip.World.borrow(hw.device_world())
    shapes = probe_shapes(rng)
    poses = poses_near(hw, 24, rng)
    t = translations(24, rng, 1.0e4, 1.2e4)
    idx = rng.integers(0, len(shapes), 24).astype(np.int32)
    hits = dw.shape_cast_closest(shapes, poses, t, shape_index=idx)
    for i in range(24):
        cast_matches(hits[i], *host_casts(hw, shapes[idx[i]], poses[i], t[i]))
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_filters_equal_the_filtered_dropin_answers(amd):
    hw = amd.world(bh.SENSORS, p0=40, seed=5)
    hw.step(40)
    L = _bind(hw)
    for k in range(2, hw.body_count):
        if k % 3 == 0:
            assert L.b2h_edit(hw.ptr, 4, k, 2.0, 0.0, 0.0) == 0
        elif k % 5 == 0:
            assert L.b2h_edit(hw.ptr, 4, k, 4.0, 0.0, 0.0) == 0
        if k % 7 == 0:
            assert L.b2h_edit(hw.ptr, 5, k, 1.0, 0.0, 0.0) == 0
    hw.step(20)
    flt = fixture_filters(hw)
    live = flt[:, 0] >= 0
    assert {1, 2, 4} <= set(flt[live, 0].tolist()) and flt[live, 1].sum() >= 3
    total = 0
    for mask in (0xFFFF, 0x0001, 0x0006, 0xFFFE):
        for sensors in (True, False):
            reported, _ = check_against_dropin(hw, n=120, seed=31, mask=mask, sensors=sensors, thi=15.0)
            total += reported
    assert total > 0
    hw.close()


@pytest.mark.gpu
def test_special_cases(amd):
    hw = amd.world(bh.RAIN, p0=200, seed=3)
    hw.step(60)
    L = _bind(hw)
    dw = b2hip.World.borrow(hw.device_world())
    b = hw.bodies()
    circle = b2hip.circle_shape(0.3)
    # casts that start in overlap, as b2ShapeCast answers them: a fixture whose skin alone the shape overlaps is hit at
    # lambda 0, one whose core it overlaps is not hit at all; the overlap query reports both at the start pose
    k = int(np.flatnonzero(b[:, 7] == 2)[0])
    pose = np.array([[b[k, 0], b[k, 1], 0.0]], np.float32)
    inside = set(dw.query_shapes(circle, pose)[1]["fixture"].tolist())
    assert inside, "the circle at a body's centre overlaps nothing"
    for t in ((6.0, 0.0), (0.0, 0.0), (0.0, -25.0)):
        tt = np.array([t], np.float32)
        h = dw.shape_cast_closest(circle, pose, tt)[0]
        assert h["fixture"] not in inside or h["fraction"] == 0.0
        cast_matches(h, *host_casts(hw, circle, pose[0], tt[0]))
    # NaN poses and non-finite translations: nothing, misses
    nan, inf = np.float32("nan"), np.float32("inf")
    bad = np.array([[nan, 1.0, 0.0], [1.0, nan, 0.0], [1.0, 1.0, nan]], np.float32)
    offs, items = dw.query_shapes(circle, bad)
    assert offs.tolist() == [0, 0, 0, 0]
    h = dw.shape_cast_closest(circle, np.concatenate([bad, pose, pose]),
                              np.array([[1, 0], [1, 0], [1, 0], [inf, 0], [0, nan]], np.float32))
    assert np.all(h["fixture"] == -1) and np.all(h["body"] == -1) and np.all(h["fraction"] == 1.0)
    # coordinates beyond 1e8: every proxy scanned, the drop-in's answer
    far = np.array([[2.0e8, 0.0, 0.3], [pose[0, 0], pose[0, 1], 0.0]], np.float32)
    tfar = np.array([[5.0, 0.0], [3.0e8, -1.0e3]], np.float32)
    offs, items = dw.query_shapes(circle, far)
    for i in range(2):
        assert items["fixture"][offs[i]:offs[i + 1]].tolist() == host_overlaps(hw, circle, far[i]).tolist()
    h = dw.shape_cast_closest(circle, far, tfar)
    for i in range(2):
        cast_matches(h[i], *host_casts(hw, circle, far[i], tfar[i]))
    # a shape touching exactly: a 0.5 x 0.5 box created beside the rain, a box query sharing its right face
    row = L.b2h_edit(hw.ptr, 0, -1, -30.0, 40.0, 0.0)
    assert row >= 0
    touch = np.array([[-29.0, 40.0, 0.0]], np.float32)
    box = b2hip.box_shape(0.5, 0.5)
    got = dw.query_shapes(box, touch)[1]["fixture"].tolist()
    assert got == host_overlaps(hw, box, touch[0]).tolist() and len(got) >= 1
    rows = fixture_rows(hw)
    assert row in rows[got, 0].tolist()
    # set_transform between steps, seen without a step
    assert L.b2h_edit(hw.ptr, 2, row, 30.0, 45.0, 0.7) == 0
    moved = np.array([[30.0, 45.0, 0.0], [-29.0, 40.0, 0.0]], np.float32)
    offs, items = dw.query_shapes(box, moved)
    assert row in rows[items["fixture"][offs[0]:offs[1]], 0].tolist()
    assert row not in rows[items["fixture"][offs[1]:offs[2]], 0].tolist()
    for i in range(2):
        assert items["fixture"][offs[i]:offs[i + 1]].tolist() == host_overlaps(hw, box, moved[i]).tolist()
    down = np.array([[30.0, 60.0, 0.0]], np.float32)
    h = dw.shape_cast_closest(box, down, np.array([[0.0, -30.0]], np.float32))[0]
    assert h["fixture"] >= 0
    cast_matches(h, *host_casts(hw, box, down[0], (0.0, -30.0)))
    # two identical calls: the same bytes
    rng = np.random.default_rng(41)
    shapes = probe_shapes(rng)
    poses = poses_near(hw, 200, rng)
    t = translations(200, rng)
    idx = rng.integers(0, len(shapes), 200).astype(np.int32)
    o1, i1 = dw.query_shapes(shapes, poses, shape_index=idx)
    o2, i2 = dw.query_shapes(shapes, poses, shape_index=idx)
    assert o1.tobytes() == o2.tobytes() and i1.tobytes() == i2.tobytes()
    h1 = dw.shape_cast_closest(shapes, poses, t, shape_index=idx)
    h2 = dw.shape_cast_closest(shapes, poses, t, shape_index=idx)
    assert h1.tobytes() == h2.tobytes()
    # empty batches
    z3, z2 = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
    assert dw.query_shapes(circle, z3)[0].tolist() == [0]
    assert len(dw.shape_cast_closest(circle, z3, z2)) == 0
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_a_cast_from_inside_a_core_is_no_hit():
    """a small circle whose centre lies inside a box's core: b2ShapeCast returns false for that box, so the cast reports
    the next fixture along the way; b2hip_query_shapes reports the box at the start pose"""
    w = b2hip.World(gravity=(0.0, 0.0))
    a = w.create_body(b2hip.STATIC, (0.0, 0.0))
    w.create_fixture(a, b2hip.box_shape(1.0, 1.0))
    c = w.create_body(b2hip.STATIC, (6.0, 0.0))
    w.create_fixture(c, b2hip.box_shape(1.0, 1.0))
    w.step()
    circle = b2hip.circle_shape(0.1)
    pose = np.array([[0.2, 0.1, 0.0]], np.float32)
    offs, items = w.query_shapes(circle, pose)
    assert items["fixture"].tolist() == [0]
    h = w.shape_cast_closest(circle, pose, np.array([[10.0, 0.0]], np.float32))[0]
    assert h["fixture"] == 1 and h["body"] == 1
    # the circle's skin meets the second box's left face (x = 5) after about (5 - 0.2 - 0.1) / 10
    assert abs(h["fraction"] - 0.47) < 2e-3, h["fraction"]
    h = w.shape_cast_closest(circle, pose, np.array([[-10.0, 0.0]], np.float32))[0]
    assert h["fixture"] == -1 and h["fraction"] == 1.0
    w.close()


@pytest.mark.gpu
def test_a_proxy_wider_than_the_grid_limit():
    """a 400 m ground among 0.2 m boxes is a large proxy (tested by every query): it is overlapped and hit"""
    w = b2hip.World()
    g = w.create_body(b2hip.STATIC, (0.0, 0.0))
    w.create_fixture(g, b2hip.box_shape(200.0, 0.5))
    for i in range(400):
        b = w.create_body(b2hip.DYNAMIC, (-100.0 + 0.5 * i, 3.0 + (i % 7)))
        w.create_fixture(b, b2hip.box_shape(0.1, 0.1), density=1.0)
    w.step()
    circle = b2hip.circle_shape(0.25)
    poses = np.array([[150.0, 0.6, 0.0], [150.0, 5.0, 0.0], [-150.0, 40.0, 0.0]], np.float32)
    offs, items = w.query_shapes(circle, poses)
    assert items["fixture"][offs[0]:offs[1]].tolist() == [0]
    assert offs[2] == offs[1]
    h = w.shape_cast_closest(circle, poses[1:], np.array([[0.0, -10.0], [0.0, -60.0]], np.float32))
    assert h["fixture"].tolist() == [0, 0]
    # the circle's skin meets the ground's top (y = 0.5) after about (5 - 0.25 - 0.5) / 10 and (40 - 0.75) / 60
    assert abs(h["fraction"][0] - 0.425) < 2e-3 and abs(h["fraction"][1] - 39.25 / 60.0) < 2e-3, h["fraction"]
    assert np.allclose(np.abs(h["normal"]), [[0.0, 1.0], [0.0, 1.0]], atol=1e-4)
    w.close()


@pytest.mark.gpu
def test_shape_queries_do_not_perturb_the_step(amd):
    kw = dict(p0=20, p1=4, flags=bh.F_CONTINUOUS | bh.F_SLEEP | bh.F_WARM, seed=5)
    a, b = amd.world(bh.BULLETS, **kw), amd.world(bh.BULLETS, **kw)
    rng = np.random.default_rng(5)
    shapes = probe_shapes(rng)
    dw = b2hip.World.borrow(a.device_world())
    for _ in range(120):
        a.step(1)
        b.step(1)
        poses = poses_near(a, 48, rng)
        idx = rng.integers(0, len(shapes), 48).astype(np.int32)
        dw.query_shapes(shapes, poses, shape_index=idx)
        dw.shape_cast_closest(shapes, poses, translations(48, rng), shape_index=idx)
    dw.close()
    assert np.array_equal(a.bodies().view(np.uint32), b.bodies().view(np.uint32))
    assert _hashes(a) == _hashes(b)
    a.close()
    b.close()


@pytest.mark.gpu
def test_refused_inside_an_open_step_and_on_a_sharded_world():
    w = b2hip.World(continuous=True)
    g = w.create_body(b2hip.STATIC, (0.0, 0.0))
    w.create_fixture(g, b2hip.box_shape(20.0, 0.05))
    for k in range(6):
        b = w.create_body(b2hip.DYNAMIC, (-5.0 + 2.0 * k, 3.0 + 0.1 * k), velocity=(1.0 * k, -60.0))
        w.create_fixture(b, b2hip.box_shape(0.1, 0.1), density=1.0)
    circle = b2hip.circle_shape(30.0)
    pose = np.zeros((1, 3), np.float32)
    assert len(w.query_shapes(circle, pose)[1]) == 7
    w.set_flags(continuous=True, sub_stepping=True)
    refused = 0
    for _ in range(12):
        w.step()
        try:
            w.query_shapes(circle, pose)
        except b2hip.B2HipError as e:
            assert "error -1" in str(e) and "inside a step" in str(e)
            with pytest.raises(b2hip.B2HipError, match="error -1"):
                w.shape_cast_closest(circle, pose, np.ones((1, 2), np.float32))
            refused += 1
    assert refused > 0, "no call left the step open"
    w.close()
    s = b2hip.World()
    g = s.create_body(b2hip.STATIC, (0.0, 0.0))
    s.create_fixture(g, b2hip.box_shape(20.0, 0.05))
    s.step()
    assert b2hip.lib().b2hip_set_shard(s.p, 0, 2) == 0
    with pytest.raises(b2hip.B2HipError, match="error -4"):
        s.query_shapes(circle, pose)
    with pytest.raises(b2hip.B2HipError, match="error -4"):
        s.shape_cast_closest(circle, pose, np.ones((1, 2), np.float32))
    s.close()
