"""GPU: batched nearest-fixture and within-range distance queries on the device (include/b2hip.h:
b2hip_shape_distance_closest, b2hip_query_shapes_within) against the answer composed from the drop-in on the SAME world (the
device world behind the drop-in, Harness.device_world()): b2World::QueryAABB over the query box, then b2Distance per reported
proxy (box2d-mt_amd/harness/harness.cpp: b2h_shape_distance_all). Every comparison is exact in every bit: a within list is
the drop-in's list in ascending id, record for record; a closest answer is the minimum (distance bits, fixture id) of it."""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
from test_gpu_queries_batch import SCENES, _bind, _hashes, fixture_filters, fixture_rows
from test_gpu_shape_queries import poses_near, probe_shapes

INF = np.float32("inf")


def _bind_distance(hw):
    L = _bind(hw)
    L.b2h_shape_distance_all.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    L.b2h_shape_distance_all.restype = C.c_int
    return L


def host_distances(hw, shape, pose, max_distance, cap=4096):
    """every drop-in proxy within range, in ascending fixture id: (ids (k, 3) fixture / body / iterations, values (k, 5)
    distance, point A, point B)"""
    L = _bind_distance(hw)
    while True:
        ids = np.zeros((cap, 3), np.int32)
        vals = np.zeros((cap, 5), np.float32)
        k = L.b2h_shape_distance_all(hw.ptr, C.byref(shape), float(pose[0]), float(pose[1]), float(pose[2]), float(max_distance),
                                     cap, ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p))
        if k <= cap:
            break
        cap = k
    order = np.argsort(ids[:k, 0], kind="stable")
    return ids[:k][order], vals[:k][order]


def records(hits):
    """DISTANCE_HIT_DTYPE rows as the drop-in's two tables"""
    ids = np.stack([hits["fixture"], hits["body"], hits["iterations"]], 1).astype(np.int32).reshape(-1, 3)
    vals = np.concatenate([hits["distance"].reshape(-1, 1), hits["point_a"].reshape(-1, 2), hits["point_b"].reshape(-1, 2)], 1)
    return ids, np.ascontiguousarray(vals, np.float32)


def closest_of(ids, vals):
    """the drop-in's list reduced as the header says: the smallest (distance bits, fixture id); distances are >= +0"""
    if len(ids) == 0:
        return None
    key = (vals[:, 0].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[:, 0].astype(np.uint64)
    return int(np.argmin(key))


def is_miss(h):
    return (h["fixture"] == -1 and h["body"] == -1 and h["distance"] == INF and h["iterations"] == 0
            and not np.any(h["point_a"].view(np.uint32)) and not np.any(h["point_b"].view(np.uint32)))


def closest_matches(h, ids, vals):
    """one closest answer against the drop-in's list; True for a hit"""
    k = closest_of(ids, vals)
    if k is None:
        assert is_miss(h), "the device finds %s, the drop-in nothing" % (h,)
        return False
    mi, mv = records(np.array([h], b2hip.DISTANCE_HIT_DTYPE))
    assert mi[0].tolist() == ids[k].tolist(), "another fixture / body / iterations: %s vs %s (distance %r vs %r)" % (
        mi[0], ids[k], mv[0, 0], vals[k, 0])
    assert np.array_equal(mv[0].view(np.uint32), vals[k].view(np.uint32)), "record differs: %s vs %s" % (mv[0], vals[k])
    return True


def within_matches(seg, ids, vals):
    """one within list against the drop-in's"""
    mi, mv = records(seg)
    assert mi[:, 0].tolist() == ids[:, 0].tolist(), "another list: %s vs %s" % (mi[:, 0].tolist(), ids[:, 0].tolist())
    assert np.all(np.diff(mi[:, 0]) > 0), "not in ascending fixture id"
    assert np.array_equal(mi, ids), "bodies / iterations differ"
    assert np.array_equal(mv.view(np.uint32), vals.view(np.uint32)), "records differ"


def check_against_dropin(hw, n, seed, mask=0xFFFF, sensors=True, dmax=5.0):
    """both calls over every probe shape against the drop-in's lists (filtered in Python); returns per query the closest
    distance (inf for a miss)"""
    rng = np.random.default_rng(seed)
    dw = b2hip.World.borrow(hw.device_world())
    shapes = probe_shapes(rng)
    poses = poses_near(hw, n, rng)
    idx = rng.integers(0, len(shapes), n).astype(np.int32)
    dist = rng.uniform(0.0, dmax, n).astype(np.float32)
    flt = fixture_filters(hw)
    best = dw.shape_distance_closest(shapes, poses, dist, shape_index=idx, mask=mask, sensors=sensors)
    offs, hits = dw.query_shapes_within(shapes, poses, dist, shape_index=idx, mask=mask, sensors=sensors)
    assert offs[0] == 0 and offs[-1] == len(hits)
    for i in range(n):
        ids, vals = host_distances(hw, shapes[idx[i]], poses[i], dist[i])
        keep = ((flt[ids[:, 0], 0] & mask) != 0) & (sensors | (flt[ids[:, 0], 1] == 0)) if len(ids) else np.zeros(0, bool)
        ids, vals = ids[keep], vals[keep]
        assert np.all(vals[:, 0] <= dist[i])
        closest_matches(best[i], ids, vals)
        within_matches(hits[offs[i]:offs[i + 1]], ids, vals)
    dw.close()
    return best["distance"].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene,kw,steps", [s for s in SCENES if s[0] != "field200k"])
def test_distance_queries_match_the_dropin(amd, name, scene, kw, steps):
    hw = amd.world(scene, **kw)
    hw.step(steps)
    d = check_against_dropin(hw, n=200, seed=17)
    assert np.any(d < INF), "no query found anything"
    if name == "rain":  # (sparse, falling bodies: not overlaps alone)
        assert np.any((d > 0.0) & (d < INF)), "no hit at a positive distance"
        assert np.any(d == INF), "no query missed"
    hw.close()


@pytest.mark.gpu
def test_the_answer_does_not_depend_on_the_walk(amd):
    """max_distance D, 4 D and 10^4 m (every proxy scanned): wherever D finds something, all three find the same bytes"""
    hw = amd.world(bh.FIELD, p0=600, p1=0, seed=9)
    hw.step(40)
    rng = np.random.default_rng(43)
    dw = b2hip.World.borrow(hw.device_world())
    shapes = probe_shapes(rng)
    poses = poses_near(hw, 100, rng)
    idx = rng.integers(0, len(shapes), 100).astype(np.int32)
    D = 1.0
    near, mid, far = (dw.shape_distance_closest(shapes, poses, d, shape_index=idx) for d in (D, 4.0 * D, 1.0e4))
    hit = near["fixture"] >= 0
    assert np.any(hit), "nothing within D of any pose"
    assert np.any(~hit), "every pose has something within D"
    assert np.any(~hit & ((mid["fixture"] >= 0) | (far["fixture"] >= 0))), "no miss that a wider range turns into a hit"
    for i in range(100):
        for d, got in ((D, near), (4.0 * D, mid), (1.0e4, far)):
            if hit[i]:
                assert got[i].tobytes() == near[i].tobytes(), "pose %d: range %g finds another answer" % (i, d)
            closest_matches(got[i], *host_distances(hw, shapes[idx[i]], poses[i], d, cap=1 << 16))
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_a_list_longer_than_the_lds_sort(amd):
    """one circle at the median position of a 6000-body field with a range over the whole field: more than 4096 records
    (k_query_mark / k_query_compact_big, then k_query_range_eval), each the drop-in's"""
    hw = amd.world(bh.FIELD, p0=6000, p1=0, seed=9)
    hw.step(4)
    b = hw.bodies()
    pos = b[b[:, 7] >= 0][:, :2]
    c = np.median(pos, axis=0)
    reach = float(np.abs(pos - c).max() * 1.5 + 5.0)
    dw = b2hip.World.borrow(hw.device_world())
    circle = b2hip.circle_shape(0.5)
    pose = np.array([[c[0], c[1], 0.0]], np.float32)
    offs, hits = dw.query_shapes_within(circle, pose, reach)
    assert offs.tolist() == [0, len(hits)] and len(hits) > 4096, len(hits)
    within_matches(hits, *host_distances(hw, circle, pose[0], reach, cap=1 << 16))
    closest_matches(dw.shape_distance_closest(circle, pose, reach)[0], *records(hits))
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
    found = 0
    for mask in (0xFFFF, 0x0001, 0x0006, 0xFFFE):
        for sensors in (True, False):
            found += int(np.sum(check_against_dropin(hw, n=100, seed=31, mask=mask, sensors=sensors) < INF))
    assert found > 0
    hw.close()


@pytest.mark.gpu
def test_analytic_cases():
    """two static boxes of half-width 1 at the origin and at (6, 0)"""
    w = b2hip.World(gravity=(0.0, 0.0))
    for x in (0.0, 6.0):
        b = w.create_body(b2hip.STATIC, (x, 0.0))
        w.create_fixture(b, b2hip.box_shape(1.0, 1.0))
    w.step()
    circle = b2hip.circle_shape(0.25)
    mid = np.array([[3.0, 0.0, 0.0]], np.float32)
    # from the middle both faces are 2 m from the centre, in the same float operations: the lower id, at
    # 3 - 1 - 0.25 - b2_polygonRadius
    h = w.shape_distance_closest(circle, mid, 5.0)[0]
    assert h["fixture"] == 0 and h["body"] == 0 and h["iterations"] > 0
    assert abs(h["distance"] - 1.74) < 2e-3, h["distance"]
    assert np.allclose(h["point_b"], [1.01, 0.0], atol=2e-3) and np.allclose(h["point_a"], [2.75, 0.0], atol=2e-3)
    offs, hits = w.query_shapes_within(circle, mid, 5.0)
    assert hits["fixture"].tolist() == [0, 1] and hits["body"].tolist() == [0, 1]
    assert hits[0].tobytes() == h.tobytes()
    assert abs(hits[1]["distance"] - 1.74) < 2e-3 and np.allclose(hits[1]["point_b"], [4.99, 0.0], atol=2e-3)
    # half a metre to the right the second box is the nearer one
    h = w.shape_distance_closest(circle, np.array([[3.5, 0.0, 0.0]], np.float32), 5.0)[0]
    assert h["fixture"] == 1 and h["body"] == 1 and abs(h["distance"] - 1.24) < 2e-3, h
    # a range of 1 from the middle: nothing
    h = w.shape_distance_closest(circle, mid, 1.0)[0]
    assert is_miss(h), h
    assert w.query_shapes_within(circle, mid, 1.0)[0].tolist() == [0, 0]
    # a circle centred inside box 0: distance 0, both points the same
    inside = np.array([[0.3, -0.2, 0.0]], np.float32)
    h = w.shape_distance_closest(circle, inside, 5.0)[0]
    assert h["fixture"] == 0 and h["distance"] == 0.0 and h["point_a"].tobytes() == h["point_b"].tobytes()
    # max_distance = 0 reports exactly the fixtures at distance 0: the box the circle is in, and not the box whose skin is
    # 1e-4 m away (a distance that a range of 1e-3 reports)
    poses = np.array([[0.3, -0.2, 0.0], [1.2601, 0.0, 0.0], [3.0, 0.0, 0.0]], np.float32)
    offs, hits = w.query_shapes_within(circle, poses, 0.0)
    assert offs.tolist() == [0, 1, 1, 1] and hits["fixture"].tolist() == [0] and hits["distance"].tolist() == [0.0]
    z = w.shape_distance_closest(circle, poses, 0.0)
    assert z["fixture"].tolist() == [0, -1, -1] and z["distance"].tolist() == [0.0, INF, INF]
    near = w.shape_distance_closest(circle, poses[1:2], 1.0e-3)[0]
    assert near["fixture"] == 0 and 0.0 < near["distance"] < 1.0e-3, near
    # invalid records: misses and empty lists, among valid ones
    nan = np.float32("nan")
    bad = np.array([[nan, 0.0, 0.0], [3.0, nan, 0.0], [3.0, 0.0, nan], [INF, 0.0, 0.0], [3.0, 0.0, INF], [3.0, 0.0, 0.0],
                    [3.0, 0.0, 0.0], [3.0, 0.0, 0.0], [3.0, 0.0, 0.0]], np.float32)
    rng_ = np.array([5.0, 5.0, 5.0, 5.0, 5.0, nan, -1.0, INF, 5.0], np.float32)
    h = w.shape_distance_closest(circle, bad, rng_)
    assert all(is_miss(r) for r in h[:8]) and h[8]["fixture"] == 0
    offs, hits = w.query_shapes_within(circle, bad, rng_)
    assert offs.tolist() == [0] * 9 + [2] and hits["fixture"].tolist() == [0, 1]
    # empty batches
    z3 = np.zeros((0, 3), np.float32)
    assert len(w.shape_distance_closest(circle, z3, 1.0)) == 0
    offs, hits = w.query_shapes_within(circle, z3, 1.0)
    assert offs.tolist() == [0] and len(hits) == 0
    # a cap below the total: the offsets whole, the first records, the total returned
    L = b2hip.lib()
    r = np.zeros(1, b2hip.SHAPE_RANGE_DTYPE)
    r["x"], r["max_distance"] = 3.0, 5.0
    o2 = np.zeros(2, np.int32)
    one = np.zeros(1, b2hip.DISTANCE_HIT_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.b2hip_query_shapes_within(w.p, 1, C.byref(circle), 1, vp(r), None, 1, vp(o2), vp(one)) == 2
    assert o2.tolist() == [0, 2] and one[0]["fixture"] == 0 and abs(one[0]["distance"] - 1.74) < 2e-3
    w.close()


@pytest.mark.gpu
def test_a_proxy_wider_than_the_grid_limit():
    """a 400 m ground among 0.2 m boxes is a large proxy (tested by every query): found from 150 m along it"""
    w = b2hip.World()
    g = w.create_body(b2hip.STATIC, (0.0, 0.0))
    w.create_fixture(g, b2hip.box_shape(200.0, 0.5))
    for i in range(400):
        b = w.create_body(b2hip.DYNAMIC, (-100.0 + 0.5 * i, 3.0 + (i % 7)))
        w.create_fixture(b, b2hip.box_shape(0.1, 0.1), density=1.0)
    w.step()
    circle = b2hip.circle_shape(0.25)
    poses = np.array([[150.0, 5.0, 0.0], [-150.0, 40.0, 0.0]], np.float32)
    h = w.shape_distance_closest(circle, poses, [10.0, 30.0])
    # the circle's skin is 5 - 0.25 - 0.5 - b2_polygonRadius above the ground's; from 40 m up a range of 30 does not reach it
    assert h[0]["fixture"] == 0 and h[0]["body"] == 0 and abs(h[0]["distance"] - 4.24) < 2e-3, h[0]
    assert np.allclose(h[0]["point_b"], [150.0, 0.51], atol=2e-3)
    assert is_miss(h[1])
    offs, hits = w.query_shapes_within(circle, poses, [10.0, 30.0])
    assert offs.tolist() == [0, 1, 1] and hits[0].tobytes() == h[0].tobytes()
    w.close()


@pytest.mark.gpu
def test_special_cases_against_the_dropin(amd):
    hw = amd.world(bh.RAIN, p0=200, seed=3)
    hw.step(60)
    L = _bind(hw)
    dw = b2hip.World.borrow(hw.device_world())
    circle = b2hip.circle_shape(0.25)
    box = b2hip.box_shape(0.5, 0.5)

    def both(shape, poses, d):
        best = dw.shape_distance_closest(shape, poses, d)
        offs, hits = dw.query_shapes_within(shape, poses, d)
        dd = np.broadcast_to(np.asarray(d, np.float32), (len(poses),))
        for i in range(len(poses)):
            ids, vals = host_distances(hw, shape, poses[i], dd[i])
            closest_matches(best[i], ids, vals)
            within_matches(hits[offs[i]:offs[i + 1]], ids, vals)
        return best, offs, hits

    # two boxes created beside the rain, a circle exactly between them: a tie only if the bits agree - the drop-in's answer
    ra = L.b2h_edit(hw.ptr, 0, -1, -30.0, 40.0, 0.0)
    rb = L.b2h_edit(hw.ptr, 0, -1, -24.0, 40.0, 0.0)
    assert ra >= 0 and rb >= 0
    rows = fixture_rows(hw)
    between = np.array([[-27.0, 40.0, 0.0], [-26.5, 40.0, 0.0]], np.float32)
    best, offs, hits = both(circle, between, 4.0)
    assert {int(rows[f, 0]) for f in hits["fixture"][offs[0]:offs[1]]} == {ra, rb}
    assert rows[best[1]["fixture"], 0] == rb
    # a pose at 2e8 m (every proxy scanned), with and without anything in range
    far = np.array([[2.0e8, 0.0, 0.3], [2.0e8, 0.0, 0.3]], np.float32)
    both(circle, far, [5.0, 3.0e8])
    # set_transform between steps, seen without a step
    assert L.b2h_edit(hw.ptr, 2, ra, 30.0, 45.0, 0.7) == 0
    moved = np.array([[30.0, 47.0, 0.0], [-30.0, 42.0, 0.0]], np.float32)
    best, offs, hits = both(box, moved, 1.5)
    assert rows[best[0]["fixture"], 0] == ra and best[0]["distance"] > 0.0
    assert ra not in rows[hits["fixture"][offs[1]:offs[2]], 0].tolist()
    # two identical calls: the same bytes
    rng = np.random.default_rng(41)
    shapes = probe_shapes(rng)
    poses = poses_near(hw, 200, rng)
    idx = rng.integers(0, len(shapes), 200).astype(np.int32)
    d = rng.uniform(0.0, 8.0, 200).astype(np.float32)
    h1 = dw.shape_distance_closest(shapes, poses, d, shape_index=idx)
    h2 = dw.shape_distance_closest(shapes, poses, d, shape_index=idx)
    assert h1.tobytes() == h2.tobytes()
    o1, w1 = dw.query_shapes_within(shapes, poses, d, shape_index=idx)
    o2, w2 = dw.query_shapes_within(shapes, poses, d, shape_index=idx)
    assert o1.tobytes() == o2.tobytes() and w1.tobytes() == w2.tobytes()
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_distance_queries_do_not_perturb_the_step(amd):
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
        d = rng.uniform(0.0, 10.0, 48).astype(np.float32)
        dw.shape_distance_closest(shapes, poses, d, shape_index=idx)
        dw.query_shapes_within(shapes, poses, d, shape_index=idx)
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
    circle = b2hip.circle_shape(1.0)
    pose = np.zeros((1, 3), np.float32)
    assert len(w.query_shapes_within(circle, pose, 30.0)[1]) == 7
    assert w.shape_distance_closest(circle, pose, 30.0)[0]["fixture"] == 0
    w.set_flags(continuous=True, sub_stepping=True)
    refused = 0
    for _ in range(12):
        w.step()
        try:
            w.shape_distance_closest(circle, pose, 30.0)
        except b2hip.B2HipError as e:
            assert "error -1" in str(e) and "inside a step" in str(e)
            with pytest.raises(b2hip.B2HipError, match="error -1") as info:
                w.query_shapes_within(circle, pose, 30.0)
            assert "inside a step" in str(info.value)
            refused += 1
    assert refused > 0, "no call left the step open"
    w.close()
    s = b2hip.World()
    g = s.create_body(b2hip.STATIC, (0.0, 0.0))
    s.create_fixture(g, b2hip.box_shape(20.0, 0.05))
    s.step()
    assert b2hip.lib().b2hip_set_shard(s.p, 0, 2) == 0
    with pytest.raises(b2hip.B2HipError, match="error -4"):
        s.shape_distance_closest(circle, pose, 30.0)
    with pytest.raises(b2hip.B2HipError, match="error -4"):
        s.query_shapes_within(circle, pose, 30.0)
    s.close()
