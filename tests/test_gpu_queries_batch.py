"""GPU: batched AABB, point and closest-ray queries on the device (include/b2hip.h: b2hip_query_aabbs, b2hip_query_points,
b2hip_ray_cast_closest) against the drop-in's host queries (b2World::QueryAABB / RayCast over its shadow tree) on the SAME
world: the device world behind the drop-in (Harness.device_world()). Sets equal; closest hits equal as raw bits, except where
two fixtures tie in fraction (the device keeps the lower id, the tree the one it visits last): there the fraction alone."""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip

CCD = bh.F_CONTINUOUS | bh.F_SLEEP | bh.F_WARM
SCENES = [("rain", bh.RAIN, dict(p0=200, seed=3), 120), ("sensors", bh.SENSORS, dict(p0=40, seed=5), 100),
          ("field", bh.FIELD, dict(p0=600, p1=0, seed=9), 40), ("circles", bh.CIRCLE_STACK, dict(p0=8, p1=6), 80),
          ("chains", bh.CHAINS, dict(p0=70, flags=CCD, seed=5), 120), ("tumbler", bh.TUMBLER, dict(p0=30, seed=1), 90),
          ("bullets_ccd", bh.BULLETS, dict(p0=20, p1=4, flags=CCD, seed=5), 40),
          ("field200k", bh.FIELD, dict(p0=200000, p1=2000, flags=CCD, seed=3), 4)]


def _bind(hw):
    L = hw.L
    L.b2h_device_fixture_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.b2h_device_fixture_rows.restype = C.c_int
    L.b2h_query_point.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p]
    L.b2h_query_point.restype = C.c_int
    L.b2h_edit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
    L.b2h_edit.restype = C.c_int
    L.b2h_fixture_filters.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.b2h_fixture_filters.restype = C.c_int
    L.b2h_raycast_closest_filtered.argtypes = [C.c_void_p] + [C.c_float] * 4 + [C.c_int, C.c_int, C.c_void_p]
    L.b2h_raycast_closest_filtered.restype = C.c_int
    return L


def fixture_filters(hw):
    """device fixture id -> (categoryBits, is sensor) as the drop-in's host fixtures hold them; -1 rows for ids nobody owns"""
    L = _bind(hw)
    n = L.b2h_fixture_filters(hw.ptr, 0, None)
    out = np.full((max(n, 1), 2), -1, np.int32)
    L.b2h_fixture_filters(hw.ptr, n, out.ctypes.data_as(C.c_void_p))
    return out[:n]


def host_ray_filtered(hw, p1, p2, mask, sensors):
    """the drop-in's closest hit among the fixtures the filter passes (a callback returning -1 for the others)"""
    L = _bind(hw)
    out = np.zeros(7, np.float32)
    if not L.b2h_raycast_closest_filtered(hw.ptr, float(p1[0]), float(p1[1]), float(p2[0]), float(p2[1]), mask, int(sensors),
                                          out.ctypes.data_as(C.c_void_p)):
        return None
    return out


def ray_matches(rows, h, r):
    """one device hit against the drop-in's (None: a miss): 'same' (all bits), 'tie' (same fraction, the device's fixture
    id the lower - the header's tie rule), else an assertion"""
    if r is None:
        assert h["fixture"] == -1, "the device hits, the drop-in does not"
        return "miss"
    assert h["fixture"] >= 0, "the drop-in hits, the device does not"
    b, f = rows[h["fixture"]]
    mine = np.array([b, f, h["point"][0], h["point"][1], h["normal"][0], h["normal"][1], h["fraction"]], np.float32)
    if np.array_equal(mine.view(np.uint32), r.view(np.uint32)):
        return "same"
    # (equal fractions; +0.0 and -0.0 are one value: a ray that starts on a surface)
    assert mine[6] == r[6], "closest hit differs: %s vs %s" % (mine, r)
    ids = np.flatnonzero((rows[:, 0] == int(r[0])) & (rows[:, 1] == int(r[1])))
    if (b, f) != (int(r[0]), int(r[1])):
        # the drop-in kept another fixture at the same fraction: the device's is the lower id (a chain's children share
        # one drop-in row, so the drop-in's child is only known to be one of its ids)
        assert h["fixture"] < (ids.max() if len(ids) > 1 else ids[0]), "tie not won by the lowest fixture id"
    return "tie"


def fixture_rows(hw):
    """device fixture id -> (harness body row, fixture index in body); -1 rows for ids nobody owns"""
    L = _bind(hw)
    n = L.b2h_device_fixture_rows(hw.ptr, 0, None)
    out = np.full((max(n, 1), 2), -1, np.int32)
    L.b2h_device_fixture_rows(hw.ptr, n, out.ctypes.data_as(C.c_void_p))
    return out[:n]


def host_point(hw, p, cap=4096):
    L = _bind(hw)
    out = np.zeros((cap, 2), np.int32)
    n = L.b2h_query_point(hw.ptr, float(p[0]), float(p[1]), cap, out.ctypes.data_as(C.c_void_p))
    return out[:min(n, cap)]


def device(hw):
    return b2hip.World.borrow(hw.device_world())


def rows_of(rows, fixtures):
    r = rows[fixtures]
    return sorted(map(tuple, r.tolist()))


def batch(hw, n, rng):
    b = hw.bodies()
    pos = b[b[:, 7] >= 0][:, :2]
    lo, hi = pos.min(axis=0) - 2.0, pos.max(axis=0) + 2.0
    c = rng.uniform(lo, hi, (n, 2)).astype(np.float32)
    e = rng.uniform(0.2, 6.0, (n, 2)).astype(np.float32)
    pts = np.concatenate([rng.uniform(lo, hi, (n // 2, 2)), pos[rng.integers(0, len(pos), n - n // 2)]]).astype(np.float32)
    p1 = rng.uniform(lo, hi, (n, 2)).astype(np.float32)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    ln = rng.uniform(1.0, 30.0, n)
    p2 = np.where((np.arange(n) % 2 == 0)[:, None], rng.uniform(lo, hi, (n, 2)),
                  p1 + np.stack([np.cos(ang) * ln, np.sin(ang) * ln], 1)).astype(np.float32)
    return c - e, c + e, pts, p1, p2


def check_against_dropin(hw, n=2000, seed=7, mask=0xFFFF, sensors=True):
    """every kind of query on the device against the drop-in's answers; returns (items reported, ray hits, ties)"""
    rng = np.random.default_rng(seed)
    dw = device(hw)
    rows = fixture_rows(hw)
    lo, hi, pts, p1, p2 = batch(hw, n, rng)
    offs, items = dw.query_aabbs(lo, hi, mask=mask, sensors=sensors)
    assert offs[0] == 0 and offs[-1] == len(items)
    reported = 0
    for i in range(n):
        seg = items["fixture"][offs[i]:offs[i + 1]]
        assert np.all(np.diff(seg) > 0), "box %d: items not in ascending fixture id" % i
        got = rows_of(rows, seg)
        want = sorted(map(tuple, hw.query_aabb(lo[i], hi[i]).tolist()))
        assert got == want, "box %d reports another set" % i
        reported += len(seg)
    offs, items = dw.query_points(pts)
    for i in range(n):
        seg = items["fixture"][offs[i]:offs[i + 1]]
        assert np.all(np.diff(seg) > 0)
        assert rows_of(rows, seg) == sorted(map(tuple, host_point(hw, pts[i]).tolist())), "point %d" % i
    hits = dw.ray_cast_closest(p1, p2)
    nhit = ties = 0
    for i in range(n):
        verdict = ray_matches(rows, hits[i], hw.raycast_closest(p1[i], p2[i]))
        nhit += verdict != "miss"
        ties += verdict == "tie"
    dw.close()
    return reported, nhit, ties


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene,kw,steps", SCENES)
def test_batched_queries_match_the_dropin(amd, name, scene, kw, steps):
    hw = amd.world(scene, **kw)
    hw.step(steps)
    reported, nhit, ties = check_against_dropin(hw, n=2000 if name != "field200k" else 1000)
    assert reported > 0 and nhit > 0
    assert ties <= max(2, nhit // 50), "%d ties of %d hits" % (ties, nhit)
    if name == "field200k":
        # a box over the whole world: every live proxy once (the reference's DuplicateProxyTest), past the LDS sort
        dw = device(hw)
        rows = fixture_rows(hw)
        live = np.flatnonzero(rows[:, 0] >= 0)
        offs, items = dw.query_aabbs(np.array([[-1e6, -1e6]], np.float32), np.array([[1e6, 1e6]], np.float32))
        assert np.array_equal(items["fixture"], live)
        lo = np.array([[-1e4, -1e4]], np.float32)
        offs2, items2 = dw.query_aabbs(lo, -lo)  # (also wider than 4096 cells: every proxy scanned, as above)
        assert np.array_equal(items2["fixture"], live)
        dw.close()
    hw.close()


@pytest.mark.gpu
def test_filters_equal_the_filtered_dropin_answers(amd):
    """mask / sensor settings against the drop-in: its unfiltered box and point answers filtered in Python by the host
    fixtures' categoryBits and sensor flags, and its closest hit among the passing fixtures (a callback skipping the others)"""
    hw = amd.world(bh.SENSORS, p0=40, seed=5)
    hw.step(40)
    L = _bind(hw)
    nb = hw.body_count
    # three categories and more sensors, through the drop-in API (b2Fixture::SetFilterData / SetSensor)
    for k in range(2, nb):
        if k % 3 == 0:
            assert L.b2h_edit(hw.ptr, 4, k, 2.0, 0.0, 0.0) == 0
        elif k % 5 == 0:
            assert L.b2h_edit(hw.ptr, 4, k, 4.0, 0.0, 0.0) == 0
        if k % 7 == 0:
            assert L.b2h_edit(hw.ptr, 5, k, 1.0, 0.0, 0.0) == 0
    hw.step(20)
    dw = device(hw)
    rows = fixture_rows(hw)
    flt = fixture_filters(hw)
    live = rows[:, 0] >= 0
    cats = set(flt[live, 0].tolist())
    assert {1, 2, 4} <= cats and flt[live, 1].sum() >= 3, (cats, flt[live, 1].sum())
    rng = np.random.default_rng(3)
    lo, hi, pts, p1, p2 = batch(hw, 400, rng)

    def passes(fid, mask, sensors):
        return (flt[fid, 0] & mask) != 0 and (sensors or flt[fid, 1] == 0)

    host_boxes = [hw.query_aabb(lo[i], hi[i]) for i in range(len(lo))]
    host_pts = [host_point(hw, pts[i]) for i in range(len(pts))]
    # drop-in rows -> device ids (no chains in this scene: one id per row)
    by_row = {tuple(rows[fid]): int(fid) for fid in np.flatnonzero(live)}
    assert len(by_row) == int(live.sum())
    checked = 0
    for mask in (0xFFFF, 0x0001, 0x0002, 0x0006, 0xFFFE):
        for sensors in (True, False):
            offs, items = dw.query_aabbs(lo, hi, mask=mask, sensors=sensors)
            for i in range(len(lo)):
                want = sorted(by_row[r] for r in map(tuple, host_boxes[i].tolist()) if passes(by_row[r], mask, sensors))
                got = items["fixture"][offs[i]:offs[i + 1]].tolist()
                assert got == want, "box %d, mask %#x, sensors %d" % (i, mask, sensors)
                checked += len(got)
            offs, items = dw.query_points(pts, mask=mask, sensors=sensors)
            for i in range(len(pts)):
                want = sorted(by_row[r] for r in map(tuple, host_pts[i].tolist()) if passes(by_row[r], mask, sensors))
                assert items["fixture"][offs[i]:offs[i + 1]].tolist() == want, "point %d, mask %#x" % (i, mask)
            hits = dw.ray_cast_closest(p1, p2, mask=mask, sensors=sensors)
            for i in range(len(p1)):
                ray_matches(rows, hits[i], host_ray_filtered(hw, p1[i], p2[i], mask, sensors))
    assert checked > 0
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_edits_between_steps_are_seen(amd):
    hw = amd.world(bh.RAIN, p0=200, seed=3)
    hw.step(40)
    L = _bind(hw)
    assert L.b2h_edit(hw.ptr, 0, -1, 3.0, 12.0, 0.3) >= 0      # a new body with a box
    assert L.b2h_edit(hw.ptr, 1, 5, 0.0, 0.0, 0.0) == 0        # a fixture destroyed
    assert L.b2h_edit(hw.ptr, 2, 7, -4.0, 15.0, 1.1) == 0      # SetTransform
    assert L.b2h_edit(hw.ptr, 3, 9, 0.0, 0.0, 0.0) == 0        # SetActive(false)
    reported, nhit, _ = check_against_dropin(hw, n=600, seed=11)
    assert reported > 0 and nhit > 0
    hw.step(5)
    check_against_dropin(hw, n=300, seed=12)
    hw.close()


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


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene,kw,lazy", [("rain", bh.RAIN, dict(p0=200, seed=3), False),
                                                ("bullets_ccd", bh.BULLETS, dict(p0=20, p1=4, flags=CCD, seed=5), False),
                                                ("bullets_ccd_lazy", bh.BULLETS, dict(p0=20, p1=4, flags=CCD, seed=5), True)])
def test_queries_do_not_perturb_the_step(amd, name, scene, kw, lazy):
    a, b = amd.world(scene, **kw), amd.world(scene, **kw)
    if lazy:
        for hw in (a, b):
            assert b2hip.lib().b2hip_set_lazy_readback(C.c_void_p(hw.device_world()), 1) == 0
    rng = np.random.default_rng(5)
    dw = device(a)
    for k in range(120):
        a.step(1)
        b.step(1)
        lo, hi, pts, p1, p2 = batch(a, 64, rng)
        dw.query_aabbs(lo, hi)
        dw.query_points(pts)
        dw.ray_cast_closest(p1, p2)
    dw.close()
    assert np.array_equal(a.bodies().view(np.uint32), b.bodies().view(np.uint32))
    assert _hashes(a) == _hashes(b)
    a.close()
    b.close()


@pytest.mark.gpu
def test_edge_cases(amd):
    hw = amd.world(bh.RAIN, p0=200, seed=3)
    hw.step(60)
    dw = device(hw)
    rows = fixture_rows(hw)
    z = np.zeros((0, 2), np.float32)
    offs, items = dw.query_aabbs(z, z)
    assert offs.tolist() == [0] and len(items) == 0
    assert len(dw.ray_cast_closest(z, z)) == 0
    assert len(dw.query_points(z)[1]) == 0
    # n = 1
    offs, items = dw.query_aabbs(np.array([[-5, 0]], np.float32), np.array([[5, 10]], np.float32))
    assert rows_of(rows, items["fixture"]) == sorted(map(tuple, hw.query_aabb((-5, 0), (5, 10)).tolist()))
    # the whole world once
    live = np.flatnonzero(rows[:, 0] >= 0)
    offs, items = dw.query_aabbs(np.array([[-1e5, -1e5]], np.float32), np.array([[1e5, 1e5]], np.float32))
    assert np.array_equal(items["fixture"], live)
    # overflow: a cap below the total, then the same answer in full
    rng = np.random.default_rng(9)
    lo, hi, pts, p1, p2 = batch(hw, 300, rng)
    offs, items = dw.query_aabbs(lo, hi)
    total = len(items)
    assert total > 10
    L = b2hip.lib()
    boxes = np.ascontiguousarray(np.concatenate([lo, hi], 1), np.float32)
    o2 = np.zeros(301, np.int32)
    it2 = np.zeros(total // 2, b2hip.QUERY_ITEM_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = L.b2hip_query_aabbs(dw.p, 300, vp(boxes), None, total // 2, vp(o2), vp(it2))
    assert got == total and np.array_equal(o2, offs) and np.array_equal(it2, items[:total // 2])
    # same batch, same bytes
    offs3, items3 = dw.query_aabbs(lo, hi)
    assert offs3.tobytes() == offs.tobytes() and items3.tobytes() == items.tobytes()
    h1, h2 = dw.ray_cast_closest(p1, p2), dw.ray_cast_closest(p1, p2)
    assert h1.tobytes() == h2.tobytes()
    # zero-length and NaN rays, inverted boxes: misses / nothing
    nan = np.float32("nan")
    r1 = np.array([[0, 5], [nan, 1], [1, 1]], np.float32)
    r2 = np.array([[0, 5], [3, 1], [nan, 4]], np.float32)
    assert np.all(dw.ray_cast_closest(r1, r2)["fixture"] == -1)
    offs, items = dw.query_aabbs(np.array([[5, 5], [0, nan]], np.float32), np.array([[-5, 6], [1, 1]], np.float32))
    assert offs.tolist() == [0, 0, 0]
    # a ray from inside a polygon: no hit on that polygon (b2PolygonShape::RayCast)
    b = hw.bodies()
    k = int(np.flatnonzero(b[:, 7] == 2)[0])
    c = b[k, :2]
    hit = dw.ray_cast_closest(c[None, :], (c + np.float32([0.01, 0.0]))[None, :])
    assert hit[0]["fixture"] == -1 or rows[hit[0]["fixture"]][0] != k
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_refused_inside_an_open_step_and_on_a_sharded_world():
    w = b2hip.World(continuous=True)
    g = w.create_body(b2hip.STATIC, (0.0, 0.0))
    w.create_fixture(g, b2hip.box_shape(20.0, 0.05))
    for k in range(6):
        b = w.create_body(b2hip.DYNAMIC, (-5.0 + 2.0 * k, 3.0 + 0.1 * k), velocity=(1.0 * k, -60.0))
        w.create_fixture(b, b2hip.box_shape(0.1, 0.1), density=1.0)
    lo, hi = np.array([[-30, -30]], np.float32), np.array([[30, 30]], np.float32)
    assert len(w.query_aabbs(lo, hi)[1]) == 7
    w.set_flags(continuous=True, sub_stepping=True)
    refused = 0
    for _ in range(12):
        w.step()  # (the boxes reach the platform in the third step: six impacts, one per call, the step stays open)
        try:
            w.query_aabbs(lo, hi)
        except b2hip.B2HipError as e:
            assert "error -1" in str(e) and "inside a step" in str(e)
            with pytest.raises(b2hip.B2HipError, match="error -1"):
                w.ray_cast_closest(lo, hi)
            refused += 1
    assert refused > 0, "no call left the step open"
    w.close()
    s = b2hip.World()
    g = s.create_body(b2hip.STATIC, (0.0, 0.0))
    s.create_fixture(g, b2hip.box_shape(20.0, 0.05))
    s.step()
    L = b2hip.lib()
    assert L.b2hip_set_shard(s.p, 0, 2) == 0
    with pytest.raises(b2hip.B2HipError, match="error -4"):
        s.query_points(np.zeros((1, 2), np.float32))
    s.close()


@pytest.mark.gpu
def test_a_long_list_through_the_grid():
    """A box whose window stays within 4096 grid cells but holds more than 4096 proxies: the grid path feeds the long-list
    ordering (k_query_mark / k_query_compact_big); a smaller box stays in the LDS sort. Both against the fat AABBs."""
    w = b2hip.World(gravity=(0.0, 0.0))
    side, pitch = 65, 0.26
    for i in range(side):
        for j in range(side):
            b = w.create_body(b2hip.DYNAMIC, (i * pitch, j * pitch))
            w.create_fixture(b, b2hip.box_shape(0.125, 0.125), density=1.0)
    w.step()
    n = side * side
    fat = np.zeros((n, 4), np.float32)
    assert b2hip.lib().b2hip_get_fat_aabbs(w.p, 0, n, fat.ctypes.data_as(C.c_void_p)) == 0
    # the grid's cell is at least half of 1.5 x the widest fixture box at creation (0.25 m + 2 x 0.1 m of extension), the window
    # adds at most 2 cells of margin a side: (17.7 / 0.3375 + 4)^2 = 3 249 cells <= 4096
    for lo, hi in (((-0.5, -0.5), (17.2, 17.2)), ((2.0, 3.0), (9.0, 12.5))):
        assert ((hi[0] - lo[0]) / (0.5 * 1.5 * 0.45) + 4) ** 2 <= 4096
        want = np.flatnonzero((fat[:, 0] <= hi[0]) & (fat[:, 1] <= hi[1]) & (fat[:, 2] >= lo[0]) & (fat[:, 3] >= lo[1]))
        offs, items = w.query_aabbs(np.array([lo], np.float32), np.array([hi], np.float32))
        assert np.array_equal(items["fixture"], want)
        assert np.array_equal(items["body"], want)  # (one fixture per body, created in the same order)
    assert len(w.query_aabbs(np.array([[-0.5, -0.5]], np.float32), np.array([[17.2, 17.2]], np.float32))[1]) == n > 4096
    w.close()


@pytest.mark.gpu
def test_a_ray_that_starts_on_an_edge(amd):
    """A ray from a point of the ground edge meets it at fraction -0.0 (b2EdgeShape::RayCast rejects t < 0 only); a box
    further along must not win over it. The drop-in reports the edge (its tree stops at a zero answer)."""
    hw = amd.world(bh.SENSORS, p0=40, seed=5)
    hw.step(10)
    L = _bind(hw)
    assert L.b2h_edit(hw.ptr, 0, -1, 5.5, -3.0, 0.0) >= 0  # a box below the ground, on the ray
    dw = device(hw)
    rows = fixture_rows(hw)
    p1, p2 = np.array([[5.5, 0.0]], np.float32), np.array([[5.5, -10.0]], np.float32)
    hit = dw.ray_cast_closest(p1, p2)[0]
    r = hw.raycast_closest(p1[0], p2[0])
    assert r is not None and r[6] == 0.0
    assert ray_matches(rows, hit, r) == "same"
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_misses_are_the_same_bytes_from_the_host_and_from_the_device():
    """An empty world runs no kernel: the host writes the miss records. A world of one box queried 1 000 m away runs the
    kernels, which write theirs. One definition serves both (queryRayMiss / queryDistanceMiss): the same bytes."""
    empty = b2hip.World()
    far = b2hip.World()
    far.create_fixture(far.create_body(b2hip.STATIC, (0.0, 0.0)), b2hip.box_shape(0.5, 0.5))
    far.step()
    p1 = np.array([[1000.0, 0.0], [0.0, 1000.0], [-1000.0, -1000.0]], np.float32)
    p2 = p1 + np.float32([1.0, 0.5])
    poses = np.concatenate([p1, np.float32([[0.0], [0.7], [-2.0]])], axis=1)
    moves = np.array([[1.0, 0.0], [0.0, -1.0], [0.5, 0.5]], np.float32)
    circle = b2hip.circle_shape(0.25)
    got = []
    for w in (empty, far):
        fixed = [w.ray_cast_closest(p1, p2), w.shape_cast_closest(circle, poses, moves), w.shape_distance_closest(circle, poses, 1.0)]
        assert all(len(r) == 3 and np.all(r["fixture"] == -1) for r in fixed)
        assert not w.ray_cast_any(p1, p2).any()
        lists = [w.query_aabbs(p1, p2), w.query_points(p1), w.ray_cast_all(p1, p2), w.query_shapes(circle, poses),
                 w.query_shapes_within(circle, poses, 1.0)]
        for offs, items in lists:
            assert offs.tolist() == [0, 0, 0, 0] and len(items) == 0
        got.append([r.tobytes() for r in fixed])
        w.close()
    assert got[0] == got[1]
