"""GPU: batched all-hit and any-hit ray casts on the device (include/b2hip.h: b2hip_ray_cast_all, b2hip_ray_cast_any) against
the drop-in's b2World::RayCast with a callback that returns 1 (every fixture the ray crosses) on the SAME world, the device
world behind the drop-in. Per ray the records equal the drop-in's list bit for bit as a multiset (the tree's order is not the
device's), the keys (bits of fraction + 0.0f, fixture id) ascend strictly, the first record is b2hip_ray_cast_closest's, and
the any-hit byte says whether the list is empty."""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
from test_gpu_queries_batch import SCENES, _bind, _hashes, batch, device, fixture_filters, fixture_rows

# Every scene of test_gpu_queries_batch.SCENES but field200k. The condition each must meet - some ray hits, and more records
# than hitting rays - was checked beforehand with the same batches on the reference build of the harness alone, on the CPU
# (hitting rays / records of 1000 rays): rain 764 / 6165, sensors 731 / 2933, field 491 / 1320, circles 765 / 2224,
# chains 719 / 2270, tumbler 643 / 12661, bullets_ccd 466 / 688. None had to be dropped.
RAY_SCENES = [s for s in SCENES if s[0] != "field200k"]


def _bind_all(hw):
    L = hw.L  # (the public Box2D API only: the reference build of the harness has it too)
    L.b2h_raycast_all_filtered.argtypes = [C.c_void_p] + [C.c_float] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.b2h_raycast_all_filtered.restype = C.c_int
    return L


def host_all(hw, p1, p2, mask=0xFFFF, sensors=True, cap=4096):
    """the drop-in's hits of one ray among the fixtures the filter passes, in the tree's order: (count, 7) rows of
    body, fixture index in body, point.xy, normal.xy, fraction"""
    L = _bind_all(hw)
    out = np.zeros((cap, 7), np.float32)
    n = L.b2h_raycast_all_filtered(hw.ptr, float(p1[0]), float(p1[1]), float(p2[0]), float(p2[1]), mask, int(sensors), cap,
                                   out.ctypes.data_as(C.c_void_p))
    assert 0 <= n <= cap
    return out[:n]


def keys_of(hits):
    """(bits of fraction + 0.0f) << 32 | fixture id: the order the header states"""
    bits = (hits["fraction"] + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | hits["fixture"].astype(np.uint64)


def as_rows(rows, hits):
    """device records in the drop-in's out7 layout, as raw bits, sorted"""
    bf = rows[hits["fixture"]].astype(np.float32)
    m = np.concatenate([bf, hits["point"], hits["normal"], hits["fraction"][:, None]], axis=1).astype(np.float32)
    return sorted(map(tuple, m.view(np.uint32).tolist()))


def check_rays(hw, dw, rows, p1, p2, mask=0xFFFF, sensors=True):
    """both calls on one batch against the drop-in; returns (rays that hit, records)"""
    n = len(p1)
    offs, hits = dw.ray_cast_all(p1, p2, mask=mask, sensors=sensors)
    closest = dw.ray_cast_closest(p1, p2, mask=mask, sensors=sensors)
    some = dw.ray_cast_any(p1, p2, mask=mask, sensors=sensors)
    assert len(offs) == n + 1 and offs[0] == 0 and offs[-1] == len(hits)
    counts = np.diff(offs)
    assert np.all(counts >= 0)
    assert some.dtype == bool and np.array_equal(some, counts > 0)
    assert np.array_equal(some, closest["fixture"] >= 0)
    assert np.all(hits["pad"] == 0)
    keys = keys_of(hits)
    for i in range(n):
        seg = hits[offs[i]:offs[i + 1]]
        k = keys[offs[i]:offs[i + 1]]
        assert np.all(k[1:] > k[:-1]), "ray %d: keys not strictly ascending" % i
        assert len(np.unique(seg["fixture"])) == len(seg), "ray %d: a fixture twice" % i
        if len(seg):
            assert seg[0].tobytes() == closest[i].tobytes(), "ray %d: the first record is not the closest hit" % i
        want = host_all(hw, p1[i], p2[i], mask, sensors)
        assert as_rows(rows, seg) == sorted(map(tuple, want.view(np.uint32).tolist())), \
            "ray %d: %d records, the drop-in reports %d" % (i, len(seg), len(want))
    return int((counts > 0).sum()), len(hits)


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene,kw,steps", RAY_SCENES)
def test_all_hits_match_the_dropin(amd, name, scene, kw, steps):
    hw = amd.world(scene, **kw)
    hw.step(steps)
    dw = device(hw)
    rows = fixture_rows(hw)
    _, _, _, p1, p2 = batch(hw, 1000, np.random.default_rng(7))
    hitting, records = check_rays(hw, dw, rows, p1, p2)
    assert hitting > 0, "no ray hits"
    assert records > hitting, "no ray with more than one hit: the multi-hit path is not exercised"
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_filters_equal_the_filtered_dropin_answers(amd):
    """mask / sensor settings: the lists against the drop-in's RayCast whose callback skips (-1) what the filter rejects"""
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
    dw = device(hw)
    rows = fixture_rows(hw)
    flt = fixture_filters(hw)
    live = rows[:, 0] >= 0
    cats = set(flt[live, 0].tolist())
    assert {1, 2, 4} <= cats and flt[live, 1].sum() >= 3, (cats, flt[live, 1].sum())
    _, _, _, p1, p2 = batch(hw, 300, np.random.default_rng(3))
    totals = {}
    for mask in (0xFFFF, 0x0001, 0x0002, 0x0006, 0xFFFE):
        for sensors in (True, False):
            totals[mask, sensors] = check_rays(hw, dw, rows, p1, p2, mask, sensors)[1]
    assert totals[0xFFFF, True] > 0
    assert totals[0xFFFF, False] < totals[0xFFFF, True] and totals[0x0002, True] < totals[0xFFFF, True], totals
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_long_lists_and_every_walk():
    """4200 small static boxes in a row, a 3 m wide box behind them and two identical boxes at one place behind that. Ray (a)
    covers the first 1000 (the LDS sort), (b) the whole row (4203 hits: the long-list sort), (c) is (b) lengthened to 30 km,
    more than 4096 grid cells whatever the cell (every proxy scanned), (d) is (b) reversed."""
    w = b2hip.World(gravity=(0.0, 0.0))
    pitch, count = 0.26, 4200
    ids = []
    for i in range(count):
        b = w.create_body(b2hip.STATIC, (i * pitch, 0.0))
        ids.append(w.create_fixture(b, b2hip.box_shape(0.125, 0.125)))
    b = w.create_body(b2hip.STATIC, (count * pitch + 1.5, 0.0))  # its left face at 1092.0
    wide = w.create_fixture(b, b2hip.box_shape(1.5, 0.125))
    twins = []
    for _ in range(2):
        b = w.create_body(b2hip.STATIC, (1097.0, 0.0))
        twins.append(w.create_fixture(b, b2hip.box_shape(0.125, 0.125)))
    assert twins[0] < twins[1]
    w.step()
    forward = ids + [wide] + twins
    p1 = np.array([[-1.0, 0.0], [-1.0, 0.0], [-1.0, 0.0], [1100.0, 0.0]], np.float32)
    p2 = np.array([[999 * pitch, 0.0], [1100.0, 0.0], [30000.0, 0.0], [-1.0, 0.0]], np.float32)
    offs, hits = w.ray_cast_all(p1, p2)
    a, b_, c, d = (hits[offs[i]:offs[i + 1]] for i in range(4))
    assert len(b_) == len(forward) > 4096
    assert a["fixture"].tolist() == ids[:1000]
    assert b_["fixture"].tolist() == forward
    assert c["fixture"].tolist() == forward
    assert d["fixture"].tolist() == twins + [wide] + ids[::-1]
    assert np.abs(b_["point"] - c["point"]).max() <= 1e-3
    for seg in (a, b_, c, d):
        k = keys_of(seg)
        assert np.all(k[1:] > k[:-1])
    left = np.arange(count, dtype=np.float64) * pitch - 0.125  # (the polygon cast ignores the skin)
    assert np.abs(a["point"][:, 0] - left[:1000]).max() <= 1e-3
    assert np.abs(b_["point"][:count, 0] - left).max() <= 1e-3
    assert np.abs(d["point"][3:, 0] - (left[::-1] + 0.25)).max() <= 1e-3  # (the reversed ray meets the right faces)
    assert np.all(hits["point"][:, 1] == 0.0)
    assert abs(b_["point"][count, 0] - 1092.0) <= 1e-3 and (b_["fixture"] == wide).sum() == 1
    for seg in (b_, c, d):
        t = seg[np.isin(seg["fixture"], twins)]
        assert t["fixture"].tolist() == twins and t["fraction"][0].tobytes() == t["fraction"][1].tobytes()
    assert np.array_equal(w.ray_cast_any(p1, p2), np.ones(4, bool))
    assert w.ray_cast_closest(p1, p2).tobytes() == hits[offs[:4]].tobytes()
    # a cap below the total: the total, complete offsets, the first half of the records
    total = len(hits)
    rays = np.ascontiguousarray(np.concatenate([p1, p2], 1), np.float32)
    o2 = np.zeros(5, np.int32)
    h2 = np.zeros(total // 2, b2hip.RAY_HIT_DTYPE)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert b2hip.lib().b2hip_ray_cast_all(w.p, 4, vp(rays), None, total // 2, vp(o2), vp(h2)) == total
    assert np.array_equal(o2, offs) and h2.tobytes() == hits[:total // 2].tobytes()
    w.close()


@pytest.mark.gpu
def test_edges_of_the_contract(amd):
    hw = amd.world(bh.SENSORS, p0=40, seed=5)
    hw.step(10)
    L = _bind(hw)
    assert L.b2h_edit(hw.ptr, 0, -1, 5.5, -3.0, 0.0) >= 0  # a box below the ground, on the last ray
    dw = device(hw)
    rows = fixture_rows(hw)
    z = np.zeros((0, 2), np.float32)
    offs, hits = dw.ray_cast_all(z, z)
    assert offs.tolist() == [0] and len(hits) == 0 and hits.dtype == b2hip.RAY_HIT_DTYPE
    assert len(dw.ray_cast_any(z, z)) == 0
    # zero-length and NaN rays: an empty list / 0
    nan = np.float32("nan")
    r1 = np.array([[0, 5], [nan, 1], [1, 1], [0, np.inf]], np.float32)
    r2 = np.array([[0, 5], [3, 1], [nan, 4], [0, 0]], np.float32)
    offs, hits = dw.ray_cast_all(r1, r2)
    assert offs.tolist() == [0] * 5 and len(hits) == 0
    assert not dw.ray_cast_any(r1, r2).any()
    # the same batch, the same bytes
    _, _, _, p1, p2 = batch(hw, 300, np.random.default_rng(9))
    o1, h1 = dw.ray_cast_all(p1, p2)
    o2, h2 = dw.ray_cast_all(p1, p2)
    assert len(h1) > 0 and o1.tobytes() == o2.tobytes() and h1.tobytes() == h2.tobytes()
    assert dw.ray_cast_any(p1, p2).tobytes() == dw.ray_cast_any(p1, p2).tobytes()
    # a ray that starts on the ground edge: the edge at fraction 0.0 first (b2EdgeShape::RayCast gives -0.0 or +0.0 there),
    # the box below it second, as the drop-in lists them
    e1, e2 = np.array([[5.5, 0.0]], np.float32), np.array([[5.5, -10.0]], np.float32)
    offs, hits = dw.ray_cast_all(e1, e2)
    want = host_all(hw, e1[0], e2[0])
    assert len(hits) >= 2 and as_rows(rows, hits) == sorted(map(tuple, want.view(np.uint32).tolist()))
    want = want[np.argsort(want[:, 6], kind="stable")]
    assert hits["fraction"][0] == 0.0 and hits["fraction"][1] > 0.0 and want[0, 6] == 0.0
    assert [tuple(rows[f]) for f in hits["fixture"][:2]] == [(int(r[0]), int(r[1])) for r in want[:2]]
    assert hits[0].tobytes() == dw.ray_cast_closest(e1, e2)[0].tobytes()
    dw.close()
    hw.close()


@pytest.mark.gpu
def test_the_ray_casts_do_not_perturb_the_step(amd):
    kw = dict(p0=200, seed=3)
    a, b = amd.world(bh.RAIN, **kw), amd.world(bh.RAIN, **kw)
    rng = np.random.default_rng(5)
    dw = device(a)
    records = 0
    for _ in range(60):
        a.step(1)
        b.step(1)
        _, _, _, p1, p2 = batch(a, 64, rng)
        records += len(dw.ray_cast_all(p1, p2)[1])
        dw.ray_cast_any(p1, p2)
    dw.close()
    assert records > 0
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
    lo, hi = np.array([[-30, -30]], np.float32), np.array([[30, 30]], np.float32)
    assert len(w.ray_cast_all(lo, hi)[1]) >= 1 and w.ray_cast_any(lo, hi).all()
    w.set_flags(continuous=True, sub_stepping=True)
    refused = 0
    for _ in range(12):
        w.step()  # (the boxes reach the platform in the third step: six impacts, one per call, the step stays open)
        try:
            w.ray_cast_all(lo, hi)
        except b2hip.B2HipError as e:
            assert "error -1" in str(e) and "inside a step" in str(e)
            with pytest.raises(b2hip.B2HipError, match="error -1"):
                w.ray_cast_any(lo, hi)
            refused += 1
    assert refused > 0, "no call left the step open"
    w.close()
    s = b2hip.World()
    g = s.create_body(b2hip.STATIC, (0.0, 0.0))
    s.create_fixture(g, b2hip.box_shape(20.0, 0.05))
    s.step()
    assert b2hip.lib().b2hip_set_shard(s.p, 0, 2) == 0
    with pytest.raises(b2hip.B2HipError, match="error -4"):
        s.ray_cast_all(lo, hi)
    with pytest.raises(b2hip.B2HipError, match="error -4"):
        s.ray_cast_any(lo, hi)
    s.close()
