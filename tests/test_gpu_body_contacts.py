"""GPU: per-body contact lists and totals on the device (include/b2hip.h: b2hip_body_contacts, b2hip_body_contact_totals)
against tests/body_contacts_ref.py over World.contacts() and World.body_states() read at the same point. Index sets, order,
ids, counts, points, the largest impulse and the records' impulses are exact; normals and the totals' sums are bounded as the
reference's docstring derives."""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
import body_contacts_ref as ref
import test_gpu_queries_batch as qb

LONG_ROW = 4200  # boxes on one ground: more than QUERY_SORT_MAX (4096) contacts on one body


def ask(w, bodies):
    """both lists and the totals of `bodies`: {0: (offsets, records) of all contacts, 1: of the touching ones, 'totals': ...}"""
    bodies = np.asarray(bodies, np.int32)
    return {0: w.body_contacts(bodies, touching_only=False), 1: w.body_contacts(bodies, touching_only=True),
            "totals": w.body_contact_totals(bodies)}


def check(w, bodies, got=None):
    """the device's answer for `bodies` against the reference over contacts() / body_states() read now; returns
    (answer, contacts, states)"""
    bodies = np.asarray(bodies, np.int32)
    got = got if got is not None else ask(w, bodies)
    c, s = w.contacts(), w.body_states()
    exempt = 0
    for only in (0, 1):
        ro, rr = ref.lists(c, s, bodies, bool(only))
        exempt += ref.check_lists(got[only][0], got[only][1], ro, rr)
    assert exempt == 0, "a circles manifold with its centres closer than 1e-5: its normal went unchecked"
    ref.check_totals(got["totals"], got[1][0], got[1][1], ref.totals(c, s, bodies))
    return got, c, s


def box_at(hx, hy, cx, cy):
    """a box fixture shape centred at (cx, cy) of its body"""
    s = b2hip.box_shape(hx, hy)
    for i in range(4):
        s.verts[2 * i] += cx
        s.verts[2 * i + 1] += cy
    s.centroid[0], s.centroid[1] = cx, cy
    return s


def hand_made_world(library=None):
    """a ground, a stack of three boxes, a row of four resting boxes, two touching circles, a sensor over the first box of the
    row, a body far from everything, a body with two fixtures, a box hovering over the row; returns (world, names -> body ids)"""
    w = b2hip.World(allow_sleep=False, library=library)
    ids = {}
    ids["ground"] = w.create_body(b2hip.STATIC, (0.0, -0.5))
    w.create_fixture(ids["ground"], b2hip.box_shape(30.0, 0.5))
    ids["stack"] = []
    for k in range(3):
        b = w.create_body(b2hip.DYNAMIC, (-8.0, 0.5 + 1.0 * k))
        w.create_fixture(b, b2hip.box_shape(0.5, 0.5), density=1.0)
        ids["stack"].append(b)
    ids["row"] = []
    for k in range(4):
        b = w.create_body(b2hip.DYNAMIC, (-3.0 + 1.5 * k, 0.5), angle=0.0 if k != 2 else np.pi / 2)
        w.create_fixture(b, b2hip.box_shape(0.5, 0.5), density=1.0 + k)
        ids["row"].append(b)
    ids["circles"] = []
    for x in (6.0, 6.9):
        b = w.create_body(b2hip.DYNAMIC, (x, 0.5))
        w.create_fixture(b, b2hip.circle_shape(0.5), density=1.0)
        ids["circles"].append(b)
    ids["sensor"] = w.create_body(b2hip.STATIC, (-3.0, 0.6))
    w.create_fixture(ids["sensor"], b2hip.box_shape(0.3, 0.3), sensor=True)
    ids["far"] = w.create_body(b2hip.DYNAMIC, (100.0, 50.0), gravity_scale=0.0)
    w.create_fixture(ids["far"], b2hip.box_shape(0.5, 0.5), density=1.0)
    ids["two"] = w.create_body(b2hip.DYNAMIC, (12.0, 0.5))
    w.create_fixture(ids["two"], b2hip.box_shape(0.5, 0.5), density=1.0)
    w.create_fixture(ids["two"], box_at(0.5, 0.5, 1.0, 0.0), density=1.0)
    # ... and a weightless box 0.1 m above the last box of the row: the fat boxes overlap, a contact that is not touching
    ids["hover"] = w.create_body(b2hip.DYNAMIC, (1.5, 1.6), gravity_scale=0.0)
    w.create_fixture(ids["hover"], b2hip.box_shape(0.5, 0.5), density=1.0)
    return w, ids


def hand_made_is_meaningful(got, c, bodies, ids):
    """what makes the hand-made run a test: the kinds of record it must hold (bodies: the batch, in its order)"""
    offs, r = got[1]
    owner = np.repeat(np.asarray(bodies), np.diff(offs))  # the body each touching record belongs to
    k = r["contact_index"]
    assert np.any(c["manifold_type"][k] == ref.CIRCLES), "no circles manifold"
    assert np.any(c["point_count"][k] == 0), "no touching record without points (the sensor)"
    assert np.any(c["point_count"][k] == 2), "no two-point contact"
    sides = {(int(b), bool(c["body_a"][i] == b)) for b, i in zip(owner, k)}
    assert any((b, True) in sides and (b, False) in sides for b, _ in sides), "no body on both sides of different contacts"
    # a contact between two asked-for bodies: its two records are equal and opposite
    mid, top = ids["stack"][1], ids["stack"][2]
    mine = r[(owner == mid) & (r["other_body"] == top)]
    theirs = r[(owner == top) & (r["other_body"] == mid)]
    assert len(mine) == 1 and len(theirs) == 1 and mine["contact_index"][0] == theirs["contact_index"][0]
    assert np.array_equal(mine["normal"][0], -theirs["normal"][0]) and np.any(mine["normal"][0] != 0)
    assert mine["normal_impulse"][0] == theirs["normal_impulse"][0] > 0
    assert mine["tangent_impulse"][0] == theirs["tangent_impulse"][0]
    assert (mine["fixture"][0], mine["other_fixture"][0]) == (theirs["other_fixture"][0], theirs["fixture"][0])
    t = got["totals"]
    where = {int(b): i for i, b in enumerate(bodies)}
    assert t["impulse"][where[ids["row"][1]]][1] > 0, "the ground does not push a resting box up"
    assert t["impulse"][where[ids["ground"]]][1] < 0, "the boxes do not push the ground down"
    assert t["contacts"][where[ids["two"]]] == 2 and t["contacts"][where[ids["far"]]] == 0
    assert not np.array_equal(got[0][0], got[1][0]), "no contact that is not touching"


@pytest.mark.gpu
def test_hand_made_world():
    w, ids = hand_made_world()
    for _ in range(60):
        w.step()
    bodies = np.random.default_rng(3).permutation(w.body_count).astype(np.int32)
    got, c, _ = check(w, bodies)
    hand_made_is_meaningful(got, c, bodies, ids)
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene,kw,steps", [s for s in qb.SCENES if s[0] != "field200k"])
def test_harness_scenes(amd, name, scene, kw, steps):
    hw = amd.world(scene, **kw)
    hw.step(steps)
    dw = qb.device(hw)
    got, _, _ = check(dw, np.arange(dw.body_count, dtype=np.int32))
    assert len(got[1][1]) > 0, "no touching record in this scene"
    dw.close()
    hw.close()


def long_row_world(library=None):
    w = b2hip.World(allow_sleep=False, library=library)
    g = w.create_body(b2hip.STATIC, (525.0, -0.5))
    w.create_fixture(g, b2hip.box_shape(600.0, 0.5))
    for k in range(LONG_ROW):
        b = w.create_body(b2hip.DYNAMIC, (0.25 * k, 0.1))
        w.create_fixture(b, b2hip.box_shape(0.1, 0.1), density=1.0)
    return w, g


@pytest.mark.gpu
def test_a_long_list():
    """one ground under 4 200 boxes: its list takes the long-list ordering, its counters and cursor the same-address path"""
    w, g = long_row_world()
    for _ in range(5):
        w.step()
    got, c, _ = check(w, [g])
    assert got["totals"]["touching"][0] == LONG_ROW > 4096 and got["totals"]["impulse"][0][1] < 0
    rng = np.random.default_rng(5)
    batch = np.concatenate([[g], 1 + rng.choice(LONG_ROW, 100, replace=False)]).astype(np.int32)
    rng.shuffle(batch)
    got, _, _ = check(w, batch)
    # a cap below the total: the prefix of the full answer, the total returned, the offsets complete
    offs, full = got[0]
    total = len(full)
    assert total > LONG_ROW
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for cap in (total // 2, 1, 0):
        o2 = np.full(len(batch) + 1, -7, np.int32)
        r2 = np.zeros(max(cap, 1), b2hip.BODY_CONTACT_DTYPE)
        assert b2hip.lib().b2hip_body_contacts(w.p, len(batch), vp(batch), 0, cap, vp(o2), vp(r2) if cap else None) == total
        assert np.array_equal(o2, offs) and r2[:cap].tobytes() == full[:cap].tobytes()
    w.close()


@pytest.mark.gpu
def test_edge_cases():
    w, ids = hand_made_world()
    w.set_lazy_readback(True)
    for _ in range(30):
        w.step()
    none = np.zeros(0, np.int32)
    offs, r = w.body_contacts(none)
    assert offs.tolist() == [0] and len(r) == 0 and len(w.body_contact_totals(none)) == 0
    got, c, _ = check(w, [ids["row"][0]])                      # n = 1
    assert got["totals"]["touching"][0] >= 2                   # (the ground and the sensor)
    assert len(c) % 64 != 0, "the contact count is a multiple of 64: the last wave of the walk is full"
    got, _, _ = check(w, [ids["far"]])                         # a batch of bodies without contacts
    assert got[0][0].tolist() == [0, 0] and not got["totals"].tobytes().strip(b"\0")
    # the same call twice: the same bytes
    bodies = np.arange(w.body_count, dtype=np.int32)
    a, b = ask(w, bodies), ask(w, bodies)
    for key in (0, 1):
        assert a[key][0].tobytes() == b[key][0].tobytes() and a[key][1].tobytes() == b[key][1].tobytes()
    assert a["totals"].tobytes() == b["totals"].tobytes()
    check(w, bodies, a)                                        # lazy read-back on
    w.close()
    # a world without contacts
    e = b2hip.World(gravity=(0.0, 0.0))
    for x in (0.0, 50.0):
        b = e.create_body(b2hip.DYNAMIC, (x, 0.0))
        e.create_fixture(b, b2hip.box_shape(0.5, 0.5), density=1.0)
    got, c, _ = check(e, [1, 0])                               # (before the first step: no contact array yet)
    e.step()
    got, c, _ = check(e, [1, 0])
    assert len(c) == 0 and got[0][0].tolist() == [0, 0, 0] and not got["totals"].tobytes().strip(b"\0")
    e.close()


@pytest.mark.gpu
def test_edits_between_steps_are_seen():
    w, ids = hand_made_world()
    for _ in range(60):
        w.step()
    L = b2hip.lib()
    L.b2hip_set_transform.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    gone, moved = ids["stack"][1], ids["row"][1]
    before = w.body_contact_totals([gone, moved])
    assert before["touching"][0] == 2 and before["touching"][1] == 1
    w.destroy_body(gone)
    assert L.b2hip_set_transform(w.p, moved, -1.3, 0.52, 0.3) == 0
    new = w.create_body(b2hip.DYNAMIC, (3.0, 3.0))
    w.create_fixture(new, b2hip.box_shape(0.5, 0.5), density=1.0)
    bodies = np.random.default_rng(4).permutation(w.body_count).astype(np.int32)
    got = ask(w, bodies)                # (no step in between: the device call applies the edits itself ...)
    got, c, s = check(w, bodies, got)   # (... and agrees with contacts() / body_states() read afterwards)
    assert not np.any((c["body_a"] == gone) | (c["body_b"] == gone))
    where = {int(b): i for i, b in enumerate(bodies)}
    for key in (0, 1):
        offs = got[key][0]
        assert offs[where[gone] + 1] == offs[where[gone]] and offs[where[new] + 1] == offs[where[new]]
    assert not got["totals"][where[gone]].tobytes().strip(b"\0")
    # the moved box's record uses the transform that was set: its face normal is turned by 0.3 rad against the ground's
    offs, r = got[1]
    mine = r[offs[where[moved]]:offs[where[moved] + 1]]
    assert len(mine) == 1 and mine["other_body"][0] == ids["ground"]
    assert s["angle"][moved] == np.float32(0.3)
    k = mine["contact_index"][0]
    turned = c["manifold_type"][k] == (ref.FACE_A if c["body_a"][k] == moved else ref.FACE_B)
    want = (-np.sin(0.3), np.cos(0.3)) if turned else (0.0, 1.0)
    assert np.allclose(mine["normal"][0], want, rtol=0, atol=1e-6)
    w.step()
    check(w, bodies)
    w.close()


@pytest.mark.gpu
def test_bad_ids_are_refused_and_the_world_still_steps():
    w, ids = hand_made_world()
    for _ in range(10):
        w.step()
    n = w.body_count
    for bad, word in (([0, 1, n], str(n)), ([2, -1], "-1"), ([3, 5, 3, 5], "3"), ([n + 7, 1, 1], str(n + 7))):
        for call in (w.body_contacts, w.body_contact_totals):
            with pytest.raises(b2hip.B2HipError, match="error -1") as e:
                call(np.asarray(bad, np.int32))
            assert ("body " + word) in str(e.value), str(e.value)
    for _ in range(10):
        w.step()
    check(w, np.arange(n, dtype=np.int32))
    w.close()


@pytest.mark.gpu
def test_refused_inside_an_open_step_and_on_a_sharded_world():
    w = b2hip.World(continuous=True)
    g = w.create_body(b2hip.STATIC, (0.0, 0.0))
    w.create_fixture(g, b2hip.box_shape(20.0, 0.05))
    for k in range(6):
        b = w.create_body(b2hip.DYNAMIC, (-5.0 + 2.0 * k, 3.0 + 0.1 * k), velocity=(1.0 * k, -60.0))
        w.create_fixture(b, b2hip.box_shape(0.1, 0.1), density=1.0)
    bodies = np.arange(7, dtype=np.int32)
    assert len(w.body_contact_totals(bodies)) == 7
    w.set_flags(continuous=True, sub_stepping=True)
    refused = 0
    for _ in range(12):
        w.step()  # (the boxes reach the platform in the third step: six impacts, one per call, the step stays open)
        try:
            w.body_contacts(bodies)
        except b2hip.B2HipError as e:
            assert "error -1" in str(e) and "inside a step" in str(e)
            with pytest.raises(b2hip.B2HipError, match="error -1"):
                w.body_contact_totals(bodies)
            refused += 1
    assert refused > 0, "no call left the step open"
    w.close()
    s = b2hip.World()
    g = s.create_body(b2hip.STATIC, (0.0, 0.0))
    s.create_fixture(g, b2hip.box_shape(20.0, 0.05))
    s.step()
    assert b2hip.lib().b2hip_set_shard(s.p, 0, 2) == 0
    for call in (s.body_contacts, s.body_contact_totals):
        with pytest.raises(b2hip.B2HipError, match="error -4"):
            call(np.zeros(1, np.int32))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene,kw,lazy", [("rain", bh.RAIN, dict(p0=200, seed=3), False),
                                                ("rain_lazy", bh.RAIN, dict(p0=200, seed=3), True),
                                                ("bullets_ccd", bh.BULLETS, dict(p0=20, p1=4, flags=qb.CCD, seed=5), False),
                                                ("bullets_ccd_lazy", bh.BULLETS, dict(p0=20, p1=4, flags=qb.CCD, seed=5), True)])
def test_the_calls_do_not_perturb_the_step(amd, name, scene, kw, lazy):
    a, b = amd.world(scene, **kw), amd.world(scene, **kw)
    if lazy:
        for hw in (a, b):
            assert b2hip.lib().b2hip_set_lazy_readback(C.c_void_p(hw.device_world()), 1) == 0
    dw = qb.device(a)
    rng = np.random.default_rng(5)
    asked = 0
    for k in range(120):
        a.step(1)
        b.step(1)
        if k in (40, 80):  # edits on both twins; only `a` is asked before the next step
            for hw in (a, b):
                assert qb._bind(hw).b2h_edit(hw.ptr, 2, 7, -4.0 + 0.01 * k, 15.0, 1.1) == 0  # SetTransform
                if k == 80:
                    assert qb._bind(hw).b2h_edit(hw.ptr, 1, 5, 0.0, 0.0, 0.0) == 0             # a fixture destroyed
        n = dw.body_count
        bodies = rng.permutation(n)[:max(1, n // 2 if k % 2 else n)].astype(np.int32)
        asked += len(dw.body_contacts(bodies, touching_only=bool(k % 3))[1])
        dw.body_contact_totals(bodies)
    assert asked > 0
    dw.close()
    assert np.array_equal(a.bodies().view(np.uint32), b.bodies().view(np.uint32))
    assert qb._hashes(a) == qb._hashes(b)
    a.close()
    b.close()
