"""CPU tests of the per-body contact reference (tests/body_contacts_ref.py): hand-written contacts with answers worked out by
hand, the checkers against corrupted answers, and the float32 evaluation of the normal - what the device computes, op by op -
against float64 inside the bounds the GPU tests use."""
import numpy as np
import pytest

import b2hip
import body_contacts_ref as ref

F32 = np.float32
HALF_PI = float(F32(np.pi / 2))


def hand_made():
    """seven bodies, six contacts; see the comments for what each is there for"""
    s = np.zeros(7, b2hip.BODY_STATE_DTYPE)
    pose = [(0, 0, 0), (0, 1, 0), (3, 1, HALF_PI), (10, 5, 0), (10, 5, 0), (10.6, 5.8, 0), (0.5, 1.5, 0)]
    for i, (x, y, a) in enumerate(pose):
        s[i]["px"], s[i]["py"], s[i]["angle"] = x, y, a
    c = np.zeros(6, b2hip.CONTACT_DTYPE)

    def put(k, a, b, fa, fb, flags, kind, pc, ln=(0, 0), lp=(0, 0), p0=(0, 0), jn=(0, 0), jt=(0, 0)):
        c[k]["body_a"], c[k]["body_b"], c[k]["fixture_a"], c[k]["fixture_b"] = a, b, fa, fb
        c[k]["flags"], c[k]["manifold_type"], c[k]["point_count"] = flags, kind, pc
        c[k]["local_normal"], c[k]["local_point"], c[k]["point_local"][0] = ln, lp, p0
        c[k]["normal_impulse"], c[k]["tangent_impulse"] = jn, jt

    put(0, 0, 1, 100, 101, 3, ref.FACE_A, 2, ln=(0, 1), jn=(2, 3), jt=(0.5, -0.25))   # face A, two points: ground under box 1
    put(1, 1, 2, 101, 102, 3, ref.FACE_B, 1, ln=(1, 0), jn=(4, 99), jt=(1, 99))       # face B on a body turned by pi / 2; stale 2nd point
    put(2, 3, 4, 103, 104, 3, ref.CIRCLES, 1, jn=(1.5, 0))                           # circles at zero distance: (1, 0)
    put(3, 3, 5, 103, 105, 3, ref.CIRCLES, 1, jn=(2.5, 0), jt=(-0.5, 0))             # circles (0.6, 0.8) apart
    put(4, 6, 1, 106, 101, 3, ref.FACE_A, 0, ln=(0, 1), jn=(7, 7), jt=(7, 7))        # a sensor overlap: touching, no points
    put(5, 0, 2, 100, 102, 2, ref.FACE_A, 0)                                         # not touching
    return c, s


def test_hand_made_lists():
    c, s = hand_made()
    bodies = [1, 0, 3, 6, 2]
    offs, r = ref.lists(c, s, bodies, True)
    assert offs.tolist() == [0, 3, 4, 6, 7, 8]
    assert r["contact_index"].tolist() == [0, 1, 4, 0, 2, 3, 4, 1]
    assert r["other_body"].tolist() == [0, 2, 6, 1, 4, 5, 1, 1]
    assert r["fixture"].tolist() == [101, 101, 101, 100, 103, 103, 106, 102]
    assert r["other_fixture"].tolist() == [100, 102, 106, 101, 104, 105, 101, 101]
    # body 1 is body_b of contact 0 (+ normal) and body_a of contact 1 (- normal): on both sides of different contacts
    cos = np.cos(np.float64(F32(HALF_PI)))  # (-4.37e-8: the float32 angle is not pi / 2)
    want = [(0, 1), (cos, 1), (0, 0), (0, -1), (-1, 0), (-0.6, -0.8), (0, 0), (-cos, -1)]
    assert np.allclose(r["normal"], want, rtol=0, atol=1e-6)
    assert np.array_equal(r["normal"][[0, 2, 3, 4, 6]], np.array(want)[[0, 2, 3, 4, 6]])  # (exact where no rounding enters)
    assert r["normal_impulse"].tolist() == [5, 4, 0, 5, 1.5, 2.5, 0, 4]       # 2 + 3; one point: the stale 99 stays out; no points: 0
    assert r["tangent_impulse"].tolist() == [0.25, 1, 0, 0.25, 0, -0.5, 0, 1]
    assert r["point_count"].tolist() == [2, 1, 0, 2, 1, 1, 0, 1]
    assert not r["exempt"][[0, 1, 2, 3, 5, 6, 7]].any() and r["exempt"][4]  # (only the zero-distance circles)
    # every contact, touching or not
    offs, r = ref.lists(c, s, bodies, False)
    assert offs.tolist() == [0, 3, 5, 7, 8, 10]
    assert r["contact_index"].tolist() == [0, 1, 4, 0, 5, 2, 3, 4, 1, 5]
    assert r["normal"][4].tolist() == [0, 0] and r["normal_impulse"][4] == 0
    # the impulse on either side: jn n + jt (n.y, -n.x), equal and opposite
    offs, r = ref.lists(c, s, [0, 1], True)
    v = ref.impulse_vectors(r)
    assert v[0].tolist() == [-0.25, -5.0] and v[1].tolist() == [0.25, 5.0]
    # nothing asked for, and a body without contacts
    offs, r = ref.lists(c, s, [], True)
    assert offs.tolist() == [0] and len(r) == 0


def test_hand_made_totals():
    c, s = hand_made()
    t = ref.totals(c, s, [1, 0, 6, 5])
    assert t["contacts"].tolist() == [3, 2, 1, 1] and t["touching"].tolist() == [3, 1, 1, 1]
    assert t["points"].tolist() == [3, 2, 0, 1]
    assert t["max_normal_impulse"].tolist() == [5, 5, 0, 2.5]
    assert t["normal_impulse"].tolist() == [9, 5, 0, 2.5]
    # body 1: (0.25, 5) from the ground + 4 (0, 1) + 1 (1, 0) from body 2 + nothing from the sensor
    assert np.allclose(t["impulse"], [(1.25, 9), (-0.25, -5), (0, 0), (2.5 * 0.6 - 0.5 * 0.8, 2.5 * 0.8 + 0.5 * 0.6)], rtol=0, atol=1e-6)


def device_like(c, s, bodies, touching_only=True):
    """the reference's answer in the device's record types, normals rounded to float32"""
    offs, r = ref.lists(c, s, bodies, touching_only)
    d = np.zeros(len(r), b2hip.BODY_CONTACT_DTYPE)
    for name in ("contact_index", "other_body", "fixture", "other_fixture", "normal", "normal_impulse", "tangent_impulse"):
        d[name] = r[name]
    return offs, d, r


def device_like_totals(c, s, bodies):
    t = ref.totals(c, s, bodies)
    d = np.zeros(len(t), b2hip.BODY_CONTACT_TOTAL_DTYPE)
    for name in ("contacts", "touching", "impulse", "normal_impulse", "max_normal_impulse", "points"):
        d[name] = t[name]
    return d, t


def test_check_lists_rejects_corrupted_answers():
    c, s = hand_made()
    bodies = [1, 0, 3, 6, 2]
    offs, d, r = device_like(c, s, bodies)
    assert ref.check_lists(offs, d, offs, r) == 1  # (the zero-distance circles are exempt from the normal check)
    # a dropped record
    o2 = offs.copy()
    o2[1:] -= 1
    with pytest.raises(AssertionError):
        ref.check_lists(o2, np.delete(d, 2), offs, r)
    with pytest.raises(AssertionError):
        ref.check_lists(offs, np.delete(d, 2), offs, r)
    # a swapped order
    sw = d.copy()
    sw[[0, 1]] = sw[[1, 0]]
    with pytest.raises(AssertionError, match="contact_index"):
        ref.check_lists(offs, sw, offs, r)
    # a flipped normal
    fl = d.copy()
    fl["normal"][0] = -fl["normal"][0]
    with pytest.raises(AssertionError, match="normal"):
        ref.check_lists(offs, fl, offs, r)
    # ... and one just past the face bound of 8u, while half of it passes
    for scale, ok in ((4.0, True), (12.0, False)):
        nb = d.copy()
        nb["normal"][0][0] = F32(scale * ref.U)
        if ok:
            ref.check_lists(offs, nb, offs, r)
        else:
            with pytest.raises(AssertionError, match="normal"):
                ref.check_lists(offs, nb, offs, r)
    # an impulse off by one ulp
    for name in ("normal_impulse", "tangent_impulse"):
        up = d.copy()
        up[name][1] = np.nextafter(up[name][1], F32(np.inf))
        with pytest.raises(AssertionError, match=name):
            ref.check_lists(offs, up, offs, r)
    # the wrong side's fixture
    fx = d.copy()
    fx["fixture"][0], fx["other_fixture"][0] = fx["other_fixture"][0], fx["fixture"][0]
    with pytest.raises(AssertionError, match="fixture"):
        ref.check_lists(offs, fx, offs, r)


def test_check_totals_rejects_corrupted_answers():
    c, s = hand_made()
    bodies = [1, 0, 3, 6, 2, 5]
    offs, d, _ = device_like(c, s, bodies)
    t, rt = device_like_totals(c, s, bodies)
    ref.check_totals(t, offs, d, rt)
    for name, delta in (("contacts", 1), ("touching", 1), ("points", -1), ("pad", 1)):
        bad = t.copy()
        bad[name][0] += delta
        with pytest.raises(AssertionError):
            ref.check_totals(bad, offs, d, rt)
    bad = t.copy()
    bad["max_normal_impulse"][0] = np.nextafter(bad["max_normal_impulse"][0], F32(0))
    with pytest.raises(AssertionError, match="max_normal_impulse"):
        ref.check_totals(bad, offs, d, rt)
    # body 1: m = 3, sum(|jn| + |jt|) = 10.25, sum|jn| = 9: inside the bound passes, beyond it does not
    for name, inside, beyond in (("impulse", 7 * 2.0 ** -23 * 10.25, 7 * 2.0 ** -23 * 10.25),
                                 ("normal_impulse", 3 * 2.0 ** -23 * 9, 3 * 2.0 ** -23 * 9)):
        ok, bad = t.copy(), t.copy()
        if name == "impulse":
            ok[name][0][1] += F32(0.4 * inside)
            bad[name][0][1] += F32(2.0 * beyond)
        else:
            ok[name][0] += F32(0.4 * inside)
            bad[name][0] += F32(2.0 * beyond)
        ref.check_totals(ok, offs, d, rt)
        with pytest.raises(AssertionError, match=name):
            ref.check_totals(bad, offs, d, rt)


def test_float32_normals_stay_inside_the_bounds():
    """10^5 synthetic contacts, bodies up to 10^3 m from the origin, circle centres down to 10^-2 m apart: the normal op by op
    in float32 against float64."""
    rng = np.random.default_rng(11)
    n = 100000
    s = np.zeros(2 * n, b2hip.BODY_STATE_DTYPE)
    c = np.zeros(n, b2hip.CONTACT_DTYPE)
    c["body_a"], c["body_b"] = 2 * np.arange(n), 2 * np.arange(n) + 1
    c["manifold_type"] = rng.integers(0, 3, n)
    c["point_count"] = rng.integers(1, 3, n)
    pos = rng.uniform(-1e3, 1e3, (n, 2))
    circles = c["manifold_type"] == ref.CIRCLES
    # circles: half with the centres at the bodies' origins and 10^-2 .. 2 m apart (log-uniform), half with local points of
    # up to 0.5 m and the origins 1.5 .. 3 m apart; faces: anywhere near
    bare = rng.random(n) < 0.5
    gap = np.where(bare, 10.0 ** rng.uniform(-2.0, np.log10(2.0), n), rng.uniform(1.5, 3.0, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    s["px"][0::2], s["py"][0::2] = pos[:, 0], pos[:, 1]
    s["px"][1::2], s["py"][1::2] = pos[:, 0] + gap * np.cos(phi), pos[:, 1] + gap * np.sin(phi)
    s["angle"] = rng.uniform(-4 * np.pi, 4 * np.pi, 2 * n)
    local = np.where(bare[:, None], 0.0, rng.uniform(-0.35, 0.35, (n, 2)))
    c["local_point"] = np.where(circles[:, None], local, rng.uniform(-1, 1, (n, 2)))
    c["point_local"][:, 0] = np.where(circles[:, None], np.where(bare[:, None], 0.0, rng.uniform(-0.35, 0.35, (n, 2))), rng.uniform(-1, 1, (n, 2)))
    psi = rng.uniform(0, 2 * np.pi, n)
    c["local_normal"] = np.stack([np.cos(psi), np.sin(psi)], 1)  # (unit to float32 rounding, as b2CollidePolygons leaves it)
    n64, _, _, d = ref.normals(c, s)
    n32, _, _, _ = ref.normals(c, s, np.float32)
    assert n32.dtype == np.float32
    bound, exempt = ref.normal_bounds(c, s)
    assert not exempt.any()
    assert d[circles].min() >= 0.9e-2 and d[circles].min() < 2e-2 and np.abs(pos).max() > 990
    err = np.abs(n32.astype(np.float64) - n64).max(axis=1)
    worst = (err / bound).max()
    assert worst <= 1.0, "float32 normal at %.3g of its bound" % worst
    # (the bound is no blanket: face normals use a good part of theirs, and a wrong sign is thousands of bounds away)
    assert (err[~circles] / bound[~circles]).max() > 0.1
    assert (np.abs(-n32.astype(np.float64) - n64).max(axis=1) / bound)[~circles].min() > 100.0
