"""Reference for the per-body contact lists and totals (include/b2hip.h: b2hip_body_contacts, b2hip_body_contact_totals),
computed from a b2hip.CONTACT_DTYPE array and a b2hip.BODY_STATE_DTYPE array alone - what World.contacts() and
World.body_states() return at the same point - and the checkers that compare a device answer against it.

Exact: the index sets and their order, other_body, the fixtures, the counts, points, max_normal_impulse, and the records'
impulses (imp0 + imp1 is one fp32 add). Bounded, with u = 2^-24:
  face manifolds      |normal - ref| <= 8u per component. The stored rotation is within 2u of the angle's sine / cosine
                      (error <= 2u (|x| + |y|) <= 2 sqrt(2) u on a unit vector), and rotating adds three roundings (two
                      products, one sum: <= (sqrt(2) + 1) u): 5.3u.
  circles manifolds   |normal - ref| <= 8u (1 + (|pA| + |pB|) / |d|): each world point carries a rounding of its magnitude
                      (the last sum of b2MulXV), u |pA| and u |pB|, into the difference d = pB - pA of length |d|; normalising
                      divides by |d| and adds a square root, a reciprocal and a product. The rotation's own error (2u and two
                      roundings on the LOCAL point) is below the points' while the local points are no longer than the world
                      points, as they are for shapes away from the origin. A record with |d| < 1e-5 is exempt (the (1, 0)
                      default switches at |d| = 2^-23); callers assert that their scenes hold none.
  totals              against float64 sums of the DEVICE'S OWN records of the same body, m = the touching count:
                      impulse within (m + 4) 2^-23 sum(|jn| + |jt|) per component, normal_impulse within m 2^-23 sum|jn|:
                      recursive summation in any order, three roundings per term, a factor 2 for second order.
"""
import numpy as np

U = 2.0 ** -24
EPSILON = 1.192092896e-07  # b2_epsilon
CIRCLES, FACE_A, FACE_B = 0, 1, 2
EXEMPT_BELOW = 1e-5

REF_DTYPE = np.dtype([("contact_index", "i4"), ("other_body", "i4"), ("fixture", "i4"), ("other_fixture", "i4"),
                      ("normal", "f8", 2), ("normal_impulse", "f4"), ("tangent_impulse", "f4"), ("point_count", "i4"),
                      ("bound", "f8"), ("exempt", "?")])
REF_TOTAL_DTYPE = np.dtype([("contacts", "i4"), ("touching", "i4"), ("impulse", "f8", 2), ("normal_impulse", "f8"),
                            ("max_normal_impulse", "f4"), ("points", "i4")])


def normals(contacts, states, ft=np.float64):
    """b2WorldManifold::Initialize's normal (pointing from body_a to body_b) of every contact, every operation in `ft`:
    float64 is the reference, float32 is op by op what the device computes. (0, 0) where point_count == 0.
    Returns (normal (N, 2), |pA|, |pB|, |d|): the last three are the circles manifolds' world points and their distance."""
    a, b = states[contacts["body_a"]], states[contacts["body_b"]]
    f = lambda x: np.asarray(x, np.float32).astype(ft)  # noqa: E731
    sa, ca, sb, cb = np.sin(f(a["angle"])), np.cos(f(a["angle"])), np.sin(f(b["angle"])), np.cos(f(b["angle"]))
    lnx, lny = f(contacts["local_normal"][:, 0]), f(contacts["local_normal"][:, 1])
    lpx, lpy = f(contacts["local_point"][:, 0]), f(contacts["local_point"][:, 1])
    qx, qy = f(contacts["point_local"][:, 0, 0]), f(contacts["point_local"][:, 0, 1])
    fax, fay = ca * lnx - sa * lny, sa * lnx + ca * lny
    fbx, fby = -(cb * lnx - sb * lny), -(sb * lnx + cb * lny)
    pax, pay = (ca * lpx - sa * lpy) + f(a["px"]), (sa * lpx + ca * lpy) + f(a["py"])
    pbx, pby = (cb * qx - sb * qy) + f(b["px"]), (sb * qx + cb * qy) + f(b["py"])
    dx, dy = pbx - pax, pby - pay
    d2 = dx * dx + dy * dy
    far = d2 > ft(EPSILON) * ft(EPSILON)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = ft(1.0) / np.sqrt(d2)
        cx, cy = np.where(far, dx * inv, ft(1.0)), np.where(far, dy * inv, ft(0.0))
    kind = contacts["manifold_type"]
    nx = np.where(kind == CIRCLES, cx, np.where(kind == FACE_A, fax, fbx))
    ny = np.where(kind == CIRCLES, cy, np.where(kind == FACE_A, fay, fby))
    none = contacts["point_count"] <= 0
    n = np.stack([np.where(none, ft(0.0), nx), np.where(none, ft(0.0), ny)], axis=1)
    return n, np.hypot(pax, pay), np.hypot(pbx, pby), np.sqrt(d2)


def normal_bounds(contacts, states):
    """(bound per component, exempt) of every contact's normal, from the float64 evaluation (module docstring)"""
    _, pa, pb, d = normals(contacts, states)
    circles = (contacts["manifold_type"] == CIRCLES) & (contacts["point_count"] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(circles, 8.0 * U * (1.0 + (pa + pb) / d), 8.0 * U)
    return bound, circles & (d < EXEMPT_BELOW)


def _records(contacts, states):
    """every contact as body_b sees it (REF_DTYPE); body_a's view swaps the ids and negates the normal"""
    r = np.zeros(len(contacts), REF_DTYPE)
    n, _, _, _ = normals(contacts, states)
    r["bound"], r["exempt"] = normal_bounds(contacts, states)
    pc = contacts["point_count"]
    jn, jt = contacts["normal_impulse"], contacts["tangent_impulse"]
    zero = np.float32(0.0)
    r["contact_index"] = np.arange(len(contacts))
    r["other_body"], r["fixture"], r["other_fixture"] = contacts["body_a"], contacts["fixture_b"], contacts["fixture_a"]
    r["normal"] = n
    r["normal_impulse"] = np.where(pc > 1, jn[:, 0] + jn[:, 1], np.where(pc == 1, jn[:, 0], zero))  # (float32 + float32)
    r["tangent_impulse"] = np.where(pc > 1, jt[:, 0] + jt[:, 1], np.where(pc == 1, jt[:, 0], zero))
    r["point_count"] = pc
    return r


def lists(contacts, states, bodies, touching_only):
    """(offsets (n + 1), records REF_DTYPE): body i's records are records[offsets[i]:offsets[i + 1]], ascending contact_index"""
    as_b = _records(contacts, states)
    listed = (contacts["flags"] & 1) != 0 if touching_only else np.ones(len(contacts), bool)
    parts, offsets = [], [0]
    for body in np.asarray(bodies).tolist():
        idx = np.flatnonzero(((contacts["body_a"] == body) | (contacts["body_b"] == body)) & listed)
        part = as_b[idx].copy()
        mine_a = contacts["body_a"][idx] == body
        part["other_body"][mine_a] = contacts["body_b"][idx][mine_a]
        part["fixture"][mine_a] = contacts["fixture_a"][idx][mine_a]
        part["other_fixture"][mine_a] = contacts["fixture_b"][idx][mine_a]
        part["normal"][mine_a] = -part["normal"][mine_a]
        parts.append(part)
        offsets.append(offsets[-1] + len(idx))
    return np.asarray(offsets, np.int32), (np.concatenate(parts) if parts else np.zeros(0, REF_DTYPE))


def impulse_vectors(records):
    """the impulse each record puts on its body, float64: jn n + jt (n.y, -n.x)"""
    n = np.asarray(records["normal"], np.float64)
    jn, jt = records["normal_impulse"].astype(np.float64), records["tangent_impulse"].astype(np.float64)
    return np.stack([jn * n[:, 0] + jt * n[:, 1], jn * n[:, 1] - jt * n[:, 0]], axis=1)


def totals(contacts, states, bodies):
    """REF_TOTAL_DTYPE per body: counts, and over the touching records the float64 sums, the largest normal impulse, the points"""
    offs_all, _ = lists(contacts, states, bodies, False)
    offs, recs = lists(contacts, states, bodies, True)
    vec = impulse_vectors(recs)
    out = np.zeros(len(offs) - 1, REF_TOTAL_DTYPE)
    for i in range(len(out)):
        part = slice(offs[i], offs[i + 1])
        out[i]["contacts"] = offs_all[i + 1] - offs_all[i]
        out[i]["touching"] = offs[i + 1] - offs[i]
        out[i]["impulse"] = vec[part].sum(axis=0)
        out[i]["normal_impulse"] = recs["normal_impulse"][part].astype(np.float64).sum()
        out[i]["max_normal_impulse"] = recs["normal_impulse"][part].max() if offs[i + 1] > offs[i] else 0.0
        out[i]["points"] = recs["point_count"][part].sum()
    return out


def check_lists(offsets, records, ref_offsets, ref_records):
    """a device answer (offsets, BODY_CONTACT_DTYPE records) against lists(); returns how many normals were exempt"""
    assert np.array_equal(np.asarray(offsets), ref_offsets), "offsets differ: the lists' lengths"
    assert len(records) == len(ref_records), "%d records for %d" % (len(records), len(ref_records))
    for name in ("contact_index", "other_body", "fixture", "other_fixture"):
        bad = np.flatnonzero(records[name] != ref_records[name])
        assert bad.size == 0, "%s differs first at record %d: %d, expected %d" % (name, bad[0], records[name][bad[0]],
                                                                                 ref_records[name][bad[0]])
    for name in ("normal_impulse", "tangent_impulse"):  # one fp32 add: the same bits (+0.0 and -0.0 are one value)
        bad = np.flatnonzero(records[name] != ref_records[name])
        assert bad.size == 0, "%s differs first at record %d: %r, expected %r" % (name, bad[0], records[name][bad[0]],
                                                                                 ref_records[name][bad[0]])
    err = np.abs(records["normal"].astype(np.float64) - ref_records["normal"]).max(axis=1) if len(records) else np.zeros(0)
    bad = np.flatnonzero(~ref_records["exempt"] & ~(err <= ref_records["bound"]))
    assert bad.size == 0, "normal of record %d off by %.3g, bound %.3g" % (bad[0], err[bad[0]], ref_records["bound"][bad[0]])
    return int(ref_records["exempt"].sum())


def check_totals(device_totals, offsets, records, ref_totals):
    """device totals against totals() (the exact fields) and against float64 sums of the device's own TOUCHING records
    (offsets, records: the answer of b2hip_body_contacts with touching_only = 1 for the same bodies, checked by check_lists)"""
    t = device_totals
    assert len(t) == len(ref_totals) == len(offsets) - 1
    for name in ("contacts", "touching", "points", "max_normal_impulse"):
        bad = np.flatnonzero(t[name] != ref_totals[name])
        assert bad.size == 0, "%s of body %d: %r, expected %r" % (name, bad[0], t[name][bad[0]], ref_totals[name][bad[0]])
    assert not t["pad"].any(), "pad is not zero"
    vec = impulse_vectors(records)
    jn, jt = np.abs(records["normal_impulse"].astype(np.float64)), np.abs(records["tangent_impulse"].astype(np.float64))
    for i in range(len(t)):
        part = slice(offsets[i], offsets[i + 1])
        m = int(offsets[i + 1] - offsets[i])
        bound_v = (m + 4) * 2.0 ** -23 * (jn[part] + jt[part]).sum()
        bound_n = m * 2.0 ** -23 * jn[part].sum()
        err_v = np.abs(t["impulse"][i].astype(np.float64) - vec[part].sum(axis=0)).max()
        err_n = abs(float(t["normal_impulse"][i]) - records["normal_impulse"][part].astype(np.float64).sum())
        assert err_v <= bound_v, "impulse of body %d off by %.3g, bound %.3g (m = %d)" % (i, err_v, bound_v, m)
        assert err_n <= bound_n, "normal_impulse of body %d off by %.3g, bound %.3g (m = %d)" % (i, err_n, bound_n, m)
