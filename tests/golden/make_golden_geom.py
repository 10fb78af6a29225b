"""Golden vectors for the one-shape geometry of the hot path's headers - b2Shape::RayCast, TestPoint, ComputeAABB, ComputeMass
and b2ShapeCast - generated from the REAL reference (oracle/_ref/libb2ref_harness.so) through the harness probes
(box2d-mt_amd/harness/harness.cpp: b2h_probe_shape_raycast, b2h_probe_test_point, b2h_probe_shape_aabb, b2h_probe_shape_mass,
b2h_probe_shape_cast). Run in the build container:

    python tests/golden/make_golden_geom.py

Output (committed, small): geom_vectors.npz - a table of shape records (circles with an off-centre m_p, edges with and without
ghost vertices, chain children, boxes, random 3 to 8 gons) and, per function, the inputs, the reference's outputs and a `kind`
tag per vector (see RAY_KINDS, POINT_KINDS, CAST_KINDS). check_coverage() states what the file must contain for the comparison
not to be vacuous; it reads the reference's outputs only, and tests/test_device_math_cpu.py runs it again on the committed file.
Fixtures are data (inputs and expected outputs); no reference source text is stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

CLASSES = ["circle", "edge", "edge_ghost", "chain", "box", "polygon"]
CIRCLE, EDGE, EDGE_GHOST, CHAIN, BOX, POLY = range(6)
RAY_KINDS = ["random", "inside", "short", "max_fraction", "zero_length", "parallel_box", "vertex_start", "face_start",
             "tangent_circle", "parallel_edge", "edge_outside"]
POINT_KINDS = ["random", "boundary", "near_boundary", "edge"]
CAST_KINDS = ["random", "overlap_start", "zero_translation"]
HALF_PI = np.float32(np.pi / 2)


def proxy_of(rec):
    """(verts[n,2], radius) of a shape record, as b2dProxy / b2DistanceProxy::Set take them"""
    t, cnt = int(rec.view(np.int32)[0]), int(rec.view(np.int32)[1])
    n = 1 if t == 0 else (2 if t in (1, 3) else cnt)
    return rec[6:6 + 2 * n].reshape(n, 2), float(rec[2])


def check_coverage(v):
    """The conditions the vectors must meet, from the reference's outputs alone. Raises AssertionError."""
    cls = v["shape_class"]
    rk, hit, rc = v["ray_kind"], v["ray_out"][:, 0] > 0, cls[v["ray_shape"]]
    for k, name in enumerate(RAY_KINDS):
        assert (rk == k).sum() >= 20, "ray kind %s: %d vectors" % (name, (rk == k).sum())
    for c, name in enumerate(CLASSES):
        m = (rk == 0) & (rc == c)
        assert m.sum() >= 50 and 0.25 <= hit[m].mean() <= 0.75, "random rays on %s: %d, hit rate %.2f" % (name, m.sum(), hit[m].mean())
    mf = v["ray_in"][rk == RAY_KINDS.index("max_fraction"), 4]
    assert ((mf > 0) & (mf < 1)).all() and (v["ray_in"][rk == 0, 4] == 1).all()
    assert (rc[rk == RAY_KINDS.index("max_fraction")] == BOX).sum() + (rc[rk == RAY_KINDS.index("max_fraction")] == POLY).sum() >= 40
    pk, inside, pc = v["pt_kind"], v["pt_out"] > 0, cls[v["pt_shape"]]
    for k, name in enumerate(POINT_KINDS):
        assert (pk == k).sum() >= 20, "point kind %s: %d vectors" % (name, (pk == k).sum())
    for c in (CIRCLE, BOX, POLY):  # (edges and chain children contain no point: kind "edge")
        m = (pk == 0) & (pc == c)
        assert m.sum() >= 50 and 0.25 <= inside[m].mean() <= 0.75, "random points on %s: %.2f inside" % (CLASSES[c], inside[m].mean())
    ck, chit = v["cast_kind"], v["cast_out"][:, 0] > 0
    for k, name in enumerate(CAST_KINDS):
        assert (ck == k).sum() >= 20, "cast kind %s: %d vectors" % (name, (ck == k).sum())
    for side in ("cast_shapeA", "cast_shapeB"):
        cc = cls[v[side]]
        for c, name in enumerate(CLASSES):
            m = (ck == 0) & (cc == c)
            assert m.sum() >= 50 and 0.25 <= chit[m].mean() <= 0.75, "random casts, %s %s: hit rate %.2f" % (side, name, chit[m].mean())
    for name, want in (("ray", 2000), ("pt", 1500), ("aabb", 1000), ("cast", 1000)):
        n = len(v[name + "_shape" if name != "cast" else "cast_shapeA"])
        assert 0.9 * want <= n <= 1.1 * want, "%s vectors: %d" % (name, n)
    for name in ("ray", "pt", "aabb", "cast"):  # a tenth of the transforms at exactly 0 or +-pi/2
        a = v[name + "_xf" if name != "cast" else "cast_xfB"][:, 2]
        assert (np.abs(a) <= 7).all()
        assert np.isin(a, [np.float32(0), HALF_PI, -HALF_PI]).mean() >= 0.08, name
    assert set(cls[v["aabb_shape"]].tolist()) == set(range(6))
    assert set(cls[v["mass_shape"]].tolist()) == {CIRCLE, EDGE, EDGE_GHOST}


def main():
    import b2harness as bh
    import probe_util as pu

    ref = bh.Harness(bh.REF_LIB)
    rng = np.random.default_rng(20250301)
    f32 = np.float32

    def rpoly():
        n = rng.integers(3, 9)
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        r = rng.uniform(0.3, 1.0)
        return [(r * np.cos(a) * rng.uniform(0.7, 1), r * np.sin(a) * rng.uniform(0.7, 1)) for a in ang]

    # ---- the shape table: descriptor for the reference's probe, record for the product's headers --------------------------
    descs, recs, classes = [], [], []

    def add(cls, kind, count=0, child=0, radius=0.0, floats=(), rec=None):
        d = np.zeros(20, f32)
        d[0], d[1], d[2], d[3] = kind, count, child, radius
        fl = np.asarray(floats, f32).reshape(-1)
        d[4:4 + fl.size] = fl
        descs.append(d); recs.append(rec(d)); classes.append(cls)

    def chain_rec(d):
        n, c = int(d[1]), int(d[2])
        p = d[4:4 + 2 * n].reshape(n, 2)
        before = p[c - 1] if c > 0 else (0, 0)
        after = p[c + 2] if c + 2 < n else (0, 0)
        flags = (1 if c > 0 else 0) | (2 if c + 2 < n else 0)
        return pu.shape_rec(3, flags, 0.01, (0, 0), [p[c], p[c + 1], before, after])

    for i in range(20):
        add(CIRCLE, 0, radius=rng.uniform(.2, .8), floats=rng.uniform(-.5, .5, 2), rec=lambda d: pu.circle_rec(d[4], d[5], d[3]))
    for i in range(24):
        flat = i >= 20  # four horizontal edges: a horizontal ray is EXACTLY parallel to them
        y1 = rng.uniform(-.3, .3)
        e = [-rng.uniform(.5, 1.5), y1, rng.uniform(.5, 1.5), y1 if flat else rng.uniform(-.3, .3), 0, 0, 0, 0, 0, 0]
        add(EDGE, 1, floats=e, rec=lambda d: pu.edge_rec(d[4:14]))
    for i in range(20):
        e = [-rng.uniform(.5, 1.5), rng.uniform(-.3, .3), rng.uniform(.5, 1.5), rng.uniform(-.3, .3),
             1, -2, rng.uniform(-1, 1), 1, 2, rng.uniform(-1, 1)]
        add(EDGE_GHOST, 1, floats=e, rec=lambda d: pu.edge_rec(d[4:14]))
    for i in range(20):
        n = int(rng.integers(3, 8))
        xs = np.sort(rng.uniform(-2, 2, n)) + 0.3 * np.arange(n)
        xs -= xs.mean()
        pts = np.stack([xs, rng.uniform(-.4, .4, n)], 1)
        add(CHAIN, 4, count=n, child=int(rng.integers(0, n - 1)), floats=pts, rec=chain_rec)
    for i in range(24):
        add(BOX, 3, count=4, floats=[rng.uniform(.2, 1), rng.uniform(.2, 1)], rec=lambda d: pu.box_rec(d[4], d[5]))
    for i in range(24):
        v = rpoly()
        add(POLY, 2, count=len(v), floats=v, rec=lambda d: pu.polygon_from_ref(ref, d[4:4 + 2 * int(d[1])].reshape(-1, 2)))
    recs = np.array(recs, f32)
    classes = np.array(classes, np.int8)
    by_class = [np.flatnonzero(classes == c) for c in range(6)]
    flat_edges = by_class[EDGE][-4:]

    def pick(cls):
        return int(rng.choice(by_class[cls]))

    def rangle():
        return f32(rng.choice([0.0, HALF_PI, -HALF_PI])) if rng.uniform() < 0.1 else f32(rng.uniform(-7, 7))

    def rxf():
        return np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rangle()], f32)

    IDENT = np.zeros(3, f32)

    def world(xf, local):
        c, s = np.cos(float(xf[2])), np.sin(float(xf[2]))
        x, y = local
        return np.array([c * x - s * y + xf[0], s * x + c * y + xf[1]])

    def segment(s):
        """local end points of the segment a ray can hit (edges, chain children)"""
        return recs[s, 6:8].astype(float), recs[s, 8:10].astype(float)

    def extent(s):
        """(centre, half extents) of a local box around the shape, for aiming"""
        c = classes[s]
        if c == CIRCLE:
            return recs[s, 6:8].astype(float), np.array([recs[s, 2], recs[s, 2]], float)
        if c in (EDGE, EDGE_GHOST, CHAIN):
            a, b = segment(s)
            return 0.5 * (a + b), np.array([0.5 * abs(b[0] - a[0]), 0.15])
        n = int(recs[s].view(np.int32)[1])
        p = recs[s, 6:6 + 2 * n].reshape(n, 2).astype(float)
        return 0.5 * (p.min(0) + p.max(0)), 0.5 * (p.max(0) - p.min(0))

    def interior(s):
        c = classes[s]
        if c == CIRCLE:
            return recs[s, 6:8].astype(float) + rng.uniform(-.4, .4, 2) * recs[s, 2]
        n = int(recs[s].view(np.int32)[1])
        p = recs[s, 6:6 + 2 * n].reshape(n, 2).astype(float)
        w = rng.uniform(0.2, 1, n)
        return (p * (w / w.sum())[:, None]).sum(0)

    # ---- rays -----------------------------------------------------------------------------------------------------------
    rays = []  # (shape, xf, ray5, kind)

    def aimed(s, spread, reach, max_fraction=1.0, kind=0, xf=None):
        xf = rxf() if xf is None else xf
        mid, half = extent(s)
        ang = rng.uniform(0, 2 * np.pi)
        p1 = mid + rng.uniform(1.8, 3.5) * np.array([np.cos(ang), np.sin(ang)])
        aim = mid + rng.uniform(-1, 1, 2) * half * spread
        p2 = p1 + rng.uniform(*reach) * (aim - p1)
        rays.append((s, xf, np.concatenate([world(xf, p1), world(xf, p2), [max_fraction]]).astype(f32), kind))

    SPREAD = {CIRCLE: 2.0, EDGE: 1.7, EDGE_GHOST: 1.7, CHAIN: 1.7, BOX: 2.4, POLY: 1.7}
    for c in range(6):
        for i in range(150):
            aimed(pick(c), SPREAD[c], (1.3, 2.2))
        for i in range(20):
            aimed(pick(c), SPREAD[c], (0.05, 0.45), kind=2)
        for i in range(60):
            aimed(pick(c), SPREAD[c], (1.5, 3.0), max_fraction=rng.uniform(0.02, 0.98), kind=3)
    for i in range(120):  # from inside a solid shape, outwards
        s = pick([CIRCLE, BOX, POLY][i % 3])
        xf = rxf()
        p1 = interior(s)
        ang = rng.uniform(0, 2 * np.pi)
        p2 = p1 + rng.uniform(2, 4) * np.array([np.cos(ang), np.sin(ang)])
        rays.append((s, xf, np.concatenate([world(xf, p1), world(xf, p2), [1.0]]).astype(f32), 1))
    for i in range(60):  # zero length, inside and outside
        s = pick(i % 6)
        xf = rxf()
        mid, half = extent(s)
        p = world(xf, mid + rng.uniform(-1.5, 1.5, 2) * half)
        rays.append((s, xf, np.concatenate([p, p, [1.0]]).astype(f32), 4))
    for i in range(120):  # axis-aligned rays at axis-aligned boxes: parallel to two faces, rate == 0 exactly
        s = pick(BOX)
        hx, hy = recs[s, 8], recs[s, 11]  # verts[1].x, verts[2].y
        axis, where = i % 2, (i // 2) % 3
        h_along, h_across = (hx, hy) if axis == 0 else (hy, hx)
        across = [f32(rng.uniform(-.9, .9) * h_across), f32(h_across * rng.uniform(1.05, 2) * rng.choice([-1, 1])),
                  f32(h_across) * f32(rng.choice([-1, 1]))][where]  # inside the slab, outside it, along the face's own line
        a0, a1 = -h_along - rng.uniform(.5, 2), h_along + rng.uniform(.5, 2)
        if (i // 6) % 2:
            a0, a1 = a1, a0
        if (i // 12) % 3 == 2:
            a1 = a0 + 0.5 * (a1 - a0) * rng.uniform(0, 1)  # (some stop inside or short of the box)
        p1, p2 = ((a0, across), (a1, across)) if axis == 0 else ((across, a0), (across, a1))
        rays.append((s, IDENT, np.array([p1[0], p1[1], p2[0], p2[1], 1.0], f32), 5))
    for i in range(80):  # p1 exactly on a vertex (identity transform: the world point IS the local vertex)
        s = pick([BOX, POLY][i % 2])
        n = int(recs[s].view(np.int32)[1])
        p1 = recs[s, 6:6 + 2 * n].reshape(n, 2)[rng.integers(0, n)]
        ang = rng.uniform(0, 2 * np.pi)
        p2 = p1 + rng.uniform(.5, 3) * np.array([np.cos(ang), np.sin(ang)])
        rays.append((s, IDENT, np.array([p1[0], p1[1], p2[0], p2[1], 1.0], f32), 6))
    for i in range(80):  # p1 exactly on a face of a box
        s = pick(BOX)
        hx, hy = recs[s, 8], recs[s, 11]
        face = i % 4
        t = f32(rng.uniform(-.9, .9))
        p1 = [(hx, t * hy), (t * hx, hy), (-hx, t * hy), (t * hx, -hy)][face]
        ang = rng.uniform(0, 2 * np.pi)
        p2 = np.array(p1, float) + rng.uniform(.5, 3) * np.array([np.cos(ang), np.sin(ang)])
        rays.append((s, IDENT, np.array([p1[0], p1[1], p2[0], p2[1], 1.0], f32), 7))
    for i in range(60):  # tangent to a circle: exactly (identity, horizontal / vertical) or to rounding (any transform)
        s = pick(CIRCLE)
        cx, cy, r = recs[s, 6], recs[s, 7], recs[s, 2]
        if i % 2 == 0:
            sign = f32(rng.choice([-1, 1]))
            if i % 4 == 0:
                y = cy + sign * r
                ray = [cx - 2, y, cx + 2, y, 1.0]
            else:
                x = cx + sign * r
                ray = [x, cy + 2, x, cy - 2, 1.0]
            rays.append((s, IDENT, np.array(ray, f32), 8))
        else:
            xf = rxf()
            ang = rng.uniform(0, 2 * np.pi)
            n = np.array([np.cos(ang), np.sin(ang)])
            t = np.array([-n[1], n[0]])
            touch = np.array([cx, cy], float) + float(r) * n
            rays.append((s, xf, np.concatenate([world(xf, touch - 2 * t), world(xf, touch + 2 * t), [1.0]]).astype(f32), 8))
    for i in range(60):  # parallel to an edge: exactly (horizontal edge, horizontal ray, identity) or to rounding
        if i % 2 == 0:
            s = int(flat_edges[(i // 2) % 4])
            a, b = segment(s)
            y = f32(a[1] + [0.0, 0.2, -0.2][(i // 8) % 3])
            rays.append((s, IDENT, np.array([a[0] - 1, y, b[0] + 1, y, 1.0], f32), 9))
        else:
            s = pick([EDGE, EDGE_GHOST, CHAIN][(i // 2) % 3])
            xf = rxf()
            a, b = segment(s)
            d = b - a
            off = rng.uniform(-.3, .3) * np.array([-d[1], d[0]])
            rays.append((s, xf, np.concatenate([world(xf, a - 0.3 * d + off), world(xf, b + 0.3 * d + off), [1.0]]).astype(f32), 9))
    for i in range(80):  # across the supporting line, beyond an end of the segment
        s = pick([EDGE, EDGE_GHOST, CHAIN][i % 3])
        xf = rxf()
        a, b = segment(s)
        d = b - a
        n = np.array([-d[1], d[0]]) / np.hypot(*d)
        u = rng.uniform(1.05, 2.0) if i % 2 else -rng.uniform(0.05, 1.0)
        cross = a + u * d
        lean = rng.uniform(-.5, .5) * d
        p1 = cross + rng.uniform(.3, 1.5) * n + lean
        p2 = cross - rng.uniform(.3, 1.5) * n - lean
        rays.append((s, xf, np.concatenate([world(xf, p1), world(xf, p2), [1.0]]).astype(f32), 10))
    ray_out = np.array([ref.shape_raycast(descs[s], xf, r) for s, xf, r, k in rays])

    # ---- points ---------------------------------------------------------------------------------------------------------
    pts = []  # (shape, xf, p, kind)
    for c, grow in ((CIRCLE, 1.3), (BOX, 1.3), (POLY, 1.15)):
        for i in range(400):
            s = pick(c)
            xf = rxf()
            mid, half = extent(s)
            pts.append((s, xf, world(xf, mid + rng.uniform(-1, 1, 2) * half * grow).astype(f32), 0))
    for i in range(240):  # exactly on the boundary (identity transform), or there to rounding (any position)
        s = pick(BOX if i % 8 else CIRCLE)
        if classes[s] == BOX:
            hx, hy = recs[s, 8], recs[s, 11]
            p = [(hx, hy), (-hx, hy), (-hx, -hy), (hx, -hy), (hx, 0), (0, hy), (-hx, 0), (0, -hy)][i % 8]
        else:
            p = (recs[s, 6] + recs[s, 2], recs[s, 7])
        if i % 3 == 2:
            xf = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 0], f32)
            pts.append((s, xf, (np.array(p, f32) + xf[:2]).astype(f32), 2))
        else:
            pts.append((s, IDENT, np.array(p, f32), 1))
    for i in range(60):
        s = pick([EDGE, EDGE_GHOST, CHAIN][i % 3])
        xf = rxf()
        a, b = segment(s)
        pts.append((s, xf, world(xf, a + rng.uniform(0, 1) * (b - a)).astype(f32), 3))
    pt_out = np.array([ref.test_point(descs[s], xf, p) for s, xf, p, k in pts], np.int8)

    # ---- AABBs ----------------------------------------------------------------------------------------------------------
    boxes = [(pick(i % 6), rxf()) for i in range(1000)]
    aabb_out = np.array([ref.shape_aabb(descs[s], xf) for s, xf in boxes])

    # ---- mass (circle, edge; polygons are in polygon_vectors.npz) --------------------------------------------------------
    masses = [(pick([CIRCLE, EDGE, EDGE_GHOST, CIRCLE][i % 4]), f32(rng.uniform(0.1, 20))) for i in range(128)]
    mass_out = np.array([ref.shape_mass(descs[s], d) for s, d in masses])

    # ---- shape casts ----------------------------------------------------------------------------------------------------
    casts = []  # (shapeA, shapeB, xfA, xfB, travel, kind)
    for i in range(1000):
        sa, sb = pick(i % 6), pick((i // 6) % 6)
        xa, xb = rxf(), rxf()
        kind = 0 if i < 800 else (1 if i < 900 else 2)
        ang = rng.uniform(0, 2 * np.pi)
        away = np.array([np.cos(ang), np.sin(ang)])
        if kind == 0 or (kind == 2 and i % 2):
            xb[:2] = xa[:2] + rng.uniform(2.0, 4.5) * away
            aim = xa[:2] + rng.uniform(-1.8, 1.8, 2)
            t = rng.uniform(0.5, 2.0) * (aim - xb[:2])
        else:
            xb[:2] = xa[:2] + rng.uniform(0, 0.3) * away
            t = rng.uniform(-2, 2, 2)
        if kind == 2:
            t = np.zeros(2)
        casts.append((sa, sb, xa, xb, t.astype(f32), kind))
    cast_out = []
    for sa, sb, xa, xb, t, k in casts:
        (va, ra), (vb, rb) = proxy_of(recs[sa]), proxy_of(recs[sb])
        cast_out.append(ref.shape_cast(va, ra, xa, vb, rb, xb, t))
    cast_out = np.array(cast_out)
    cast_out[cast_out[:, 0] == 0, 1:] = 0  # (a miss compares the flag only)
    # A cast whose loop never runs (the two skins touch at the start) reports a hit with 0 iterations, and the reference reads its
    # witness point from a simplex it never filled (b2Distance.cpp:730-740: uninitialised memory, another value every run):
    # such a vector keeps flag, normal, lambda and iterations, and its point is blanked (probe_util.cast_fields skips it).
    undefined = (cast_out[:, 0] > 0) & (cast_out[:, 6] == 0)
    cast_out[undefined, 1:3] = 0
    print("casts that hit without an iteration (point undefined in the reference):", int(undefined.sum()))

    out = dict(
        shapes=recs, shape_class=classes, classes=np.array(CLASSES),
        ray_kinds=np.array(RAY_KINDS), point_kinds=np.array(POINT_KINDS), cast_kinds=np.array(CAST_KINDS),
        ray_shape=np.array([r[0] for r in rays], np.int16), ray_xf=np.array([r[1] for r in rays], f32),
        ray_in=np.array([r[2] for r in rays], f32), ray_out=ray_out, ray_kind=np.array([r[3] for r in rays], np.int8),
        pt_shape=np.array([p[0] for p in pts], np.int16), pt_xf=np.array([p[1] for p in pts], f32),
        pt_in=np.array([p[2] for p in pts], f32), pt_out=pt_out, pt_kind=np.array([p[3] for p in pts], np.int8),
        aabb_shape=np.array([b[0] for b in boxes], np.int16), aabb_xf=np.array([b[1] for b in boxes], f32), aabb_out=aabb_out,
        mass_shape=np.array([m[0] for m in masses], np.int16), mass_density=np.array([m[1] for m in masses], f32), mass_out=mass_out,
        cast_shapeA=np.array([c[0] for c in casts], np.int16), cast_shapeB=np.array([c[1] for c in casts], np.int16),
        cast_xfA=np.array([c[2] for c in casts], f32), cast_xfB=np.array([c[3] for c in casts], f32),
        cast_t=np.array([c[4] for c in casts], f32), cast_out=cast_out, cast_kind=np.array([c[5] for c in casts], np.int8))
    rk, rc = out["ray_kind"], classes[out["ray_shape"]]
    for c, name in enumerate(CLASSES):
        m = (rk == 0) & (rc == c)
        print("random rays %-10s hit %.2f" % (name, (ray_out[m, 0] > 0).mean()),
              "| casts as A %.2f as B %.2f" % tuple((cast_out[(out["cast_kind"] == 0) & (classes[out[k]] == c), 0] > 0).mean()
                                                    for k in ("cast_shapeA", "cast_shapeB")))
    for k, name in enumerate(RAY_KINDS):
        print("ray kind %-14s %4d vectors, %4d hits" % (name, (rk == k).sum(), (ray_out[rk == k, 0] > 0).sum()))
    for c in (CIRCLE, BOX, POLY):
        m = (out["pt_kind"] == 0) & (classes[out["pt_shape"]] == c)
        print("random points %-8s inside %.2f" % (CLASSES[c], (pt_out[m] > 0).mean()))
    for k, name in enumerate(POINT_KINDS):
        print("point kind %-14s %4d vectors, %4d inside" % (name, (out["pt_kind"] == k).sum(), (pt_out[out["pt_kind"] == k] > 0).sum()))
    check_coverage(out)
    path = os.path.join(HERE, "geom_vectors.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("rays", len(rays), "points", len(pts), "aabbs", len(boxes), "casts", len(casts), "bytes", size)
    assert size < 300 * 1024


if __name__ == "__main__":
    main()
