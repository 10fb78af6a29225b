"""Batched shape queries on the device (include/b2hip.h: b2hip_query_shapes / b2hip_shape_cast_closest) on the two BASELINE
worlds bench.py settles (the worlds and the settling of tools/gpu_queries.py), against their composition from the drop-in.

  python tools/gpu_shape_queries.py queries [--out FILE]   call times of 10^5 overlap queries (circles of 0.5-3 m and boxes of
                                                           half extents 0.25-1.5 m, random angles) and 10^5 casts (1-20 m) on
                                                           the settled config 5 field (10^6 bodies) and the settled config 3
                                                           Tumbler; the drop-in composition per query: b2World::QueryAABB
                                                           then b2TestOverlap / b2ShapeCast per proxy (harness.cpp:
                                                           b2h_query_shape, b2h_shape_cast_all) over 1 000 of them, plus the
                                                           first QueryAABB after a step (its shadow-tree sync) spread over
                                                           the batch
  python tools/gpu_shape_queries.py kernels DIR            the k_query_* kernel times of a separate
                                                           `rocprofv3 --kernel-trace --stats -d DIR -- ... queries --quick`
b2hip_step A/B against another build: tools/gpu_queries.py steps. tools/gpu_shape_queries.sh runs the whole sequence.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "box2d-mt_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import b2harness as bh  # noqa: E402
import b2hip  # noqa: E402
from gpu_queries import WORLDS, settled, timed  # noqa: E402


def probe_batch(n, lo, hi, rng):
    """n poses over the world's extent, a table of 64 circles (0.5-3 m) and 64 boxes, one picked per pose"""
    shapes = [b2hip.circle_shape(float(r)) for r in rng.uniform(0.5, 3.0, 64)]
    shapes += [b2hip.box_shape(float(a), float(b)) for a, b in rng.uniform(0.25, 1.5, (64, 2))]
    xy = rng.uniform(lo, hi, (n, 2))
    poses = np.concatenate([xy, rng.uniform(0.0, 2.0 * np.pi, (n, 1))], 1).astype(np.float32)
    idx = rng.integers(0, len(shapes), n).astype(np.int32)
    ang, ln = rng.uniform(0, 2 * np.pi, n), rng.uniform(1.0, 20.0, n)
    t = np.stack([np.cos(ang) * ln, np.sin(ang) * ln], 1).astype(np.float32)
    return shapes, poses, idx, t


def run_queries(args):
    h = bh.Harness(bh.AMD_LIB)
    out = {"worlds": []}
    n = args.n
    for spec in WORLDS:
        w = settled(h, spec)
        L = w.L
        L.b2h_query_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p]
        L.b2h_query_shape.restype = C.c_int
        L.b2h_shape_cast_all.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
        L.b2h_shape_cast_all.restype = C.c_int
        dw = b2hip.World.borrow(w.device_world())
        b = w.bodies()
        pos = b[b[:, 7] >= 0][:, :2]
        rng = np.random.default_rng(1)
        shapes, poses, idx, t = probe_batch(n, pos.min(axis=0), pos.max(axis=0), rng)
        rec = {"world": spec[0], "bodies": w.body_count, "batch": n}
        one = poses[:1]
        rec["fixed_call_ms"], _ = timed(lambda: dw.query_shapes(shapes[0], one), args.reps)  # edits + grid rebuild + 1 query
        rec["overlaps_call_ms"], _ = timed(lambda: dw.query_shapes(shapes, poses, shape_index=idx), args.reps)
        rec["casts_call_ms"], _ = timed(lambda: dw.shape_cast_closest(shapes, poses, t, shape_index=idx), args.reps)
        offs, _ = dw.query_shapes(shapes, poses, shape_index=idx)
        rec["overlap_items"] = int(offs[-1])
        hits = dw.shape_cast_closest(shapes, poses, t, shape_index=idx)
        rec["cast_hits"] = int((hits["fixture"] >= 0).sum())
        if not args.quick:
            w.step(1)
            t0 = time.perf_counter()
            w.query_aabb(pos[0] - 1.0, pos[0] + 1.0)
            rec["dropin_first_query_after_step_ms"] = 1000.0 * (time.perf_counter() - t0)
            k = 1000
            buf = np.zeros(1 << 16, np.int32)
            ids = np.zeros((4096, 2), np.int32)
            vals = np.zeros((4096, 5), np.float32)
            t0 = time.perf_counter()
            for i in range(k):
                L.b2h_query_shape(w.ptr, C.byref(shapes[idx[i]]), float(poses[i, 0]), float(poses[i, 1]), float(poses[i, 2]),
                                  len(buf), buf.ctypes.data_as(C.c_void_p))
            rec["dropin_overlap_us"] = 1e6 * (time.perf_counter() - t0) / k
            t0 = time.perf_counter()
            for i in range(k):
                # (every hit, not just the closest: the composition a user writes from QueryAABB + b2ShapeCast)
                L.b2h_shape_cast_all(w.ptr, C.byref(shapes[idx[i]]), float(poses[i, 0]), float(poses[i, 1]), float(poses[i, 2]),
                                     float(t[i, 0]), float(t[i, 1]), len(ids), ids.ctypes.data_as(C.c_void_p),
                                     vals.ctypes.data_as(C.c_void_p))
            rec["dropin_cast_us"] = 1e6 * (time.perf_counter() - t0) / k
            for kind, key in (("overlap", "overlaps_call_ms"), ("cast", "casts_call_ms")):
                dev_us = 1000.0 * rec[key] / n
                host_us = rec["dropin_%s_us" % kind] + 1000.0 * rec["dropin_first_query_after_step_ms"] / n
                rec["%s_speedup_per_query" % kind] = host_us / dev_us
        out["worlds"].append(rec)
        print(json.dumps(rec), flush=True)
        dw.close()
        w.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def run_kernels(args):
    """the k_query_* dispatches of a rocprofv3 run of `queries --quick`, split into the two worlds at the longest gap"""
    import collections
    import glob
    import sqlite3
    db = sorted(glob.glob(os.path.join(args.dir, "**", "*.db"), recursive=True))[0]
    rows = list(sqlite3.connect(db).execute(
        "select name, start, end, duration from kernels where name like '%k_query%' order by start"))
    cut = max(range(len(rows) - 1), key=lambda i: rows[i + 1][1] - rows[i][2])
    for spec, seg in zip(WORLDS, (rows[:cut + 1], rows[cut + 1:])):
        print(spec[0])
        d = collections.defaultdict(list)
        for r in seg:
            d[r[0].split("(")[0].replace("void ", "")].append(r[3] / 1000.0)
        for k, v in d.items():
            v = sorted(v)
            print("  %-22s launches %3d  median %9.1f us  max %9.1f us" % (k, len(v), v[len(v) // 2], v[-1]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    q = sub.add_parser("queries")
    q.add_argument("--n", type=int, default=100000)
    q.add_argument("--reps", type=int, default=5)
    q.add_argument("--out", default="")
    q.add_argument("--quick", action="store_true", help="device calls only (the rocprofv3 run)")
    k = sub.add_parser("kernels")
    k.add_argument("dir", help="the -d directory of the rocprofv3 run")
    args = ap.parse_args()
    if args.mode == "kernels":
        return run_kernels(args)
    b2hip.use_torch_hip_runtime()
    run_queries(args)


if __name__ == "__main__":
    main()
