"""Batched distance queries on the device (include/b2hip.h: b2hip_shape_distance_closest / b2hip_query_shapes_within) on the
settled config 5 field bench.py measures (the world and the settling of tools/gpu_queries.py), against their composition from
the drop-in.

  python tools/gpu_distance_queries.py queries [--out FILE]   call times of 10^5 closest and 10^5 within queries (circles of
                                                              0.5-3 m and boxes of half extents 0.25-1.5 m, random angles)
                                                              at max_distance 2 m and 50 m; the drop-in composition per
                                                              query: b2World::QueryAABB then b2Distance per proxy
                                                              (harness.cpp: b2h_shape_distance_all) over 200 of them, plus
                                                              the first QueryAABB after a step (its shadow-tree sync) spread
                                                              over the batch
  python tools/gpu_distance_queries.py kernels DIR            the k_query_* kernel times of a separate
                                                              `rocprofv3 --kernel-trace --stats -d DIR -- ... queries --quick`
A range whose batch would take longer than --budget-ms per call (estimated from 1 000 queries) runs a smaller batch, and says so.
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
from gpu_shape_queries import probe_batch  # noqa: E402

RANGES = (2.0, 50.0)
SAMPLE = 200


def run_queries(args):
    h = bh.Harness(bh.AMD_LIB)
    spec = WORLDS[0]
    w = settled(h, spec)
    L = w.L
    L.b2h_shape_distance_all.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    L.b2h_shape_distance_all.restype = C.c_int
    dw = b2hip.World.borrow(w.device_world())
    b = w.bodies()
    pos = b[b[:, 7] >= 0][:, :2]
    rng = np.random.default_rng(1)
    shapes, poses, idx, _ = probe_batch(args.n, pos.min(axis=0), pos.max(axis=0), rng)
    out = {"world": spec[0], "bodies": w.body_count, "ranges": []}
    out["fixed_call_ms"], _ = timed(lambda: dw.shape_distance_closest(shapes[0], poses[:1], 2.0), args.reps)  # edits + grid + 1 query
    for d in RANGES:
        n = args.n
        probe = min(n, 1000)
        t0 = time.perf_counter()
        dw.query_shapes_within(shapes, poses[:probe], d, shape_index=idx[:probe])
        est = 1000.0 * (time.perf_counter() - t0) * n / probe
        if est > args.budget_ms:
            n = max(probe, int(n * args.budget_ms / est))
        p, k = poses[:n], idx[:n]
        rec = {"max_distance": d, "batch": n}
        rec["closest_call_ms"], _ = timed(lambda: dw.shape_distance_closest(shapes, p, d, shape_index=k), args.reps)
        rec["within_call_ms"], _ = timed(lambda: dw.query_shapes_within(shapes, p, d, shape_index=k), args.reps)
        best = dw.shape_distance_closest(shapes, p, d, shape_index=k)
        offs, hits = dw.query_shapes_within(shapes, p, d, shape_index=k)
        rec["closest_hits"] = int((best["fixture"] >= 0).sum())
        rec["within_records"] = int(offs[-1])
        first = offs[:-1][offs[1:] > offs[:-1]]
        assert rec["closest_hits"] == len(first), "the two calls disagree on which queries find something"
        out["ranges"].append(rec)
        print(json.dumps(rec), flush=True)
    if not args.quick:
        w.step(1)
        t0 = time.perf_counter()
        w.query_aabb(pos[0] - 1.0, pos[0] + 1.0)
        out["dropin_first_query_after_step_ms"] = 1000.0 * (time.perf_counter() - t0)
        ids = np.zeros((1 << 16, 3), np.int32)
        vals = np.zeros((1 << 16, 5), np.float32)
        for rec in out["ranges"]:
            t0 = time.perf_counter()
            for i in range(SAMPLE):
                L.b2h_shape_distance_all(w.ptr, C.byref(shapes[idx[i]]), float(poses[i, 0]), float(poses[i, 1]), float(poses[i, 2]),
                                         rec["max_distance"], len(ids), ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p))
            rec["dropin_us"] = 1e6 * (time.perf_counter() - t0) / SAMPLE
            host_us = rec["dropin_us"] + 1000.0 * out["dropin_first_query_after_step_ms"] / rec["batch"]
            for kind in ("closest", "within"):
                rec["%s_speedup_per_query" % kind] = host_us / (1000.0 * rec["%s_call_ms" % kind] / rec["batch"])
            print(json.dumps(rec), flush=True)
    dw.close()
    w.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def run_kernels(args):
    """every k_query_* dispatch of a rocprofv3 run of `queries --quick`, per kernel in launch order: the one-query calls
    first, then for 2 m and again for 50 m the 1 000-query probe (within only), `reps` closest calls, `reps` within calls and
    one more of each"""
    import collections
    import glob
    import sqlite3
    db = sorted(glob.glob(os.path.join(args.dir, "**", "*.db"), recursive=True))[0]
    rows = list(sqlite3.connect(db).execute(
        "select name, start, end, duration from kernels where name like '%k_query%' order by start"))
    d = collections.defaultdict(list)
    for r in rows:
        d[r[0].split("(")[0].replace("void ", "")].append(r[3] / 1000.0)
    for k, v in d.items():
        print("  %-26s launches %3d  in order (us): %s" % (k, len(v), " ".join("%.1f" % x for x in v)))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    q = sub.add_parser("queries")
    q.add_argument("--n", type=int, default=100000)
    q.add_argument("--reps", type=int, default=5)
    q.add_argument("--budget-ms", type=float, default=4000.0, help="the longest a batch call may take before the batch shrinks")
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
