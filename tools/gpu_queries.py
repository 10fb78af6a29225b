"""Batched device queries (include/b2hip.h: b2hip_query_aabbs / b2hip_query_points / b2hip_ray_cast_closest / b2hip_ray_cast_all /
b2hip_ray_cast_any) on the two BASELINE worlds bench.py settles, against the drop-in's host path on the same world.

  python tools/gpu_queries.py queries [--out FILE]    call times of 10^5 rays (1-20 m), 10^5 boxes (half extents 0.25-3 m)
                                                      and 10^5 points on the settled config 5 field (10^6 bodies) and the
                                                      settled config 3 Tumbler; the fixed cost of a call (edits, the grid
                                                      rebuild, one query) apart; the drop-in: the first b2World::QueryAABB
                                                      after a step (its shadow-tree sync) and 1 000 rays / boxes through
                                                      b2World::RayCast / QueryAABB, per query. The all-hit and any-hit
                                                      calls take the same rays as the closest call, in the same run: their
                                                      times against it, beside the spread of its repeated runs (the noise),
                                                      and the drop-in's RayCast with an all-hits callback on 1 000 of them
  python tools/gpu_queries.py steps --harness LIB     ms per b2hip_step of both settled worlds (one JSON line), for an
                                                      A/B of two builds in separate processes
  python tools/gpu_queries.py kernels DIR             the k_query_* kernel times of a separate
                                                      `rocprofv3 --kernel-trace --stats -d DIR -- ... queries --quick` run
tools/gpu_queries.sh runs the whole sequence, every GPU step under its own time limit.
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

import b2harness as bh  # noqa: E402
import b2hip  # noqa: E402

CCD = bh.F_CONTINUOUS | bh.F_SLEEP | bh.F_WARM
# (name, scene, p0, p1, flags, seed, settle steps) as bench.py builds and settles them (bench.py: SETTLE, the config jobs)
WORLDS = [("config5_field_1M", bh.FIELD, 1000000, 10000, CCD, 3, 30),
          ("config3_tumbler316", bh.TUMBLER, 316, 0, bh.F_SLEEP | bh.F_WARM, 1, 700)]


def settled(h, spec):
    name, scene, p0, p1, flags, seed, settle = spec
    w = h.world(scene, p0, p1, seed=seed, flags=flags)
    w.step(settle)
    return w


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1000.0 * (time.perf_counter() - t0))
    return float(np.median(ts)), ts


def run_queries(args):
    h = bh.Harness(bh.AMD_LIB)
    out = {"worlds": []}
    n = args.n
    for spec in WORLDS:
        w = settled(h, spec)
        dw = b2hip.World.borrow(w.device_world())
        b = w.bodies()
        pos = b[b[:, 7] >= 0][:, :2]
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        rng = np.random.default_rng(1)
        p1 = rng.uniform(lo, hi, (n, 2)).astype(np.float32)
        ang, ln = rng.uniform(0, 2 * np.pi, n), rng.uniform(1.0, 20.0, n)
        p2 = (p1 + np.stack([np.cos(ang) * ln, np.sin(ang) * ln], 1)).astype(np.float32)
        c = rng.uniform(lo, hi, (n, 2)).astype(np.float32)
        e = rng.uniform(0.25, 3.0, (n, 2)).astype(np.float32)
        pts = rng.uniform(lo, hi, (n, 2)).astype(np.float32)
        rec = {"world": spec[0], "bodies": w.body_count, "batch": n}
        one = np.zeros((1, 2), np.float32)
        rec["fixed_call_ms"], _ = timed(lambda: dw.ray_cast_closest(one, one + 1.0), args.reps)  # edits + grid rebuild + 1 ray
        rec["rays_call_ms"], _ = timed(lambda: dw.ray_cast_closest(p1, p2), args.reps)
        rec["aabbs_call_ms"], _ = timed(lambda: dw.query_aabbs(c - e, c + e), args.reps)
        rec["points_call_ms"], _ = timed(lambda: dw.query_points(pts), args.reps)
        hits = dw.ray_cast_closest(p1, p2)
        rec["ray_hits"] = int((hits["fixture"] >= 0).sum())
        # all hits / any hit on the closest call's rays; the closest call once more around them, its runs' spread = the noise
        rec["rays_all_call_ms"], _ = timed(lambda: dw.ray_cast_all(p1, p2), args.reps)
        rec["rays_any_call_ms"], _ = timed(lambda: dw.ray_cast_any(p1, p2), args.reps)
        again, ts = timed(lambda: dw.ray_cast_closest(p1, p2), args.reps)
        rec["rays_call_again_ms"] = again
        rec["rays_call_spread_ms"] = max(ts) - min(ts)
        rec["rays_all_over_closest"] = rec["rays_all_call_ms"] / again
        rec["rays_any_over_closest"] = rec["rays_any_call_ms"] / again
        rec["ray_all_records"] = int(dw.ray_cast_all(p1, p2)[0][-1])
        rec["ray_any_true"] = int(dw.ray_cast_any(p1, p2).sum())
        offs, _ = dw.query_aabbs(c - e, c + e)
        rec["aabb_items"] = int(offs[-1])
        if not args.quick:
            # the drop-in's host path on the same world: the first query after a step pays the shadow-tree sync
            w.step(1)
            t0 = time.perf_counter()
            w.query_aabb(c[0] - e[0], c[0] + e[0])
            rec["dropin_first_query_after_step_ms"] = 1000.0 * (time.perf_counter() - t0)
            k = 1000
            t0 = time.perf_counter()
            for i in range(k):
                w.raycast_closest(p1[i], p2[i])
            rec["dropin_ray_us"] = 1e6 * (time.perf_counter() - t0) / k
            every = w.L.b2h_raycast_all_filtered  # (b2World::RayCast, a callback that returns 1: every fixture crossed)
            every.argtypes = [C.c_void_p] + [C.c_float] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p]
            rows = np.zeros((4096, 7), np.float32)
            sample = np.concatenate([p1[:k], p2[:k]], axis=1).astype(np.float64).tolist()
            t0 = time.perf_counter()
            for x1, y1, x2, y2 in sample:
                every(w.ptr, x1, y1, x2, y2, 0xFFFF, 1, len(rows), rows.ctypes.data_as(C.c_void_p))
            rec["dropin_ray_all_us"] = 1e6 * (time.perf_counter() - t0) / k
            t0 = time.perf_counter()
            for i in range(k):
                w.query_aabb(c[i] - e[i], c[i] + e[i])
            rec["dropin_aabb_us"] = 1e6 * (time.perf_counter() - t0) / k
            # per query, the drop-in path = its sync once (spread over the batch) + its per-query time
            for kind, key in (("ray", "rays_call_ms"), ("ray_all", "rays_all_call_ms"), ("aabb", "aabbs_call_ms")):
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


def run_steps(args):
    h = bh.Harness(args.harness)
    rec = {"harness": args.label}
    for spec in WORLDS:
        w = settled(h, spec)
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            w.step(1)
            ms.append(1000.0 * (time.perf_counter() - t0))
        rec[spec[0] + "_step_ms_median"] = float(np.median(ms))
        w.close()
    print(json.dumps(rec), flush=True)


def run_kernels(args):
    """the k_query_* dispatches of a rocprofv3 run of `queries --quick` (rocpd database, `kernels` view), split into the two
    worlds at the longest gap between them (the second world is built and settled in between)"""
    import collections
    import glob
    import sqlite3
    db = sorted(glob.glob(os.path.join(args.dir, "*.db")))[0]
    rows = list(sqlite3.connect(db).execute(
        "select name, start, end, duration from kernels where name like '%k_query%' order by start"))
    cut = max(range(len(rows) - 1), key=lambda i: rows[i + 1][1] - rows[i][2])
    for (name, _, _, _, _, _, _), seg in zip(WORLDS, (rows[:cut + 1], rows[cut + 1:])):
        print(name)
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
    s = sub.add_parser("steps")
    s.add_argument("--harness", default=bh.AMD_LIB)
    s.add_argument("--label", default="this tree")
    s.add_argument("--steps", type=int, default=100)
    k = sub.add_parser("kernels")
    k.add_argument("dir", help="the -d directory of the rocprofv3 run")
    args = ap.parse_args()
    if args.mode == "kernels":
        return run_kernels(args)
    b2hip.use_torch_hip_runtime()
    run_queries(args) if args.mode == "queries" else run_steps(args)


if __name__ == "__main__":
    main()
