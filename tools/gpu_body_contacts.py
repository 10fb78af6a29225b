"""Per-body contact lists and totals on the device (include/b2hip.h: b2hip_body_contacts, b2hip_body_contact_totals) on the
settled 100 000-box Tumbler bench.py measures, against the route a caller had before: b2hip_get_contacts (every contact of the
world to the host) plus a numpy grouping by body, in the same run.

  python tools/gpu_body_contacts.py [--out FILE] [--reps N]

Four batches: 10^4 random dynamic bodies, every body, the container alone (the body with the most contacts), and the container
alone with touching_only = 0 (every contact that names it: its list takes the long-list ordering). Per batch: one call of each kind and the host route, warmed up, then --reps rounds that alternate the
three (other work shares the host: the spread is printed beside the median). Every call blocks until its answer is on the
host, so a host clock around it is the call time. The index sets of the two routes are compared before anything is timed.
Kernel times are a separate run:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_body_contacts.py --reps 1 --out FILE
  python tools/gpu_body_contacts.py --kernels DIR     the calls' kernels in that run's database: launches, median, max
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "box2d-mt_amd", "python"))

import b2harness as bh  # noqa: E402
import b2hip  # noqa: E402

# the Tumbler as bench.py builds and settles it (tools/gpu_queries.py: WORLDS)
TUMBLER = ("config3_tumbler316", bh.TUMBLER, 316, 0, bh.F_SLEEP | bh.F_WARM, 1, 700)


def host_route(dw, bodies, touching_only=True):
    """the (touching) contacts of `bodies` by b2hip_get_contacts and numpy: (offsets, contact indices, seconds of the copy)"""
    t0 = time.perf_counter()
    c = dw.contacts()
    copy_s = time.perf_counter() - t0
    t = np.flatnonzero(c["flags"] & 1) if touching_only else np.arange(len(c))
    key = np.concatenate([c["body_a"][t], c["body_b"][t]])
    idx = np.concatenate([t, t])
    order = np.lexsort((idx, key))
    key, idx = key[order], idx[order]
    lo, hi = np.searchsorted(key, bodies, "left"), np.searchsorted(key, bodies, "right")
    lens = hi - lo
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    take = np.repeat(lo - offsets[:-1], lens) + np.arange(int(lens.sum()))  # body i's range [lo[i], hi[i]) at offsets[i]
    return offsets, idx[take], copy_s


def kernels(directory):
    """the kernels of the two calls in a rocprofv3 --kernel-trace run (rocpd database, `kernels` view)"""
    import collections
    import glob
    import sqlite3
    db = sorted(glob.glob(os.path.join(directory, "**", "*.db"), recursive=True))[0]
    names = ("k_bc_", "k_query_sort", "k_query_mark", "k_query_compact_big", "k_scan")
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start")
    d = collections.defaultdict(list)
    for name, duration in rows:
        short = name.split("(")[0].replace("void ", "")
        if any(n in short for n in names):
            d[short].append(duration / 1000.0)
    for k, v in sorted(d.items()):
        v = sorted(v)
        print("  %-40s launches %4d  median %9.1f us  max %9.1f us" % (k, len(v), v[len(v) // 2], v[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_contacts_tumbler316.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernels", metavar="DIR", default="", help="summarise the -d directory of a rocprofv3 run instead")
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.kernels)
    b2hip.use_torch_hip_runtime()
    h = bh.Harness(bh.AMD_LIB)
    name, scene, p0, p1, flags, seed, settle = TUMBLER
    w = h.world(scene, p0, p1, seed=seed, flags=flags)
    w.step(settle)
    dw = b2hip.World.borrow(w.device_world())
    states, contacts = dw.body_states(), dw.contacts()
    nb = dw.body_count
    per_body = np.bincount(np.concatenate([contacts["body_a"], contacts["body_b"]]), minlength=nb)
    container = int(np.argmax(per_body))
    dynamic = np.flatnonzero(((states["flags"] & 3) == 2) & (np.arange(nb) != container))
    rng = np.random.default_rng(1)
    batches = [("10^4 random dynamic bodies", rng.choice(dynamic, min(10000, len(dynamic)), replace=False).astype(np.int32), True),
               ("every body", np.arange(nb, dtype=np.int32), True),
               ("the container alone", np.asarray([container], np.int32), True),
               ("the container alone, touching_only = 0", np.asarray([container], np.int32), False)]
    lines = ["%s settled %d steps: %d bodies, %d contacts (%d touching), %d on the container (body %d)" % (
        name, settle, nb, len(contacts), int((contacts["flags"] & 1).sum()), int(per_body[container]), container),
        "call times in ms, host clock around blocking calls, median [min .. max] of %d alternating rounds after a warm-up" % args.reps,
        "host route = b2hip_get_contacts (%d B a contact, %.1f MB) + numpy grouping of the listed contacts by body" % (
            contacts.dtype.itemsize, contacts.nbytes / 1e6)]
    for label, bodies, only in batches:
        routes = {"b2hip_body_contacts": lambda: dw.body_contacts(bodies, touching_only=only),
                  "b2hip_body_contact_totals": lambda: dw.body_contact_totals(bodies),
                  "host route": lambda: host_route(dw, bodies, only)}
        offs, recs = routes["b2hip_body_contacts"]()  # (also the warm-up: arrays grown, code objects loaded)
        totals = routes["b2hip_body_contact_totals"]()
        hoffs, hidx, _ = routes["host route"]()
        if not (np.array_equal(offs, hoffs) and np.array_equal(recs["contact_index"], hidx)
                and np.array_equal(totals["touching" if only else "contacts"], np.diff(hoffs))):
            raise SystemExit("%s: the two routes disagree" % label)
        ms = {k: [] for k in routes}
        copy_ms = []
        for _ in range(args.reps):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                r = fn()
                ms[k].append(1000.0 * (time.perf_counter() - t0))
                if k == "host route":
                    copy_ms.append(1000.0 * r[2])
        lines.append("%s: n = %d, %d records, longest list %d" % (label, len(bodies), int(offs[-1]), int(np.diff(offs).max())))
        for k, v in ms.items():
            lines.append("  %-32s %9.3f  [%9.3f .. %9.3f]" % (k, np.median(v), min(v), max(v)))
        lines.append("  %-32s %9.3f  (of the host route)" % ("... its b2hip_get_contacts", np.median(copy_ms)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    dw.close()
    w.close()


if __name__ == "__main__":
    main()
