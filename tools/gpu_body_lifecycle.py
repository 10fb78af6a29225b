"""Batched body destruction and activation sets on the device (include/b2hip.h, block I: b2hip_destroy_bodies,
b2hip_set_actives) on the settled 100 000-box Tumbler bench.py measures, against the route a caller had before: one
b2hip_set_active or b2hip_destroy_body per body, in the same run.

  python tools/gpu_body_lifecycle.py [--out FILE] [--reps N] [--bodies N] [--looped-limit SECONDS] [--batched-only]

Cases, each timed together with the step that follows it, beside a plain step, through the C ABI (b2hip_step on the drop-in
world's device world): N random dynamic boxes deactivated; the same boxes re-activated; N boxes destroyed (another N in every
round: a destroyed body does not come back). The batched route runs --reps rounds at N = --bodies (10^4).
The looped route queues one contact-array operation per body, and each operation is a walk of one workgroup over the whole
contact array: it is timed first at 10^2 bodies, and at 10^3 and 10^4 only while the size before projects the next one to
less than --looped-limit seconds (60) for a case; otherwise the largest size run is reported with the projection, named as
one. The batched route is timed at every size the looped route ran at as well, so that each looped figure has a batched
figure of the same size from the same run beside it. The looped calls are made from Python through ctypes with their
arguments prepared beforehand.
Before anything is timed the two routes are run on twin worlds - built and settled alike - with 10^2 bodies per case, and
body_states() after every call (behind a read of the contact count, which makes the looped route apply its queued
operations) and after the step that follows must agree to the byte.
--batched-only skips the twin and the looped route: the run a kernel profiler wraps.
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
CASES = ("deactivate", "re-activate", "destroy")


def looped(dw, case, bodies):
    L, p = dw.L, dw.p
    if case == "destroy":
        calls = [(L.b2hip_destroy_body, (p, b)) for b in bodies.tolist()]
    else:
        calls = [(L.b2hip_set_active, (p, b, int(case == "re-activate"))) for b in bodies.tolist()]
    t0 = time.perf_counter()
    for fn, a in calls:
        if fn(*a) != 0:
            raise SystemExit("a single-body call failed: %s" % L.b2hip_last_error().decode())
    return 1000.0 * (time.perf_counter() - t0)


def batched(dw, case, bodies):
    t0 = time.perf_counter()
    if case == "destroy":
        dw.destroy_bodies(bodies)
    else:
        dw.set_actives(bodies, case == "re-activate")
    return 1000.0 * (time.perf_counter() - t0)


def stat(v):
    return "%10.3f  [%10.3f .. %10.3f]" % (np.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_lifecycle_tumbler316.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bodies", type=int, default=10000)
    ap.add_argument("--looped-limit", type=float, default=60.0)
    ap.add_argument("--batched-only", action="store_true")
    args = ap.parse_args()
    b2hip.use_torch_hip_runtime()
    h = bh.Harness(bh.AMD_LIB)
    name, scene, p0, p1, flags, seed, settle = TUMBLER
    worlds = []
    for _ in range(1 if args.batched_only else 2):
        w = h.world(scene, p0, p1, seed=seed, flags=flags)
        w.step(settle)
        worlds.append((w, b2hip.World.borrow(w.device_world())))
    wa, a = worlds[0]
    step = lambda dw: dw.step(1.0 / 60.0, wa.vel_iters, wa.pos_iters)  # noqa: E731

    def timed_step(dw):
        t0 = time.perf_counter()
        step(dw)
        return 1000.0 * (time.perf_counter() - t0)

    states = a.body_states()
    types = states["flags"] & 3
    dynamic = np.flatnonzero(types == 2).astype(np.int32)
    if types[1] != 2 or (states["flags"][1] & 8) != 0:
        raise SystemExit("body 1 is not the container")
    boxes = np.random.default_rng(1).permutation(dynamic[dynamic != 1]).astype(np.int32)
    cursor = [0]

    def fresh(n):
        """n boxes nobody has named yet"""
        if cursor[0] + n > len(boxes):
            raise SystemExit("out of boxes")
        cursor[0] += n
        return np.ascontiguousarray(boxes[cursor[0] - n:cursor[0]])

    lines = ["command: python tools/gpu_body_lifecycle.py --reps %d --bodies %d --looped-limit %g%s" %
             (args.reps, args.bodies, args.looped_limit, " --batched-only" if args.batched_only else ""),
             "%s settled %d steps: %d bodies, %d dynamic, %d awake, %d contacts" %
             (name, settle, a.body_count, len(dynamic), int(((states["flags"] & 4) != 0).sum()), a.contact_count),
             "ms, host clock around blocking calls, median [min .. max]; steps through b2hip_step; every case is the call(s) + the step that follows",
             "looped route = one single-body C call per body from Python (ctypes, arguments prepared); its contact operations run in the step that follows",
             "(the parent commit has no batched route: both routes' times are of this run)"]
    # ---- the two routes agree on twin worlds --------------------------------------------------------------------------------------
    if not args.batched_only:
        wb, b = worlds[1]
        if a.body_states().tobytes() != b.body_states().tobytes():
            raise SystemExit("the twin worlds differ before anything was done")
        pool = fresh(200)
        for case, bodies in (("deactivate", pool[:100]), ("re-activate", pool[:100]), ("destroy", pool[100:])):
            batched(a, case, bodies)
            looped(b, case, bodies)
            if a.contact_count != b.contact_count or a.body_states().tobytes() != b.body_states().tobytes():
                raise SystemExit("%s: the two routes disagree right after the call" % case)
            step(a)
            step(b)
            if a.body_states().tobytes() != b.body_states().tobytes():
                raise SystemExit("%s: the two routes disagree after the next step" % case)
            print("agree: %s" % case, file=sys.stderr, flush=True)
        lines.append("the two routes agree on body_states() to the byte, right after the calls and after the next step (3 cases of 100 bodies, twin worlds)")
        b.close()
        wb.close()
    # ---- the looped route, from 10^2 bodies up, and the batched route at the same sizes --------------------------------------------
    for _ in range(3):
        step(a)
    if not args.batched_only:
        size, go = 100, True
        while go and size <= args.bodies:
            act, gone = fresh(size), fresh(size)
            act2, gone2 = fresh(size), fresh(size)
            plain = timed_step(a)
            worst = 0.0
            lines.append("n = %d, one round: plain step %.3f" % (size, plain))
            for case, lb, bb in (("deactivate", act, act2), ("re-activate", act, act2), ("destroy", gone, gone2)):
                lc = looped(a, case, lb)
                ls = timed_step(a)
                bc = batched(a, case, bb)
                bs = timed_step(a)
                worst = max(worst, lc + ls)
                lines.append("  %-12s looped: calls %10.3f + step %10.3f = %10.3f    batched: call %8.3f + step %8.3f = %8.3f" %
                             (case, lc, ls, lc + ls, bc, bs, bc + bs))
                print(lines[-1], file=sys.stderr, flush=True)
            nxt = size * 10
            projected = worst * nxt / size / 1000.0
            if nxt <= args.bodies and projected >= args.looped_limit:
                lines.append("  the looped route at n = %d is a PROJECTION, not a measurement: %.0f s for its slowest case (%.3f ms x %d); not run" %
                             (nxt, projected, worst, nxt // size))
                if nxt * 10 <= args.bodies:
                    lines.append("  ... and at n = %d, projected the same way: %.0f s" % (nxt * 10, projected * 10))
                go = False
            size = nxt
    # ---- the batched route at --bodies ------------------------------------------------------------------------------------------
    n = args.bodies
    ms = {k: [] for k in ("plain step",) + tuple("%s: %s" % (c, part) for c in CASES for part in ("the call", "the next step"))}
    some = fresh(n)
    for rep in range(args.reps + 1):
        gone = fresh(n)
        ms["plain step"].append(timed_step(a))
        for case, bodies in (("deactivate", some), ("re-activate", some), ("destroy", gone)):
            ms["%s: the call" % case].append(batched(a, case, bodies))
            ms["%s: the next step" % case].append(timed_step(a))
        if rep == 0:  # (the warm-up: arrays grown, code objects loaded)
            for v in ms.values():
                v.clear()
    lines.append("batched route, n = %d, %d rounds after a warm-up (every round destroys another %d boxes: %d contacts at the end)" %
                 (n, args.reps, n, a.contact_count))
    lines.append("  %-28s %s" % ("plain step", stat(ms["plain step"])))
    for case in CASES:
        c, s = np.asarray(ms["%s: the call" % case]), np.asarray(ms["%s: the next step" % case])
        lines.append("  %-28s %s" % (case + ": the call", stat(c)))
        lines.append("  %-28s %s" % (case + ": the next step", stat(s)))
        lines.append("  %-28s %s" % (case + ": call + step", stat(c + s)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    a.close()
    wa.close()


if __name__ == "__main__":
    main()
