"""Batched fixture filter, sensor and material sets on the device (include/b2hip.h, block J: b2hip_fixture_set_filters,
b2hip_fixture_set_sensors, b2hip_fixture_set_materials) on the settled 100 000-box Tumbler bench.py measures, against the
route a caller had before: one b2hip_fixture_set_filter, _sensor or _material per fixture, in the same run.

  python tools/gpu_fixture_batch.py [--out FILE] [--reps N] [--fixtures N] [--looped-limit SECONDS] [--batched-only]

Cases, each timed together with the step that follows it, beside a plain step, through the C ABI (b2hip_step on the drop-in
world's device world): the filters of N random boxes' fixtures set (a second category bit: every contact of theirs is
re-filtered and stays); the same fixtures made sensors, and solid again; the friction of EVERY fixture of the world set.
The batched route runs --reps rounds at N = --fixtures (10^4).
The looped route queues one or two contact-array operations per fixture, and each operation is a walk of one workgroup over
the whole contact array: it is timed first at 10^2 fixtures, and at 10^3 and 10^4 only while the size before projects the
next one to less than --looped-limit seconds (60) for a case; otherwise the largest size run is reported with the projection,
named as one. The batched route is timed at every size the looped route ran at as well, so that each looped figure has a
batched figure of the same size from the same run beside it. The looped friction case names every fixture at every size
(it queues no contact operation). The looped calls are made from Python through ctypes with their arguments prepared
beforehand.
Before anything is timed the two routes are run on twin worlds - built and settled alike - with 10^2 fixtures per case, and
body_states() after every call (behind a read of the contact count, which makes the looped route apply its queued operations)
and after the step that follows must agree to the byte.
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
CASES = ("filters", "sensors on", "sensors off", "friction")
FRICTION = 0.35


def looped(dw, case, fixtures, materials=None):
    L, p = dw.L, dw.p
    if case == "filters":
        calls = [(L.b2hip_fixture_set_filter, (p, f, 3, 0xFFFF, 0)) for f in fixtures.tolist()]
    elif case == "friction":
        calls = [(L.b2hip_fixture_set_material, (p, f, float(d), FRICTION, float(r))) for f, (d, r) in zip(fixtures.tolist(), materials)]
    else:
        calls = [(L.b2hip_fixture_set_sensor, (p, f, int(case == "sensors on"))) for f in fixtures.tolist()]
    t0 = time.perf_counter()
    for fn, a in calls:
        if fn(*a) != 0:
            raise SystemExit("a single-fixture call failed: %s" % L.b2hip_last_error().decode())
    return 1000.0 * (time.perf_counter() - t0)


def batched(dw, case, fixtures):
    t0 = time.perf_counter()
    if case == "filters":
        dw.fixture_set_filters(fixtures, 3, 0xFFFF, 0)
    elif case == "friction":
        dw.fixture_set_materials(fixtures, friction=FRICTION)
    else:
        dw.fixture_set_sensors(fixtures, case == "sensors on")
    return 1000.0 * (time.perf_counter() - t0)


def stat(v):
    return "%10.3f  [%10.3f .. %10.3f]" % (np.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixture_batch_tumbler316.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fixtures", type=int, default=10000)
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
    if (states["flags"][1] & 3) != 2 or (states["flags"][1] & 8) != 0:
        raise SystemExit("body 1 is not the container")
    # every proxy and its body, from one query over the whole world; the boxes' fixtures are the ones not on the container
    _, items = a.query_aabbs(np.asarray([[-1e6, -1e6]], np.float32), np.asarray([[1e6, 1e6]], np.float32))
    nf = a.L.b2hip_fixture_count(a.p)
    every = np.arange(nf, dtype=np.int32)
    box_fixtures = np.random.default_rng(1).permutation(items["fixture"][items["body"] > 1]).astype(np.int32)
    # (the loop passes the density and restitution a fixture has: the scene's boxes share theirs, the container's walls theirs)
    on_container = np.zeros(nf, bool)
    on_container[items["fixture"][items["body"] == 1]] = True
    materials = [(5.0, 0.0) if c else (1.0, 0.0) for c in on_container.tolist()]
    cursor = [0]

    def fresh(n):
        """n box fixtures nobody has named yet"""
        if cursor[0] + n > len(box_fixtures):
            raise SystemExit("out of fixtures")
        cursor[0] += n
        return np.ascontiguousarray(box_fixtures[cursor[0] - n:cursor[0]])

    lines = ["command: python tools/gpu_fixture_batch.py --reps %d --fixtures %d --looped-limit %g%s" %
             (args.reps, args.fixtures, args.looped_limit, " --batched-only" if args.batched_only else ""),
             "%s settled %d steps: %d bodies, %d fixtures, %d awake, %d contacts" %
             (name, settle, a.body_count, nf, int(((states["flags"] & 4) != 0).sum()), a.contact_count),
             "ms, host clock around blocking calls, median [min .. max]; steps through b2hip_step; every case is the call(s) + the step that follows",
             "looped route = one single-fixture C call per fixture from Python (ctypes, arguments prepared); its contact operations run in the step that follows",
             "friction names EVERY fixture of the world (%d) at every size; the other cases n random boxes' fixtures" % nf,
             "(the parent commit has no batched route: both routes' times are of this run)"]
    # ---- the two routes agree on twin worlds --------------------------------------------------------------------------------------
    if not args.batched_only:
        wb, b = worlds[1]
        if a.body_states().tobytes() != b.body_states().tobytes():
            raise SystemExit("the twin worlds differ before anything was done")
        pool = fresh(100)
        for case, fixtures in (("filters", pool), ("sensors on", pool), ("sensors off", pool), ("friction", every)):
            batched(a, case, fixtures)
            looped(b, case, fixtures, materials)
            if a.contact_count != b.contact_count or a.body_states().tobytes() != b.body_states().tobytes():
                raise SystemExit("%s: the two routes disagree right after the call" % case)
            step(a)
            step(b)
            if a.body_states().tobytes() != b.body_states().tobytes():
                raise SystemExit("%s: the two routes disagree after the next step" % case)
            print("agree: %s" % case, file=sys.stderr, flush=True)
        lines.append("the two routes agree on body_states() to the byte, right after the calls and after the next step (4 cases, 100 fixtures / every fixture, twin worlds)")
        b.close()
        wb.close()
    # ---- the looped route, from 10^2 fixtures up, and the batched route at the same sizes ------------------------------------------
    for _ in range(3):
        step(a)
    if not args.batched_only:
        size, go = 100, True
        while go and size <= args.fixtures:
            lf, bf = fresh(size), fresh(size)
            plain = timed_step(a)
            worst = 0.0
            lines.append("n = %d, one round: plain step %.3f" % (size, plain))
            for case in CASES:
                lc = looped(a, case, every if case == "friction" else lf, materials)
                ls = timed_step(a)
                bc = batched(a, case, every if case == "friction" else bf)
                bs = timed_step(a)
                if case != "friction":
                    worst = max(worst, lc + ls)
                lines.append("  %-12s looped: calls %10.3f + step %10.3f = %10.3f    batched: call %8.3f + step %8.3f = %8.3f" %
                             (case, lc, ls, lc + ls, bc, bs, bc + bs))
                print(lines[-1], file=sys.stderr, flush=True)
            nxt = size * 10
            projected = worst * nxt / size / 1000.0
            if nxt <= args.fixtures and projected >= args.looped_limit:
                lines.append("  the looped route at n = %d is a PROJECTION, not a measurement: %.0f s for its slowest case (%.3f ms x %d); not run" %
                             (nxt, projected, worst, nxt // size))
                if nxt * 10 <= args.fixtures:
                    lines.append("  ... and at n = %d, projected the same way: %.0f s" % (nxt * 10, projected * 10))
                go = False
            size = nxt
    # ---- the batched route at --fixtures ------------------------------------------------------------------------------------------
    n = args.fixtures
    ms = {k: [] for k in ("plain step",) + tuple("%s: %s" % (c, part) for c in CASES for part in ("the call", "the next step"))}
    some = fresh(n)
    for rep in range(args.reps + 1):
        ms["plain step"].append(timed_step(a))
        for case in CASES:
            ms["%s: the call" % case].append(batched(a, case, every if case == "friction" else some))
            ms["%s: the next step" % case].append(timed_step(a))
        if rep == 0:  # (the warm-up: arrays grown, code objects loaded)
            for v in ms.values():
                v.clear()
    lines.append("batched route, n = %d (friction: %d), %d rounds after a warm-up (%d contacts at the end)" % (n, nf, args.reps, a.contact_count))
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
