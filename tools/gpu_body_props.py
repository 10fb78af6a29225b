"""Batched body property sets on the device (include/b2hip.h, block K: b2hip_set_types, b2hip_set_bullets,
b2hip_set_fixed_rotations, b2hip_set_sleeping_alloweds, b2hip_set_body_dampings, b2hip_set_mass_datas, b2hip_reset_mass_datas)
on the settled 100 000-box Tumbler bench.py measures, against the route a caller had before: one single-body call per body,
in the same run.

  python tools/gpu_body_props.py [--out FILE] [--reps N] [--bodies N] [--slow-bodies N] [--no-toi]

Cases, each timed together with the step that follows it, beside a plain step, through the C ABI (b2hip_step on the drop-in
world's device world), on N random dynamic boxes (--bodies, 10^4): the linear damping set; sleeping forbidden and allowed
again; the rotation fixed and let go; explicit mass data; the mass data reset; the bullet flag on and off; the type changed to
kinematic and back to dynamic (the D -> K -> D round trip). The batched route runs --reps rounds. The looped route runs one
round: at N for the calls that only edit rows, and at --slow-bodies (10^3) for b2hip_set_type and b2hip_set_bullet, which queue
one contact-array operation per body - a walk of one workgroup over the whole contact array each; their figure at N is a
PROJECTION (x N / slow-bodies), named as one. The looped calls are made from Python through ctypes with their arguments
prepared beforehand.
Unless --no-toi is given a second Tumbler is built with continuous collision on, where the bullet flag decides which contacts
are candidates: the batched bullet sets are timed there at N bodies, and the one-lane replay of the listed contacts is
reported apart (the call with the replay less the same call on bodies that have the flag already, which lists nothing), with
the number of slots the partition gained.
Before anything is timed the two routes are run on twin worlds - built and settled alike - with 10^2 bodies per case, and
body_states() after every call (behind a read of the contact count, which makes the looped route apply its queued operations)
and after the step that follows must agree to the byte.
"""
import argparse
import ctypes as C
import os
import struct
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
# (case, slow: the single call queues a contact-array operation)
CASES = (("dampings", False), ("sleeping off", False), ("sleeping on", False), ("fixed rotation on", False), ("fixed rotation off", False),
         ("mass data", False), ("mass data reset", False), ("bullets on", True), ("bullets off", True), ("types D->K", True), ("types K->D", True))
MASS = (1.0, 0.2, (0.01, 0.0))


def looped(dw, case, bodies):
    L, p = dw.L, dw.p
    ids = bodies.tolist()
    if case == "dampings":
        calls = [(L.b2hip_set_body_damping, (p, q, 0.01, 0.0, 1.0)) for q in ids]
    elif case.startswith("sleeping"):
        calls = [(L.b2hip_set_sleeping_allowed, (p, q, int(case.endswith("on")))) for q in ids]
    elif case.startswith("fixed"):
        calls = [(L.b2hip_set_fixed_rotation, (p, q, int(case.endswith("on")))) for q in ids]
    elif case == "mass data":
        md = np.zeros(1, b2hip.MASS_DATA_DTYPE)
        md["mass"], md["inertia"], md["local_center"] = MASS
        ptr = md.ctypes.data_as(C.c_void_p)
        calls = [(L.b2hip_set_mass_data, (p, q, ptr)) for q in ids]
    elif case == "mass data reset":
        calls = [(L.b2hip_set_mass_data, (p, q, None)) for q in ids]
    elif case.startswith("bullets"):
        calls = [(L.b2hip_set_bullet, (p, q, int(case.endswith("on")))) for q in ids]
    else:
        calls = [(L.b2hip_set_type, (p, q, b2hip.KINEMATIC if case.endswith("->K") else b2hip.DYNAMIC)) for q in ids]
    t0 = time.perf_counter()
    for fn, a in calls:
        if fn(*a) != 0:
            raise SystemExit("a single-body call failed: %s" % L.b2hip_last_error().decode())
    return 1000.0 * (time.perf_counter() - t0)


def batched(dw, case, bodies):
    t0 = time.perf_counter()
    if case == "dampings":
        dw.set_body_dampings(bodies, linear=0.01)
    elif case.startswith("sleeping"):
        dw.set_sleeping_alloweds(bodies, case.endswith("on"))
    elif case.startswith("fixed"):
        dw.set_fixed_rotations(bodies, case.endswith("on"))
    elif case == "mass data":
        dw.set_mass_datas(bodies, *MASS)
    elif case == "mass data reset":
        dw.reset_mass_datas(bodies)
    elif case.startswith("bullets"):
        dw.set_bullets(bodies, case.endswith("on"))
    else:
        dw.set_types(bodies, b2hip.KINEMATIC if case.endswith("->K") else b2hip.DYNAMIC)
    return 1000.0 * (time.perf_counter() - t0)


def stat(v):
    return "%10.3f  [%10.3f .. %10.3f]" % (np.median(v), min(v), max(v))


def toi_slots(dw):
    return struct.unpack_from("<I", dw.save_snapshot(), 8 + 4 * 12)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_props_tumbler316.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bodies", type=int, default=10000)
    ap.add_argument("--slow-bodies", type=int, default=1000)
    ap.add_argument("--no-toi", action="store_true")
    args = ap.parse_args()
    b2hip.use_torch_hip_runtime()
    h = bh.Harness(bh.AMD_LIB)
    name, scene, p0, p1, flags, seed, settle = TUMBLER

    def tumbler(world_flags):
        w = h.world(scene, p0, p1, seed=seed, flags=world_flags)
        w.step(settle)
        return w, b2hip.World.borrow(w.device_world())

    wa, a = tumbler(flags)
    wb, b = tumbler(flags)
    step = lambda dw: dw.step(1.0 / 60.0, wa.vel_iters, wa.pos_iters)  # noqa: E731

    def timed_step(dw):
        t0 = time.perf_counter()
        step(dw)
        return 1000.0 * (time.perf_counter() - t0)

    states = a.body_states()
    boxes = np.flatnonzero((np.arange(a.body_count) > 1) & ((states["flags"] & 3) == 2))
    pool = np.random.default_rng(1).permutation(boxes).astype(np.int32)
    cursor = [0]

    def fresh(n):
        """n boxes nobody has named yet"""
        if cursor[0] + n > len(pool):
            raise SystemExit("out of bodies")
        cursor[0] += n
        return np.ascontiguousarray(pool[cursor[0] - n:cursor[0]])

    n, slow = args.bodies, min(args.slow_bodies, args.bodies)
    lines = ["command: python tools/gpu_body_props.py --reps %d --bodies %d --slow-bodies %d%s" % (args.reps, n, slow, " --no-toi" if args.no_toi else ""),
             "%s settled %d steps: %d bodies, %d awake, %d contacts" % (name, settle, a.body_count, int(((states["flags"] & 4) != 0).sum()), a.contact_count),
             "ms, host clock around blocking calls, median [min .. max]; steps through b2hip_step; every case is the call(s) + the step that follows",
             "looped route = one single-body C call per body from Python (ctypes, arguments prepared); its uploads and contact operations run in the step that follows",
             "(the parent commit has no batched route: both routes' times are of this run)"]
    # ---- the two routes agree on twin worlds ------------------------------------------------------------------------------------------
    if a.body_states().tobytes() != b.body_states().tobytes():
        raise SystemExit("the twin worlds differ before anything was done")
    some = fresh(100)
    for case, _ in CASES:
        batched(a, case, some)
        looped(b, case, some)
        if a.contact_count != b.contact_count or a.body_states().tobytes() != b.body_states().tobytes():
            raise SystemExit("%s: the two routes disagree right after the call" % case)
        step(a)
        step(b)
        if a.body_states().tobytes() != b.body_states().tobytes():
            raise SystemExit("%s: the two routes disagree after the next step" % case)
        print("agree: %s" % case, file=sys.stderr, flush=True)
    lines.append("the two routes agree on body_states() to the byte, right after the calls and after the next step (%d cases, 100 bodies, twin worlds)" % len(CASES))
    b.close()
    wb.close()
    # ---- the looped route: one round ----------------------------------------------------------------------------------------------------
    for _ in range(3):
        step(a)
    lines.append("looped route, one round: n = %d for the calls that edit rows only, n = %d for b2hip_set_type and b2hip_set_bullet (a contact-array walk each)" % (n, slow))
    lf, ls = fresh(n), fresh(slow)
    for case, is_slow in CASES:
        who = ls if is_slow else lf
        plain = timed_step(a)
        lc = looped(a, case, who)
        st = timed_step(a)
        lines.append("  %-20s n = %6d  plain step %8.3f   calls %10.3f + step %10.3f = %10.3f%s" % (
            case, len(who), plain, lc, st, lc + st,
            "   PROJECTED to n = %d, not measured: %.0f" % (n, (lc + st) * n / len(who)) if is_slow and len(who) < n else ""))
        print(lines[-1], file=sys.stderr, flush=True)
    # ---- the batched route at n -----------------------------------------------------------------------------------------------------------
    ms = {k: [] for k in ("plain step",) + tuple("%s: %s" % (c, part) for c, _ in CASES for part in ("the call", "the next step"))}
    mine = fresh(n)
    for rep in range(args.reps + 1):
        ms["plain step"].append(timed_step(a))
        for case, _ in CASES:
            ms["%s: the call" % case].append(batched(a, case, mine))
            ms["%s: the next step" % case].append(timed_step(a))
        if rep == 0:  # (the warm-up: arrays grown, code objects loaded)
            for v in ms.values():
                v.clear()
    lines.append("batched route, n = %d, %d rounds after a warm-up (%d contacts at the end)" % (n, args.reps, a.contact_count))
    lines.append("  %-32s %s" % ("plain step", stat(ms["plain step"])))
    for case, _ in CASES:
        c, s = np.asarray(ms["%s: the call" % case]), np.asarray(ms["%s: the next step" % case])
        lines.append("  %-32s %s" % (case + ": the call", stat(c)))
        lines.append("  %-32s %s" % (case + ": the next step", stat(s)))
        lines.append("  %-32s %s" % (case + ": call + step", stat(c + s)))
    a.close()
    wa.close()
    # ---- the one-lane TOI replay, on a world with continuous collision on ------------------------------------------------------------------
    if args.no_toi:
        lines.append("the one-lane TOI replay: NOT TIMED YET (--no-toi)")
    else:
        wc, c = tumbler(flags | bh.F_CONTINUOUS)
        sc = c.body_states()
        cboxes = np.flatnonzero((np.arange(c.body_count) > 1) & ((sc["flags"] & 3) == 2))
        who = np.ascontiguousarray(np.random.default_rng(2).permutation(cboxes)[:n].astype(np.int32))
        lines.append("continuous collision on: %s settled %d steps, %d contacts, %d slots in the TOI partition" % (name, settle, c.contact_count, toi_slots(c)))
        on, again, off, gained = [], [], [], []
        for rep in range(args.reps + 1):
            before = toi_slots(c)
            on.append(batched(c, "bullets on", who))
            gained.append(toi_slots(c) - before)
            again.append(batched(c, "bullets on", who))  # (every entry has the flag already: rows written, no contact pass)
            off.append(batched(c, "bullets off", who))
            if rep == 0:
                on, again, off, gained = [], [], [], []
        lines.append("  bullets on, n = %d: the call      %s   (the partition gained %s slots)" % (n, stat(on), sorted(set(gained))))
        lines.append("  bullets on again (no-op entries)  %s" % stat(again))
        lines.append("  bullets off: the call             %s" % stat(off))
        lines.append("  the contact pass, the sort and the ONE-LANE REPLAY of the listed contacts (on less on-again): %.3f ms for %d contacts" % (
            np.median(on) - np.median(again), int(np.median(gained))))
        c.close()
        wc.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
