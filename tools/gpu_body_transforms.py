"""Batched teleports and sleep / wake sets on the device (include/b2hip.h, block H: b2hip_set_transforms, b2hip_set_awakes)
on the settled 100 000-box Tumbler bench.py measures, against the route a caller had before: one b2hip_set_transform or
b2hip_set_awake per body, in the same run.

  python tools/gpu_body_transforms.py [--out FILE] [--reps N] [--slow-reps N] [--fine-reps N]

Cases: 10^4 random dynamic bodies nudged 0.03 m (no proxy leaves its fat box); the same bodies teleported 2 m up; every
dynamic body reset to its pose of 100 steps earlier; b2hip_set_awakes(false) on the 10^4 bodies; the container body alone,
set to the pose it has (its proxy list - four boxes - walked by one lane). The single-body calls edit the host's mirror,
read the fat AABB of every fixture back from the device, and pay again at the next step's upload, so what is timed is "call
+ the next step" for both routes, beside a plain step, through the C ABI (b2hip_step on the drop-in world's device world).
--reps rounds alternate plain step, looped route, batched route on ONE world (other work shares the host: the spread is
printed beside the median); a case whose looped route takes more than a second per round is cut to --slow-reps rounds, and
its line says so. A case whose looped route costs less than a plain step on top of its step - the batch of one body - differs
from the batched route by less than the step's own spread: it gets --fine-reps rounds, and its line says so. The two routes
swap places from round to round, so that neither always runs on the world the other left. A case whose batched median is not
below its looped median is marked NOT FASTER and the tool exits with status 1. Before either route of a round an untimed
batched call puts the bodies back where the case starts from and an untimed step empties the move buffer, so both routes do
the same work. The container is not put back anywhere: its pose is read, untimed, right before each route and set as it is,
so that the drum keeps turning as in a plain run (put back to a pose of many steps ago, its walls would pass through the
boxes that lie against them, and the boxes that got out would fall for ever). The looped calls are made from Python through
ctypes with their arguments prepared beforehand; the loop's own time is printed apart from the step's.
Before anything is timed the two routes are run on twin worlds - built and settled alike - and body_states() right after the
calls and after the next step must agree to the byte, per case.
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
f32 = np.float32


def poses(states, bodies):
    s = states[bodies]
    return np.stack([s["px"], s["py"], s["angle"]], axis=1).astype(f32)


class Case:
    """start: the poses (or None: awake) the bodies are put back to before either route; target: where the routes send them
    (None: asleep). in_place: no start, and the target is the pose the bodies have when a route begins - the world is never
    disturbed, however many rounds are run"""

    def __init__(self, label, bodies, start, target, in_place=False):
        self.label, self.bodies, self.start, self.target = label, np.ascontiguousarray(bodies, np.int32), start, target
        self.in_place = in_place

    def reset(self, dw):
        if self.in_place:
            return
        if self.start is None:
            dw.set_awakes(self.bodies, True)
        else:
            dw.set_transforms(self.bodies, self.start[:, :2], self.start[:, 2])

    def aim(self, dw):
        """right before a route, untimed: an in-place case reads where its bodies are"""
        if self.in_place:
            self.target = poses(dw.body_states_of(self.bodies), slice(None))

    def batched(self, dw):
        if self.target is None:
            dw.set_awakes(self.bodies, False)
        else:
            dw.set_transforms(self.bodies, self.target[:, :2], self.target[:, 2])

    def looped(self, dw):
        """the single-body calls of the batch, arguments prepared: a list of (function, argument tuple)"""
        L, p = dw.L, dw.p
        if self.target is None:
            return [(L.b2hip_set_awake, (p, b, 0)) for b in self.bodies.tolist()]
        return [(L.b2hip_set_transform, (p, b, q[0], q[1], q[2])) for b, q in zip(self.bodies.tolist(), self.target.tolist())]


def run_looped(calls):
    for fn, a in calls:
        if fn(*a) != 0:
            raise SystemExit("a single-body call failed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_transforms_tumbler316.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--fine-reps", type=int, default=1001)
    args = ap.parse_args()
    b2hip.use_torch_hip_runtime()
    h = bh.Harness(bh.AMD_LIB)
    name, scene, p0, p1, flags, seed, settle = TUMBLER
    worlds = []
    for _ in range(2):
        w = h.world(scene, p0, p1, seed=seed, flags=flags)
        w.step(settle - 100)
        worlds.append((w, b2hip.World.borrow(w.device_world())))
    (wa, a), (wb, b) = worlds
    step = lambda dw: dw.step(1.0 / 60.0, wa.vel_iters, wa.pos_iters)  # noqa: E731
    earlier = a.body_states()
    for _ in range(100):
        step(a)
        step(b)
    states = a.body_states()
    nb = a.body_count
    types = states["flags"] & 3
    dynamic = np.flatnonzero(types == 2).astype(np.int32)
    # the container: the dynamic body that may not sleep and carries the four walls (harness/scenes.h: BuildTumbler) - body 1
    container = np.asarray([1], np.int32)
    if types[1] != 2 or (states["flags"][1] & 8) != 0:
        raise SystemExit("body 1 is not the container")
    boxes = dynamic[dynamic != 1]
    rng = np.random.default_rng(1)
    some = np.sort(rng.choice(boxes, min(10000, len(boxes)), replace=False)).astype(np.int32)
    here = poses(states, some)
    cases = [Case("10^4 random dynamic bodies nudged 0.03 m", some, here, here + np.asarray([0.03, 0.0, 0.0], f32)),
             Case("10^4 random dynamic bodies teleported 2 m up", some, here, here + np.asarray([0.0, 2.0, 0.0], f32)),
             Case("every dynamic body reset to its pose of 100 steps earlier", dynamic, poses(states, dynamic), poses(earlier, dynamic)),
             Case("set_awakes(false) on 10^4 random dynamic bodies", some, None, None),
             # (in place: put back to a pose of many steps ago, the walls would pass through the boxes that lie against them)
             Case("the container body alone, set to the pose it has (4 proxies on one lane)", container, None, None, in_place=True)]
    lines = ["command: python tools/gpu_body_transforms.py --reps %d --slow-reps %d --fine-reps %d" % (args.reps, args.slow_reps, args.fine_reps),
             "%s settled %d steps: %d bodies, %d dynamic, %d awake" % (name, settle, nb, len(dynamic), int(((states["flags"] & 4) != 0).sum())),
             "ms, host clock around blocking calls, median [min .. max] of alternating rounds after a warm-up; steps through b2hip_step",
             "looped route = one single-body C call per body from Python (ctypes, arguments prepared), paid for again at the next step's upload"]
    # ---- the two routes agree, per case, on twin worlds ----------------------------------------------------------------------
    if a.body_states().tobytes() != b.body_states().tobytes():
        raise SystemExit("the twin worlds differ before anything was done")
    for case in cases:
        case.aim(a)
        case.batched(a)
        run_looped(case.looped(b))
        if a.body_states().tobytes() != b.body_states().tobytes():
            raise SystemExit("%s: the two routes disagree right after the call" % case.label)
        step(a)
        step(b)
        if a.body_states().tobytes() != b.body_states().tobytes():
            raise SystemExit("%s: the two routes disagree after the next step" % case.label)
        for dw in (a, b):
            case.reset(dw)
            step(dw)
        print("agree: %s" % case.label, file=sys.stderr, flush=True)
    lines.append("the two routes agree on body_states() to the byte, right after the calls and after the next step (%d cases, twin worlds)" % len(cases))
    b.close()
    wb.close()
    # ---- timing, on one world ---------------------------------------------------------------------------------------------------
    failed = []
    for case in cases:
        keys = ("plain step", "looped: the calls", "looped: the next step", "batched: the call", "batched: the next step")
        ms = {k: [] for k in keys}

        def timed(key, fn):
            t0 = time.perf_counter()
            fn()
            ms[key].append(1000.0 * (time.perf_counter() - t0))

        def looped_route():
            case.reset(a)
            step(a)
            case.aim(a)
            calls = case.looped(a)
            timed("looped: the calls", lambda: run_looped(calls))
            timed("looped: the next step", lambda: step(a))

        def batched_route():
            case.reset(a)
            step(a)
            case.aim(a)
            timed("batched: the call", lambda: case.batched(a))
            timed("batched: the next step", lambda: step(a))

        reps, rep, note = args.reps, 0, ""
        while rep < reps + 1:
            timed("plain step", lambda: step(a))
            for route in ((looped_route, batched_route) if rep % 2 == 0 else (batched_route, looped_route)):
                route()
            if rep % 100 == 99:
                print("  round %d of %d" % (rep + 1, reps + 1), file=sys.stderr, flush=True)
            if ms["plain step"] and ms["plain step"][-1] > 20.0 * ms["plain step"][0] + 50.0:
                raise SystemExit("%s: the plain step has grown from %.3f to %.3f ms: the rounds disturb the world" %
                                 (case.label, ms["plain step"][0], ms["plain step"][-1]))
            if rep == 0:  # (the warm-up: arrays grown, code objects loaded)
                looped0 = ms["looped: the calls"][0] + ms["looped: the next step"][0]
                if looped0 > 1000.0 and reps > args.slow_reps:
                    reps, note = args.slow_reps, " (cut: the looped route takes more than a second a round)"
                elif looped0 < 2.0 * ms["plain step"][0] and reps < args.fine_reps:
                    reps, note = args.fine_reps, " (raised: the looped route costs less than a plain step on top of its step)"
                for v in ms.values():
                    v.clear()
            rep += 1
        print("timed: %s" % case.label, file=sys.stderr, flush=True)
        lines.append("%s: n = %d, %d rounds%s" % (case.label, len(case.bodies), reps, note))
        for k in keys:
            v = ms[k]
            lines.append("  %-28s %10.3f  [%10.3f .. %10.3f]" % (k, np.median(v), min(v), max(v)))
        lo = np.asarray(ms["looped: the calls"]) + np.asarray(ms["looped: the next step"])
        ba = np.asarray(ms["batched: the call"]) + np.asarray(ms["batched: the next step"])
        lines.append("  %-28s %10.3f  [%10.3f .. %10.3f]" % ("looped: call + step", np.median(lo), lo.min(), lo.max()))
        lines.append("  %-28s %10.3f  [%10.3f .. %10.3f]" % ("batched: call + step", np.median(ba), ba.min(), ba.max()))
        d = lo - ba  # (round by round: both routes of a round ran within a few steps of each other)
        lines.append("  %-28s %10.3f  [%10.3f .. %10.3f]  batched below looped in %d of %d rounds" %
                     ("looped - batched, per round", np.median(d), d.min(), d.max(), int((d > 0).sum()), len(d)))
        if not np.median(ba) < np.median(lo):
            lines.append("  NOT FASTER: the batched route does not beat the looped one here")
            failed.append(case.label)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    a.close()
    wa.close()
    if failed:
        raise SystemExit("batched call + step is not below looped calls + step: %s" % "; ".join(failed))


if __name__ == "__main__":
    main()
