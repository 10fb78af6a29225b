"""Batched body writes on the device (include/b2hip.h, block F: b2hip_apply_forces, b2hip_apply_impulses,
b2hip_set_velocities) on the settled 100 000-box Tumbler bench.py measures, against the route a caller had before: one
single-body call per body (b2hip_apply_force, b2hip_apply_linear_impulse + b2hip_apply_angular_impulse, b2hip_set_velocity),
in the same run.

  python tools/gpu_body_writes.py [--out FILE] [--reps N]

Two batches: 10^4 random dynamic bodies and every dynamic body. The single-body calls edit the host's mirror and pay at the
next step's upload, so what is timed is "write + the next step" for both routes, beside a plain step, through the C ABI
(b2hip_step on the drop-in world's device world, as bench.py's sharded runs step). --reps rounds alternate plain step, looped
route, batched route on ONE world (other work shares the host: the spread is printed beside the median); the looped calls are
made from Python through ctypes with their arguments prepared beforehand, and the loop's own time is printed apart from the
step's so that the interpreter's share can be seen. The pushes are small (forces of 0.01 N, impulses of 1e-5 N s, velocities
set to what they were when the batch was drawn) so that the pile stays the settled pile while it is measured.
Before anything is timed the two routes are run on twin worlds - built and settled alike - and body_states() after the next
step must agree to the byte, per family.
"""
import argparse
import ctypes as C
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
FAMILIES = ("forces", "impulses", "velocities")


def pushes(n, scale, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, b2hip.BODY_PUSH_DTYPE)
    p["x"], p["y"] = rng.uniform(-scale, scale, n), rng.uniform(-scale, scale, n)
    p["angular"] = rng.uniform(-0.1 * scale, 0.1 * scale, n)
    return p  # (at the centre of mass: the looped route needs no body state to form a torque)


def looped(dw, family, bodies, data):
    """the single-body calls of the batch, arguments prepared: a list of (function, argument tuple)"""
    L, p = dw.L, dw.p
    calls = []
    if family == "velocities":
        for b, v in zip(bodies.tolist(), data.tolist()):
            calls.append((L.b2hip_set_velocity, (p, b, v[0], v[1], v[2])))
        return calls
    for b, q in zip(bodies.tolist(), data.tolist()):
        if family == "forces":
            calls.append((L.b2hip_apply_force, (p, b, q[0], q[1], q[2], 1)))
        else:
            calls.append((L.b2hip_apply_linear_impulse_to_center, (p, b, q[0], q[1], 1)))
            calls.append((L.b2hip_apply_angular_impulse, (p, b, q[2], 1)))
    return calls


def run_looped(calls):
    for fn, a in calls:
        if fn(*a) != 0:
            raise SystemExit("a single-body call failed")


def batched(dw, family, bodies, data):
    if family == "forces":
        dw.apply_forces(bodies, data)
    elif family == "impulses":
        dw.apply_impulses(bodies, data)
    else:
        dw.set_velocities(bodies, data[:, :2], data[:, 2])


def data_of(dw, family, bodies, seed):
    if family == "forces":
        return pushes(len(bodies), 0.01, seed)
    if family == "impulses":
        return pushes(len(bodies), 1e-5, seed)
    s = dw.body_states()[bodies]
    return np.stack([s["vx"], s["vy"], s["w"]], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_writes_tumbler316.txt"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    b2hip.use_torch_hip_runtime()
    h = bh.Harness(bh.AMD_LIB)
    name, scene, p0, p1, flags, seed, settle = TUMBLER
    worlds = []
    for _ in range(2):
        w = h.world(scene, p0, p1, seed=seed, flags=flags)
        w.step(settle)
        worlds.append((w, b2hip.World.borrow(w.device_world())))
    (wa, a), (wb, b) = worlds
    step = lambda dw: dw.step(1.0 / 60.0, wa.vel_iters, wa.pos_iters)  # noqa: E731
    states = a.body_states()
    nb = a.body_count
    dynamic = np.flatnonzero((states["flags"] & 3) == 2).astype(np.int32)
    rng = np.random.default_rng(1)
    batches = [("10^4 random dynamic bodies", np.sort(rng.choice(dynamic, min(10000, len(dynamic)), replace=False)).astype(np.int32)),
               ("every dynamic body", dynamic)]
    lines = ["%s settled %d steps: %d bodies, %d dynamic, %d awake" % (name, settle, nb, len(dynamic), int(((states["flags"] & 4) != 0).sum())),
             "ms, host clock around blocking calls, median [min .. max] of %d alternating rounds after a warm-up; steps through b2hip_step" % args.reps,
             "looped route = one single-body C call per body from Python (ctypes, arguments prepared), paid for at the next step's upload"]
    # ---- the two routes agree, per family and batch, on twin worlds ---------------------------------------------------------
    if a.body_states().tobytes() != b.body_states().tobytes():
        raise SystemExit("the twin worlds differ before anything was done")
    for family in FAMILIES:
        for label, bodies in batches:
            data = data_of(a, family, bodies, 3)
            batched(a, family, bodies, data)
            run_looped(looped(b, family, bodies, data))
            if a.body_states().tobytes() != b.body_states().tobytes():
                raise SystemExit("%s, %s: the two routes disagree right after the call" % (family, label))
            step(a)
            step(b)
            if a.body_states().tobytes() != b.body_states().tobytes():
                raise SystemExit("%s, %s: the two routes disagree after the next step" % (family, label))
    lines.append("the two routes agree on body_states() to the byte, right after the call and after the next step (3 families x 2 batches, twin worlds)")
    b.close()
    wb.close()
    # ---- timing, on one world ---------------------------------------------------------------------------------------------------
    for lazy in (0, 1):
        a.set_lazy_readback(bool(lazy))
        lines.append("---- read-back %s" % ("on demand (b2hip_set_lazy_readback)" if lazy else "with every step (the default)"))
        for family in FAMILIES if not lazy else FAMILIES[:1]:
            for label, bodies in batches:
                data = data_of(a, family, bodies, 5)
                calls = looped(a, family, bodies, data)
                ms = {"plain step": [], "looped: the calls": [], "looped: the next step": [], "batched: the call": [], "batched: the next step": []}

                def timed(key, fn):
                    t0 = time.perf_counter()
                    fn()
                    ms[key].append(1000.0 * (time.perf_counter() - t0))

                for rep in range(args.reps + 1):
                    timed("plain step", lambda: step(a))
                    timed("looped: the calls", lambda: run_looped(calls))
                    timed("looped: the next step", lambda: step(a))
                    timed("batched: the call", lambda: batched(a, family, bodies, data))
                    timed("batched: the next step", lambda: step(a))
                    if rep == 0:  # (the warm-up: arrays grown, code objects loaded)
                        for v in ms.values():
                            v.clear()
                lines.append("%s, %s: n = %d" % (family, label, len(bodies)))
                for k, v in ms.items():
                    lines.append("  %-28s %9.3f  [%9.3f .. %9.3f]" % (k, np.median(v), min(v), max(v)))
                lo = np.asarray(ms["looped: the calls"]) + np.asarray(ms["looped: the next step"])
                ba = np.asarray(ms["batched: the call"]) + np.asarray(ms["batched: the next step"])
                lines.append("  %-28s %9.3f  [%9.3f .. %9.3f]" % ("looped: write + step", np.median(lo), lo.min(), lo.max()))
                lines.append("  %-28s %9.3f  [%9.3f .. %9.3f]" % ("batched: write + step", np.median(ba), ba.min(), ba.max()))
    a.set_lazy_readback(False)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    a.close()
    wa.close()


if __name__ == "__main__":
    main()
