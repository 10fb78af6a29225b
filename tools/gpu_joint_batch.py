"""Batched joint motor targets and joint state reads on the device (include/b2hip.h, block G: b2hip_joint_set_motors,
b2hip_get_joint_states) against the routes a caller had before, in the same run: one b2hip_joint_set_motor per joint, and one
b2hip_get_joint_reaction + one b2hip_get_joint_limit_state per joint.

  python tools/gpu_joint_batch.py [--out FILE] [--reps N] [--arms N]

The scene: a field of 10^4 two-link arms, each pinned to a static anchor body: two motorised revolute joints with limits per
arm, 2 x 10^4 joints, nothing collides, sleep is off. The single-joint setter edits the host's copy and pays at the next
step's upload, so what is timed for the writes is "new motor speeds on all joints + the next step" for both routes, beside a
plain step, through the C ABI. --reps rounds alternate plain step, looped write, batched write, looped read, batched read on
ONE world (other work shares the host: the spread is printed beside the median); the looped calls are made from Python through
ctypes with their arguments prepared beforehand, and the loop's own time is printed apart from the step's so that the
interpreter's share can be seen. Every write gives every joint a speed it does not have yet, so no entry is dropped as
unchanged. Before anything is timed the two routes are run on twin worlds - built alike - and must agree to the byte:
body_states() right after the writes and after the next step, and the batched read with the looped reads.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "box2d-mt_amd", "python"))

import b2hip  # noqa: E402

MAX_TORQUE = 50.0
INV_DT = 60.0


def build(arms):
    """the field: arm k hangs from (3 (k % 100), 3 (k // 100)); returns (world, joint ids)"""
    w = b2hip.World(allow_sleep=False)
    anchor = w.create_body(b2hip.STATIC, (0.0, 0.0))
    link = b2hip.box_shape(0.05, 0.25)
    joints = []
    for k in range(arms):
        x, y = 3.0 * (k % 100), 3.0 * (k // 100)
        upper = w.create_body(b2hip.DYNAMIC, (x, y - 0.25))
        lower = w.create_body(b2hip.DYNAMIC, (x, y - 0.75))
        for b in (upper, lower):
            w.create_fixture(b, link, density=1.0, category=2, mask=0)
        joints.append(w.create_revolute_joint(anchor, upper, (x, y), (0.0, 0.25), 0.0, True, -1.0, 1.0, True, 0.2, MAX_TORQUE))
        joints.append(w.create_revolute_joint(upper, lower, (0.0, -0.25), (0.0, 0.25), 0.0, True, -1.0, 1.0, True, -0.2, MAX_TORQUE))
    return w, np.asarray(joints, np.int32)


def looped_write(w, joints, speeds):
    L, p = w.L, w.p
    return [(L.b2hip_joint_set_motor, (p, j, 1, s, MAX_TORQUE)) for j, s in zip(joints.tolist(), speeds.tolist())]


def run(calls):
    for fn, a in calls:
        if fn(*a) < 0:
            raise SystemExit("a single-joint call failed")


def looped_read(w, joints):
    """(calls, where the answers land): reaction (4 floats) and limit state per joint"""
    L, p = w.L, w.p
    out = np.zeros((len(joints), 4), np.float32)
    ptr = C.POINTER(C.c_float)
    calls = []
    for i, j in enumerate(joints.tolist()):
        calls.append((L.b2hip_get_joint_reaction, (p, j, INV_DT, out[i].ctypes.data_as(ptr))))
        calls.append((L.b2hip_get_joint_limit_state, (p, j)))
    return calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_batch_arms.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--arms", type=int, default=10000)
    args = ap.parse_args()
    b2hip.use_torch_hip_runtime()
    a, joints = build(args.arms)
    b, _ = build(args.arms)
    n = len(joints)
    for _ in range(30):
        a.step()
        b.step()
    rng = np.random.default_rng(1)
    speeds = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for _ in range(4)]
    lines = ["%d two-link arms on a static anchor body: %d bodies, %d motorised revolute joints with limits, sleep off, 30 steps in"
             % (args.arms, a.body_count, n),
             "ms, host clock around blocking calls, median [min .. max] of %d alternating rounds after a warm-up; steps through b2hip_step" % args.reps,
             "looped routes = one single-joint C call per joint from Python (ctypes, arguments prepared); a looped write is paid for at the next step's upload"]
    # ---- the routes agree, on twin worlds ------------------------------------------------------------------------------------
    if a.body_states().tobytes() != b.body_states().tobytes():
        raise SystemExit("the twin worlds differ before anything was done")
    a.joint_set_motors(joints, speed=speeds[0])
    run(looped_write(b, joints, speeds[0]))
    if a.body_states().tobytes() != b.body_states().tobytes():
        raise SystemExit("the two write routes disagree right after the call")
    a.step()
    b.step()
    if a.body_states().tobytes() != b.body_states().tobytes():
        raise SystemExit("the two write routes disagree after the next step")
    got = a.joint_states(joints, INV_DT)
    calls, out = looped_read(b, joints)
    states = [fn(*args_) for fn, args_ in calls][1::2]
    want = np.stack([got["force"][:, 0], got["force"][:, 1], got["torque"], got["motor"]], axis=1)
    if want.tobytes() != out.tobytes() or got["limit_state"].tolist() != states:
        raise SystemExit("the batched read disagrees with the single-joint reads")
    if a.joint_states(joints, INV_DT).tobytes() != b.joint_states(joints, INV_DT).tobytes():
        raise SystemExit("the twin worlds disagree on joint_states()")
    lines.append("the routes agree to the byte on twin worlds: body_states() right after the writes and after the next step, "
                 "joint_states() with the single-joint reads (%d joints with a motor impulse, %d at a limit)"
                 % (int((got["motor"] != 0.0).sum()), int((got["limit_state"] != 0).sum())))
    b.close()
    # ---- timing, on one world ------------------------------------------------------------------------------------------------
    for lazy in (0, 1):
        a.set_lazy_readback(bool(lazy))
        lines.append("---- read-back %s" % ("on demand (b2hip_set_lazy_readback)" if lazy else "with every step (the default)"))
        read_calls, sink = looped_read(a, joints)  # (sink: where the looped reads write, kept alive with the calls)
        ms = {"plain step": [], "looped write: the calls": [], "looped write: the next step": [], "batched write: the call": [],
              "batched write: the next step": [], "looped read": [], "batched read": []}

        def timed(key, fn):
            t0 = time.perf_counter()
            fn()
            ms[key].append(1000.0 * (time.perf_counter() - t0))

        for rep in range(args.reps + 1):
            write_calls = looped_write(a, joints, speeds[(2 * rep + 1) % 4])
            batch_speeds = speeds[(2 * rep + 2) % 4]
            timed("plain step", a.step)
            timed("looped write: the calls", lambda: run(write_calls))
            timed("looped write: the next step", a.step)
            timed("batched write: the call", lambda: a.joint_set_motors(joints, speed=batch_speeds))
            timed("batched write: the next step", a.step)
            timed("looped read", lambda: run(read_calls))
            timed("batched read", lambda: a.joint_states(joints, INV_DT))
            if rep == 0:  # (the warm-up: arrays grown, code objects loaded)
                for v in ms.values():
                    v.clear()
        lines.append("all joints: n = %d" % n)
        for k, v in ms.items():
            lines.append("  %-30s %9.3f  [%9.3f .. %9.3f]" % (k, np.median(v), min(v), max(v)))
        lo = np.asarray(ms["looped write: the calls"]) + np.asarray(ms["looped write: the next step"])
        ba = np.asarray(ms["batched write: the call"]) + np.asarray(ms["batched write: the next step"])
        lines.append("  %-30s %9.3f  [%9.3f .. %9.3f]" % ("looped: write + step", np.median(lo), lo.min(), lo.max()))
        lines.append("  %-30s %9.3f  [%9.3f .. %9.3f]" % ("batched: write + step", np.median(ba), ba.min(), ba.max()))
    a.set_lazy_readback(False)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    a.close()


if __name__ == "__main__":
    main()
