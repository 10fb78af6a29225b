"""The coloured large-island solvers EXECUTE their plan: replayed on the host, bit for bit.

The parity tests hold k_solve_blocks, k_blocks_sweep and the launch-per-colour kernels (k_large_warm, k_large_rest, k_rest_hub,
k_sweep_end, k_large_hub) to each other, tests/test_gpu_large_plan.py holds their plan to what it must be, and the float
bounds against the oracle in ANOTHER order are 1e-4 .. 8.5e-4 of the scene per step. A defect all forms share and that moves a
body by less than that - a row read stale, a lost hand-over, a warm start added in the wrong place, a hub row visited twice -
passes all of it. Here the oracle, whose arithmetic is the device's (bit-equal in reference order), is told to visit the
contacts in the order of the device's plan (tests/solve_order_ref.py: colour, then the place in the hub list; joints by id;
oracle/b2o.h: b2o_set_solve_order) and must then give the device's bits - every step of a default-mode trajectory:

    step the device; read its plan where plan_ref.py's docstring says it holds (behind b2hip_step, or between b2hip_solve and
    b2hip_sync_fixtures in a world with continuous physics); hand the order to the oracle; step the oracle;
    equal contact counts and equal raw words of position, angle, velocity, spin, centre, flags and sleep time of every body.

A step without large islands hands over an empty table (such steps are bit-exact anyway and keep the two in lockstep), so the
oracle follows persistent colours, incremental colouring, new partitions and adoption as they come. At the end of a case the
contact lists are compared as words too (ids, flags, manifolds, warm-start impulses). The hook's two error counts are 0 on
every step: it never guesses. Each case asserts from the counters and the plan record that it got where it is meant to go.

The default hub form (without B2HIP_HUB_SERIAL) is a fixed point settled to 2^-21 of the row, not a sequential sweep: it has
one test of its own with a measured bound (test_hub_fixed_point_against_the_replay); its integer results are exact.
"""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
import plan_ref as pr
import solve_order_ref as so
from test_gpu_large_plan import CCD, LAUNCHES, _lib, counters, reader, set_env
from test_solve_order_cpu import HookedOracle, contact_words

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
WORDS = ("x", "y", "angle", "vx", "vy", "spin", "cx", "cy", "flags", "sleep time")


def device_states(L, ptr):
    n = L.b2hip_body_count(ptr)
    out = np.zeros(n, b2hip.BODY_STATE_DTYPE)
    assert L.b2hip_get_body_states(ptr, 0, n, out.ctypes.data_as(C.c_void_p)) == 0, L.b2hip_last_error()
    return out.view(np.uint32).reshape(-1, 10)


def device_contacts(L, ptr):
    # (inside a step b2hip_contact_count is still the last step's: ask for room until the list is shorter than the room)
    cap = max(L.b2hip_contact_count(ptr), 1) + 16
    while True:
        out = np.zeros(cap, b2hip.CONTACT_DTYPE)
        n = L.b2hip_get_contacts(ptr, cap, out.ctypes.data_as(C.c_void_p))
        assert n >= 0, L.b2hip_last_error()
        if n < cap:
            return out[:n]
        cap *= 4


def capture(L, ptr):
    """(plan, contacts, body flags) of the solve that has just run; None if it had no large island."""
    ctr = counters(L, ptr)
    if ctr["large_islands"] == 0:
        return None
    read = reader(L, ptr)
    nb = L.b2hip_body_count(ptr)
    return pr.read_plan(read, nb, ctr), device_contacts(L, ptr), read(4, 0, nb, "u4")


class Seen:
    def __init__(self):
        self.steps = self.large_steps = self.rows = self.colours = self.hub_rows = self.joint_steps = self.spill_rows = self.islands = 0
        self.solvers = set()
        self.block_steps = self.sweep_steps = self.partitions = self.cut = self.rest_steps = self.fused = 0

    def note(self, plan, ctr):
        num = plan.numbers
        self.large_steps += 1
        self.rows = max(self.rows, plan.n_rows)
        self.solvers.add(num["solver"])
        colours = np.unique(plan.row_color)
        self.colours = max(self.colours, len(colours))
        is63 = plan.row_color == pr.HUB_COLOR
        self.hub_rows = max(self.hub_rows, int(is63.sum()))
        self.joint_steps += int(num["has_joints"] != 0)
        self.islands = max(self.islands, len(np.unique(plan.li_ref[:, 3])))
        self.cut = max(self.cut, ctr["cut_constraints"])
        self.rest_steps += int(num["use_rest"] != 0 and bool((plan.body_rest != 0).any()))
        self.fused += num["fuse_hub"]
        if is63.any():
            a, b = plan.li_ref[:, 1], plan.li_ref[:, 2]
            by_hub = ((a >= 0) & (plan.deg[np.maximum(a, 0)] > pr.HUB_DEGREE)) | ((b >= 0) & (plan.deg[np.maximum(b, 0)] > pr.HUB_DEGREE))
            orphan = num["serial_orphans"] and (((a >= 0) & (plan.eff_blk[np.maximum(a, 0)] == 0)) | ((b >= 0) & (plan.eff_blk[np.maximum(b, 0)] == 0)))
            self.spill_rows = max(self.spill_rows, int((is63 & ~by_hub & ~orphan).sum()))


def where_they_differ(label, step, dev, orc, got):
    """The first body whose words differ, and the rows on it in the plan."""
    bad = np.flatnonzero((dev != orc).any(axis=1))
    body = int(bad[0])
    words = [WORDS[k] for k in np.flatnonzero(dev[body] != orc[body])]
    msg = "%s, step %d: %d bodies differ; the first is body %d in %s\n  device %s\n  replay %s" % (
        label, step, len(bad), body, ", ".join(words), dev[body].view(np.float32)[:8].tolist(), orc[body].view(np.float32)[:8].tolist())
    if got is None:
        return msg + "\n  (a step without large islands)"
    plan = got[0]
    rank = so.row_ranks(plan)
    on = np.flatnonzero((plan.li_ref[:, 1] == body) | (plan.li_ref[:, 2] == body))
    rows = ["row %d: contact %d, bodies (%d, %d), colour %d, rank %d" % (r, plan.li_ref[r, 0], plan.li_ref[r, 1], plan.li_ref[r, 2], plan.row_color[r], rank[r])
            for r in on[np.argsort(rank[on], kind="stable")]]
    return msg + "\n  solver %d, %d rows, %d blocks, %d hub rows; its rows:\n    %s" % (
        plan.numbers["solver"], plan.n_rows, plan.numbers["blocks"], plan.numbers["hub_rows"], "\n    ".join(rows) or "(none)")


class Pair:
    """The device world and the oracle world of one scene, stepped in lockstep."""

    def __init__(self, amd, oracle, scene, kw):
        self.L = _lib()
        self.w = amd.world(scene, **kw)
        self.ptr = C.c_void_p(self.w.device_world())
        self.o = HookedOracle(oracle, scene, **kw)
        self.continuous = bool(kw.get("flags", bh.DEFAULT_FLAGS) & bh.F_CONTINUOUS)
        self.seen = Seen()
        self.orders = []

    def close(self):
        self.w.close()
        self.o.close()

    def device_step(self):
        """One step of the device; what capture() reads where the plan holds."""
        L, ptr = self.L, self.ptr
        if not self.continuous:
            self.w.step(1)
            return capture(L, ptr)
        # (no scene with continuous physics here has a script between its steps: the phases stand for the step)
        assert L.b2hip_step_begin(ptr, C.c_float(DT), self.w.vel_iters, self.w.pos_iters) == 0, L.b2hip_last_error()
        assert L.b2hip_collide(ptr) == 0 and L.b2hip_solve(ptr) == 0, L.b2hip_last_error()
        got = capture(L, ptr)
        for phase in (L.b2hip_sync_fixtures, L.b2hip_find_new_contacts, L.b2hip_solve_toi, L.b2hip_step_end):
            assert phase(ptr) == 0, L.b2hip_last_error()
        return got

    def step(self, label):
        got = self.device_step()
        self.seen.steps += 1
        if got is None:
            entries, large = np.zeros(0, so.ORDER_DTYPE), np.zeros(self.o.n_bodies, np.uint8)
        else:
            entries, large = so.solve_order(*got)
            self.seen.note(got[0], counters(self.L, self.ptr))
        self.orders.append((entries, large))
        self.o.set_order(entries, large)
        self.o.step()
        assert self.o.errors() == [0, 0], "%s, step %d: the hook could not follow the plan (contacts without rank, ranks without contact or partly flagged islands): %s" % (
            label, self.seen.steps, self.o.errors())
        dev, orc = device_states(self.L, self.ptr), self.o.states()
        assert dev.shape == orc.shape
        if not np.array_equal(dev, orc):
            pytest.fail(where_they_differ(label, self.seen.steps, dev, orc, got))
        nd, no = self.L.b2hip_contact_count(self.ptr), self.o.L.b2hip_contact_count(self.o.p)
        assert nd == no, "%s, step %d: %d contacts on the device, %d in the replay" % (label, self.seen.steps, nd, no)
        return got

    def contacts_equal(self, label):
        d, o = contact_words(device_contacts(self.L, self.ptr)), contact_words(self.o.contacts())
        assert d.shape == o.shape, "%s: %d contacts on the device, %d in the replay" % (label, len(d), len(o))
        bad = np.flatnonzero((d != o).any(axis=1))
        assert len(bad) == 0, "%s: %d contacts differ in ids, flags, manifold or impulses; the first: fixtures (%d, %d)" % (
            label, len(bad), d[bad[0], 0].view(np.int32) if len(bad) else -1, d[bad[0], 1].view(np.int32) if len(bad) else -1)


def replay(amd, oracle, monkeypatch, label, scene, steps, env, kw, most=True):
    set_env(monkeypatch, env)
    pair = Pair(amd, oracle, scene, kw)
    try:
        for _ in range(steps):
            pair.step(label)
        pair.contacts_equal(label)
        ctr = counters(pair.L, pair.ptr)
        pair.seen.block_steps, pair.seen.sweep_steps, pair.seen.partitions = ctr["block_solver_steps"], ctr["sweep_solver_steps"], ctr["partitions"]
    finally:
        pair.close()
        set_env(monkeypatch, {})
    s = pair.seen
    print("%s: %s" % (label, vars(s)))
    if most:
        assert s.large_steps > steps // 2, "%s: only %d of %d steps had a large island" % (label, s.large_steps, steps)
    assert s.large_steps > 0 and s.colours > 1, "%s: %d steps with large islands, %d colours in use" % (label, s.large_steps, s.colours)
    return s


def test_pyramid20_one_workgroup_of_k_solve_blocks(amd, oracle, monkeypatch):
    s = replay(amd, oracle, monkeypatch, "pyramid 20", bh.PYRAMID, 80, {}, dict(p0=20, p1=1, flags=CCD))
    # (the 210 boxes land on one another row by row: the island outgrows the reference-order tier at step 30)
    assert s.solvers == {pr.SOLVER_BLOCKS} and s.block_steps > 0 and s.islands == 1 and s.rows > 300, vars(s)


@pytest.mark.parametrize("env", [{}, LAUNCHES], ids=["k_solve_blocks", "launch per colour"])
def test_pyramid40_with_the_bench_flags(amd, oracle, monkeypatch, env):
    s = replay(amd, oracle, monkeypatch, "pyramid 40", bh.PYRAMID, 100, env, dict(p0=40, p1=1, flags=CCD))
    if not env:
        assert pr.SOLVER_BLOCKS in s.solvers and s.block_steps > 0 and s.cut > 0 and s.partitions > 0, vars(s)
    else:
        assert s.solvers == {pr.SOLVER_LAUNCHES} and s.block_steps == 0 and s.rest_steps > 0, vars(s)


TUMBLER_ENV = {"B2HIP_HUB_SERIAL": "1"}
# The 1 600 boxes of Tumbler 40 fall for 53 steps before the first of them reaches the container: the first large island is
# step 54's. The cases were asked for with 100 and 60 steps, of which 47 and 7 have a large island; they run 120 - the steps
# asked for and twenty / sixty more - so that most steps have one.
TUMBLER_STEPS = 120


@pytest.mark.parametrize("env", [TUMBLER_ENV, dict(TUMBLER_ENV, **LAUNCHES)], ids=["k_blocks_sweep", "launch per colour"])
def test_tumbler40_hub_rows_lane_after_lane_and_the_motor_joint(amd, oracle, monkeypatch, env):
    s = replay(amd, oracle, monkeypatch, "tumbler 40", bh.TUMBLER, TUMBLER_STEPS, env, dict(p0=40))
    assert s.hub_rows > pr.HUB_DEGREE and s.joint_steps > 0, vars(s)
    if "B2HIP_SOLVER_LAUNCHES" not in env:
        assert pr.SOLVER_SWEEP in s.solvers and s.sweep_steps > 0, vars(s)
    else:
        assert s.solvers == {pr.SOLVER_LAUNCHES} and s.sweep_steps == 0 and s.block_steps == 0, vars(s)
        assert s.rest_steps > 0 and s.fused > 0, "k_large_rest / k_rest_hub never ran: %s" % vars(s)


def test_tumbler40_rows_without_a_free_colour(amd, oracle, monkeypatch):
    s = replay(amd, oracle, monkeypatch, "tumbler 40, two colours per range", bh.TUMBLER, TUMBLER_STEPS, dict(TUMBLER_ENV, B2HIP_TEST_MAX_COLORS="2"), dict(p0=40))
    assert s.spill_rows > 0 and s.hub_rows > pr.HUB_DEGREE, vars(s)


def test_machines_joints_buried_in_one_island(amd, oracle, monkeypatch):
    # (the boxes bury the machines late: 160 steps, as
    # tests/test_gpu_large_plan.py runs the scene, where 120 were asked for and have none; 29 steps with a jointed large island)
    s = replay(amd, oracle, monkeypatch, "machines buried", bh.MACHINES, 160, {}, dict(p0=600, p1=6, seed=3), most=False)
    assert s.joint_steps > 0, "no large island owned a joint: %s" % vars(s)


def test_dense_field_large_islands_among_small_ones(amd, oracle, monkeypatch):
    s = replay(amd, oracle, monkeypatch, "dense field", bh.FIELD, 40, {}, dict(p0=800, p1=200, f0=50.0, f1=3.0, seed=29))
    assert s.block_steps > 0 and s.islands > 1 and s.cut > 0, vars(s)


def test_many_small_islands_in_the_coloured_table(amd, oracle, monkeypatch):
    s = replay(amd, oracle, monkeypatch, "field, every island large", bh.FIELD, 40, {"B2HIP_FORCE_LARGE": "1"}, dict(p0=800, p1=200, f0=50.0, f1=3.0, seed=29))
    assert s.islands > 10, vars(s)


# ---- the hub fixed point ---------------------------------------------------------------------------------------------------------
# Largest deviation of the default hub form (one fixed point over the hub's rows, settled to 2^-21 of the row) from the replay
# of its own plan after ONE step from the identical state, Tumbler 40, measured on an MI355X (absolute: metres, radians, m/s,
# rad/s; a box is 0.25 m wide). Steps 30 and 80 were asked for; at step 30 the boxes are still falling (the first large island
# is step 54's: that step is bit-equal, deviation 0), so step 60 - six steps after the first box has reached the container -
# is measured with them. The bound is 4 x the largest figure of the three (the number of rounds varies with the state).
FIXED_POINT_STEPS = (30, 60, 80)
#   step 31 (no large island yet)     position 0         angle 0   velocity 0          spin 0
#   step 61 (40 hub rows)             position 9.09e-13  angle 0   velocity 5.82e-11   spin 0
#   step 81 (51 hub rows)             position 1.82e-12  angle 0   velocity 3.64e-12   spin 0
# In both steps ONE body differs, body 1: the container, the hub itself, which is pinned with its origin at x = 0 - 9.09e-13 =
# 2^-40 and 5.82e-11 = 2^-34 are last bits of components of about 1e-5 and 1e-3. Every box is the replay's bit for bit, and so
# are the container's angle and spin: their bound is 0. The same figures came out of two runs on two machines.
FIXED_POINT_MEASURED = {"position": 1.8189894035458565e-12, "angle": 0.0, "velocity": 5.820766091346741e-11, "spin": 0.0}


def fixed_point_deviation(dev, orc):
    d, o = dev.view(np.float32), orc.view(np.float32)
    return {"position": float(np.abs(d[:, 0:2] - o[:, 0:2]).max()), "angle": float(np.abs(d[:, 2] - o[:, 2]).max()),
            "velocity": float(np.abs(d[:, 3:5] - o[:, 3:5]).max()), "spin": float(np.abs(d[:, 5] - o[:, 5]).max())}


def as_partition(labels):
    """Island labels as a set partition: every body carries the lowest body id of its island (-1: in none)."""
    labels = np.asarray(labels, np.int64)
    out = np.full(len(labels), -1, np.int64)
    lowest = {}
    for i, v in enumerate(labels.tolist()):
        if v >= 0:
            out[i] = lowest.setdefault(v, i)
    return out


def test_hub_fixed_point_against_the_replay(amd, oracle, monkeypatch):
    """Tumbler 40 followed bitwise (hub rows lane after lane) to steps 30, 60 and 80; at each the device world is saved and
    loaded WITHOUT B2HIP_HUB_SERIAL, stepped once, and compared with the oracle's replay of that world's own plan from the
    identical state. Integers - island labels, awake flags, the contact set - are exact; floats within 4 x the measured
    deviation (FIXED_POINT_MEASURED)."""
    kw = dict(p0=40)
    label = "tumbler 40 (fixed point)"
    set_env(monkeypatch, TUMBLER_ENV)
    main = Pair(amd, oracle, bh.TUMBLER, kw)
    # an oracle of its own for every stop but the last: it leaves the trajectory there
    twins = {stop: HookedOracle(oracle, bh.TUMBLER, **kw) for stop in FIXED_POINT_STEPS[:-1]}
    worst = dict.fromkeys(FIXED_POINT_MEASURED, 0.0)
    hub_steps = 0
    try:
        for stop in FIXED_POINT_STEPS:
            while main.seen.steps < stop:
                main.step(label)
                for at, twin in twins.items():
                    if at >= main.seen.steps:
                        twin.set_order(*main.orders[-1])
                        twin.step()
            orc = twins.get(stop, main.o)
            assert np.array_equal(device_states(main.L, main.ptr), orc.states())
            blob = b2hip.World.borrow(main.ptr.value).save_snapshot()
            set_env(monkeypatch, {})
            loaded = b2hip.World.from_snapshot(blob)
            set_env(monkeypatch, TUMBLER_ENV)
            try:
                loaded.step(DT, main.w.vel_iters, main.w.pos_iters)
                got = capture(main.L, loaded.p)
                if got is None:
                    orc.set_order(np.zeros(0, so.ORDER_DTYPE), np.zeros(orc.n_bodies, np.uint8))
                else:
                    num, ctr = got[0].numbers, counters(main.L, loaded.p)
                    assert num["hub_wide"] == 1 and num["hub_wide_rows"] > pr.HUB_DEGREE and ctr["hub_fixpoint_rounds"] > 0, (num, ctr)
                    hub_steps += 1
                    orc.set_order(*so.solve_order(*got))
                orc.L.b2hip_step(orc.p, C.c_float(DT), orc.w.vel_iters, orc.w.pos_iters)
                assert orc.errors() == [0, 0]
                dev, rep = device_states(main.L, loaded.p), orc.states()
                # integers: flags (type, awake ...), island labels, the contact set
                assert np.array_equal(dev[:, 8], rep[:, 8]), "flags differ at step %d" % (stop + 1)
                labels = np.zeros(len(dev), np.int32)
                assert main.L.b2hip_get_island_labels(loaded.p, len(dev), labels.ctypes.data_as(C.c_void_p)) == len(dev)
                assert np.array_equal(as_partition(labels), as_partition(orc.labels())), "island labels differ at step %d" % (stop + 1)
                dc, oc = device_contacts(main.L, loaded.p), orc.contacts()
                key = lambda c: sorted(zip(c["fixture_a"].tolist(), c["fixture_b"].tolist(), (c["flags"] & 3).tolist()))
                assert key(dc) == key(oc), "the contact sets differ at step %d" % (stop + 1)
                dv = fixed_point_deviation(dev, rep)
                differ = np.flatnonzero((dev != rep).any(axis=1))
                print("fixed point against the replay, step %d (%s): %s; bodies that differ: %s" % (
                    stop + 1, "no large island" if got is None else "%d hub rows" % got[0].numbers["hub_rows"], dv, differ[:8].tolist()))
                if got is None:
                    assert np.array_equal(dev, rep), "a step without large islands differs at step %d" % (stop + 1)
                for k in worst:
                    worst[k] = max(worst[k], dv[k])
            finally:
                loaded.close()
    finally:
        main.close()
        for twin in twins.values():
            twin.close()
        set_env(monkeypatch, {})
    print("fixed point against the replay, largest: %s" % worst)
    assert hub_steps >= 2, "the fixed point ran in %d of the %d steps" % (hub_steps, len(FIXED_POINT_STEPS))
    for k, m in FIXED_POINT_MEASURED.items():
        assert m is not None, "no measured figure recorded for %s (this run: %g)" % (k, worst[k])
        assert worst[k] <= 4.0 * m, "%s deviates by %g from the replay, measured %g (bound 4 x)" % (k, worst[k], m)
