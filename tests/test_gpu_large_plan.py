"""GPU tests of the PLAN of the large-island solve: after every step the device's colours, per-body masks, block partition,
row table and hub list are read back (b2hip_debug_read 12 - 21, 26 - 28) and held to what tests/plan_ref.py recomputes from
the world's own contact list, island labels and joints. The parity tests compare solvers that share one plan bit for bit; a
plan that is wrong for all of them alike - two rows of one colour on a body, a row in no group, a rest bit that is not set -
passes those and is named here. Every comparison is of integers and bit masks: exact, no tolerance.

Where the plan is read (plan_ref's docstring gives every array's window): behind the step in worlds without continuous
physics; between b2hip_solve and b2hip_sync_fixtures in worlds with it, where the TOI sub-steps change TOUCHING flags and use
hubList as scratch. Only steps with large islands are read. Each case also asserts that it reached the path it is here
for, from the counters and the plan record, so that none passes by not getting there.

Scene parameters are those of tests/test_gpu_sweep_end.py / test_gpu_recovery.py / the goldens. Changed against the list this
file was asked for: "one island in ONE workgroup of k_solve_blocks" is Pyramid 20, not 40 (Pyramid 40 has 2 400 constraints,
above 900 the host cuts 256-lane blocks: it stays as a case of a few blocks); B2HIP_TEST_MAX_COLORS / B2HIP_TEST_COLOR_ROUNDS run
on Tumbler 60 as asked AND on the recovery test's own scene, Pyramid 40, which is what reaches k_solve_blocks' second pass;
the machines are buried late, so 29 of their 160 steps have a large island (all of them checked).

What it found on the way (docs/SOLVER_LARGE_ISLANDS.md, "The plan's invariants"): Tumbler 60 with two colours per range laid
a row without a colour out by block after the census had counted it in its home block (row_set / static_encoding at step 23:
a stale row "between bodies 0 and 0" in the block's segment), and from 4 097 hub rows on the four-launch hub list left entries
unwritten (hub_list at step 78). Both fixed on the host side.

Wall time on an MI355X: every case under 2 s (the slowest: Tumbler 60 with two colours per range, 1.6 s; the others 0.05 -
0.5 s), the file about 5 s."""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
import plan_ref as pr
from test_gpu_sweep_end import two_hub_world

pytestmark = pytest.mark.gpu

KEYS = ("B2HIP_SOLVER_LAUNCHES", "B2HIP_NO_HUB_BUILD", "B2HIP_HUB_WIDE", "B2HIP_TEST_MAX_COLORS", "B2HIP_TEST_COLOR_ROUNDS", "B2HIP_FORCE_LARGE",
        "B2HIP_NO_REST", "B2HIP_NO_SWEEP_END", "B2HIP_HUB_SERIAL", "B2HIP_REST_ROWS", "B2HIP_REST_HUB", "B2HIP_NO_BLOCKS", "B2HIP_NO_SWEEP_BLOCKS",
        "B2HIP_HUB_ORDER", "B2HIP_NO_HUB_ORDER", "B2HIP_TEST_SPIN_MAX", "B2HIP_SMALL_MAX_W", "B2HIP_TRACE")
CCD = bh.F_SLEEP | bh.F_WARM | bh.F_CONTINUOUS
LAUNCHES = {"B2HIP_SOLVER_LAUNCHES": "1"}
DTYPES = {"i4": (np.int32, 1), "u4": (np.uint32, 1), "u8": (np.uint64, 1), "i4x4": (np.int32, 4)}


def _lib():
    L = b2hip.lib()
    L.b2hip_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.b2hip_debug_read.restype = C.c_int
    return L


def reader(L, ptr):
    def read(which, first, count, dtype):
        kind, width = DTYPES[dtype]
        out = np.zeros(max(count, 1) * width, kind)
        if count > 0:
            rc = L.b2hip_debug_read(ptr, which, first, count, out.ctypes.data_as(C.c_void_p))
            assert rc == 0, "b2hip_debug_read %d [%d, %d): %s" % (which, first, first + count, L.b2hip_last_error())
        return out[:count * width]
    return read


def counters(L, ptr):
    c = b2hip.Counters()
    assert L.b2hip_get_counters(ptr, C.byref(c)) == 0
    return {n: getattr(c, n) for n, _ in b2hip.Counters._fields_}


def capture(L, ptr):
    """(plan, world) of the solve that has just run, or None if it had no large island."""
    ctr = counters(L, ptr)
    if ctr["large_islands"] == 0:
        return None
    read = reader(L, ptr)
    nb = L.b2hip_body_count(ptr)
    plan = pr.read_plan(read, nb, ctr)
    # (inside a step b2hip_contact_count is still the last step's: ask for room until the list is shorter than the room)
    cap, n = max(L.b2hip_contact_count(ptr), 1) + 16, -1
    while True:
        contacts = np.zeros(cap, b2hip.CONTACT_DTYPE)
        n = L.b2hip_get_contacts(ptr, cap, contacts.ctypes.data_as(C.c_void_p))
        assert n >= 0, L.b2hip_last_error()
        if n < cap:
            break
        cap *= 4
    contacts = contacts[:n]
    labels = np.zeros(nb, np.int32)
    assert L.b2hip_get_island_labels(ptr, nb, labels.ctypes.data_as(C.c_void_p)) == nb
    world = pr.World(read(4, 0, nb, "u4"), labels, contacts["body_a"], contacts["body_b"], (contacts["flags"] & 3) == 3,
                     read(28, 0, plan.numbers["joints"], "i4x4").reshape(-1, 4))
    return plan, world


class Seen:
    """What the steps of a case reached (for the assertions that no case passes without getting where it is meant to go)."""

    def __init__(self):
        self.steps = self.checked = 0
        self.solvers = set()
        self.blocks = self.cut = self.hub_rows = self.colors = self.leftover = self.islands = self.joint_islands = 0
        self.partitions = []
        self.new_with_large = self.rest_steps = self.fused = self.hub_build = self.hub_lists = self.wide_steps = 0
        self.orphan_rows = self.spill_rows = self.hub_bodies = self.block_sorted = self.colour_sorted = 0
        self.recoveries = 0

    def note(self, plan, world, after):
        num = plan.numbers
        self.checked += 1
        self.solvers.add(num["solver"])
        self.blocks = max(self.blocks, plan.counters["blocks"])
        self.cut = max(self.cut, plan.counters["cut_constraints"])
        self.colors = max(self.colors, plan.counters["colors"])
        self.islands = max(self.islands, len(np.unique(plan.li_ref[:, 3])))
        self.partitions.append(after["partitions"])
        self.new_with_large += int(after["new_contacts"] > 0)
        self.recoveries = after["solver_recoveries"]
        self.block_sorted += num["block_sort"]
        self.colour_sorted += 1 - num["block_sort"]
        if num["solver"] == pr.SOLVER_EXACT:
            return
        is63 = plan.row_color == pr.HUB_COLOR
        if is63.any():
            self.hub_lists += 1
            self.hub_rows = max(self.hub_rows, int(is63.sum()))
            self.hub_build += num["hub_build_one"]
            self.wide_steps += int(num["hub_wide"] and num["hub_wide_rows"] > 0)
            self.leftover = max(self.leftover, int(is63.sum()) - num["hub_wide_rows"])
            a = np.where(plan.li_ref[:, 1] >= 0, plan.li_ref[:, 1], 0)
            b = np.where(plan.li_ref[:, 2] >= 0, plan.li_ref[:, 2], 0)
            by_hub = ((plan.li_ref[:, 1] >= 0) & (plan.deg[a] > pr.HUB_DEGREE)) | ((plan.li_ref[:, 2] >= 0) & (plan.deg[b] > pr.HUB_DEGREE))
            orphan = num["serial_orphans"] and (((plan.li_ref[:, 1] >= 0) & (plan.eff_blk[a] == 0)) | ((plan.li_ref[:, 2] >= 0) & (plan.eff_blk[b] == 0)))
            self.orphan_rows = max(self.orphan_rows, int((is63 & ~by_hub & orphan).sum()))
            self.spill_rows = max(self.spill_rows, int((is63 & ~by_hub & ~orphan).sum()))
        self.hub_bodies = max(self.hub_bodies, int((world.non_static & (plan.deg > pr.HUB_DEGREE)).sum()))
        if num["use_rest"] and (plan.body_rest != 0).any():
            self.rest_steps += 1
        self.fused += num["fuse_hub"]
        if num["has_joints"]:
            self.joint_islands += 1


def set_env(monkeypatch, env):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run_steps(L, ptr, steps, step, continuous, seen, label):
    """`steps` steps of the world at `ptr`, the plan of each checked. `step()`: one whole step (worlds without continuous
    physics: the plan is read behind it); with continuous physics the phases are called here and the plan is read behind the
    solve."""
    for _ in range(steps):
        got = None
        if continuous:
            assert L.b2hip_step_begin(ptr, 1.0 / 60.0, 8, 3) == 0, L.b2hip_last_error()
            assert L.b2hip_collide(ptr) == 0 and L.b2hip_solve(ptr) == 0, L.b2hip_last_error()
            got = capture(L, ptr)
            for phase in (L.b2hip_sync_fixtures, L.b2hip_find_new_contacts, L.b2hip_solve_toi, L.b2hip_step_end):
                assert phase(ptr) == 0, L.b2hip_last_error()
        else:
            step()
            got = capture(L, ptr)
        seen.steps += 1
        if got is None:
            continue
        plan, world = got
        found = pr.check_plan(plan, world)
        assert not found, "%s, step %d (solver %d, %d rows, %d blocks, %d hub rows):\n%s" % (
            label, seen.steps, plan.numbers["solver"], plan.n_rows, plan.numbers["blocks"], plan.numbers["hub_rows"], pr.format_violations(found))
        seen.note(plan, world, counters(L, ptr))


def run_scene(amd, monkeypatch, label, scene, steps, env, kw, min_checked=None):
    set_env(monkeypatch, env)
    L = _lib()
    w = amd.world(scene, **kw)
    ptr = C.c_void_p(w.device_world())
    seen = Seen()
    try:
        run_steps(L, ptr, steps, lambda: w.step(1), bool(kw.get("flags", bh.DEFAULT_FLAGS) & bh.F_CONTINUOUS), seen, label)
    finally:
        w.close()
        set_env(monkeypatch, {})
    run_scene.last = seen
    assert seen.checked >= (steps // 2 if min_checked is None else min_checked), "%s: only %d of %d steps had a large island" % (label, seen.checked, steps)
    return seen


def test_pyramid20_is_one_island_in_one_workgroup(amd, monkeypatch):
    """(Pyramid 40 has 2 400 constraints: above 900 the host cuts 256-lane blocks. A 20-row pyramid - 210 boxes, 400 constraints -
    is what runs k_solve_blocks as ONE workgroup of 1024 lanes.)"""
    s = run_scene(amd, monkeypatch, "pyramid 20", bh.PYRAMID, 60, {}, dict(p0=20, p1=1, flags=CCD))
    assert pr.SOLVER_BLOCKS in s.solvers and s.blocks == 1 and s.cut == 0 and s.islands == 1 and s.block_sorted > 0, vars(s)


def test_pyramid40_a_few_blocks(amd, monkeypatch):
    s = run_scene(amd, monkeypatch, "pyramid 40", bh.PYRAMID, 60, {}, dict(p0=40, p1=1, flags=CCD))
    assert pr.SOLVER_BLOCKS in s.solvers and s.blocks > 1 and s.cut > 0 and s.islands == 1 and s.block_sorted > 0, vars(s)


def test_pyramid90_blocks_cut_rows_and_new_partitions(amd, monkeypatch):
    s = run_scene(amd, monkeypatch, "pyramid 90", bh.PYRAMID, 150, {}, dict(p0=90, p1=1, flags=CCD))
    assert pr.SOLVER_BLOCKS in s.solvers and s.blocks > 1 and s.cut > 0, vars(s)
    assert s.partitions[-1] > s.partitions[0], "no partition was made again: %s" % s.partitions
    assert s.new_with_large > 0, "no step brought new contacts"


TUMBLER = [("k_blocks_sweep", {}), ("launch per colour", LAUNCHES), ("launch per colour, hub list by four launches", dict(LAUNCHES, B2HIP_NO_HUB_BUILD="1")),
           ("launch per colour, four launches, hub rows in contact order", dict(LAUNCHES, B2HIP_NO_HUB_BUILD="1", B2HIP_HUB_WIDE="0"))]


@pytest.mark.parametrize("case", TUMBLER, ids=[c[0] for c in TUMBLER])
def test_tumbler60_hub_joint_and_a_growing_pile(amd, monkeypatch, case):
    name, env = case
    s = run_scene(amd, monkeypatch, "tumbler 60, " + name, bh.TUMBLER, 120, env, dict(p0=60))
    assert s.hub_rows > 30 and s.hub_bodies >= 1 and s.joint_islands > 0 and s.new_with_large > 0 and s.hub_lists > 0, vars(s)
    if not env:
        assert pr.SOLVER_SWEEP in s.solvers and s.blocks > 1 and s.cut > 0 and s.orphan_rows > 0, vars(s)
    else:
        assert s.solvers == {pr.SOLVER_LAUNCHES} and s.block_sorted == 0, vars(s)
        assert s.rest_steps > 0, "no step had rest colours noted on its bodies"
        assert (s.hub_build > 0) == ("B2HIP_NO_HUB_BUILD" not in env), vars(s)
        assert (s.wide_steps > 0) == (env.get("B2HIP_HUB_WIDE") != "0"), vars(s)
        if "B2HIP_NO_HUB_BUILD" not in env:
            assert s.fused > 0, "k_rest_hub was never planned"


@pytest.mark.parametrize("env", [{}, LAUNCHES], ids=["k_blocks_sweep", "launch per colour"])
def test_machines_buried_joints_in_the_island(amd, monkeypatch, env):
    # (the boxes bury the machines late: the last thirty of the 160 steps have an island beyond the in-LDS solver)
    s = run_scene(amd, monkeypatch, "machines buried", bh.MACHINES, 160, env, dict(p0=600, p1=6, seed=3), min_checked=20)
    assert s.joint_islands > 0, vars(s)
    if not env:
        assert pr.SOLVER_SWEEP in s.solvers and s.orphan_rows > 0, vars(s)
    else:
        assert s.solvers == {pr.SOLVER_LAUNCHES}, vars(s)


def test_two_hubs_and_leftover_hub_rows(monkeypatch):
    L = _lib()
    w = two_hub_world(monkeypatch, LAUNCHES)
    seen = Seen()
    try:
        run_steps(L, w.p, 60, w.step, False, seen, "two hubs")
    finally:
        w.close()
        set_env(monkeypatch, {})
    assert seen.checked == 60 and seen.hub_bodies == 2 and seen.hub_rows > 80 and seen.leftover > 32 and seen.wide_steps > 0, vars(seen)


RUNS_OUT = [("tumbler 60, two colours per range", bh.TUMBLER, 120, {"B2HIP_TEST_MAX_COLORS": "2"}, dict(p0=60)),
            ("tumbler 60, one round of k_color_small", bh.TUMBLER, 120, {"B2HIP_TEST_COLOR_ROUNDS": "1"}, dict(p0=60)),
            ("pyramid 40, two colours per range", bh.PYRAMID, 120, {"B2HIP_TEST_MAX_COLORS": "2"}, dict(p0=40, p1=1, flags=CCD)),
            ("pyramid 40, one round of k_color_small", bh.PYRAMID, 120, {"B2HIP_TEST_COLOR_ROUNDS": "1"}, dict(p0=40, p1=1, flags=CCD))]


@pytest.mark.parametrize("case", RUNS_OUT, ids=[c[0] for c in RUNS_OUT])
def test_colouring_that_runs_out(amd, monkeypatch, case):
    name, scene, steps, env, kw = case
    s = run_scene(amd, monkeypatch, name, scene, steps, env, kw)
    assert s.recoveries > 0, "%s: never happened" % name
    if "B2HIP_TEST_MAX_COLORS" in env:
        assert s.spill_rows > 0, "no row without a free colour was in the hub group"


def test_many_small_islands_in_one_table(amd, monkeypatch):
    s = run_scene(amd, monkeypatch, "piles, every island large", bh.PILES, 60, {"B2HIP_FORCE_LARGE": "1"}, dict(p0=40, p1=5, seed=7))
    assert s.islands > 10, vars(s)


def test_exact_order_levels_as_colours(amd, monkeypatch):
    s = run_scene(amd, monkeypatch, "pyramid 20 in exact order", bh.PYRAMID, 40, {"B2HIP_FORCE_LARGE": "2"}, dict(p0=20, p1=1, flags=CCD))
    assert s.solvers == {pr.SOLVER_EXACT} and s.colors > 64, vars(s)


def test_the_plan_of_a_loaded_world(amd, monkeypatch):
    """Tumbler 60: snapshot at step 60, loaded, 20 more steps - the colours and the solver's hints travel in the snapshot."""
    set_env(monkeypatch, {})
    L = _lib()
    w = amd.world(bh.TUMBLER, p0=60)
    ptr = C.c_void_p(w.device_world())
    first, second = Seen(), Seen()
    try:
        run_steps(L, ptr, 60, lambda: w.step(1), False, first, "tumbler 60 before the snapshot")
        blob = b2hip.World.borrow(ptr.value).save_snapshot()
    finally:
        w.close()
    loaded = b2hip.World.from_snapshot(blob)
    try:
        run_steps(L, loaded.p, 20, loaded.step, False, second, "tumbler 60 loaded")
    finally:
        loaded.close()
    assert second.checked == 20 and second.hub_rows > 30 and second.joint_islands > 0 and pr.SOLVER_SWEEP in second.solvers, vars(second)
    # the loaded world goes on with the partition it was saved with
    assert second.partitions[0] >= first.partitions[-1] and second.blocks > 1, (first.partitions[-1], second.partitions[:3])
