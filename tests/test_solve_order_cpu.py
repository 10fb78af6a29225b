"""The oracle's solve order hook (oracle/b2o.h: b2o_set_solve_order) on the oracle alone: no GPU.

tests/test_gpu_solve_replay.py hands the hook the order of the device's large-island plan and requires the device's bits. That
rests on three things, checked here on a 20-row pyramid (210 boxes, one island of ~400 contacts) and a pile with joints:

  * the hook is the identity where it must be: ranks equal to each contact's place in the reference's own order (recorded from
    an unhooked twin, b2o_record_solve_order) reproduce the unhooked oracle bit for bit, joints left in DFS order;
  * the order INSIDE a colour cannot be observed: with a greedy colouring made here (no moving body in two rows of a colour; a
    body of more than 30 rows makes its rows the hub group, swept in contact order behind the colours) ranks shuffled within
    each colour by three seeds give identical bits on every step - and bits that differ from the reference order's;
  * it refuses to guess: a contact without rank, a rank without contact and a partly flagged island are counted.
"""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
import plan_ref as pr
import solve_order_ref as so
from solve_order_ref import ORDER_DTYPE

DT = 1.0 / 60.0
BF_AWAKE = 0x4
HUB_DEGREE = 30
HUB_RANK = 63
SETTLE = 50  # steps until the 20-row pyramid has landed on itself: one island of more than 300 contacts


class HookedOracle:
    """An oracle world of the scene harness, driven through the ABI shim's entry points, with the order hook."""

    def __init__(self, oracle, scene, **kw):
        self.w = oracle.world(scene, **kw)
        self.L = oracle.lib
        self.p = C.c_void_p(self.w.device_world())
        assert self.p.value, "the oracle harness has no world behind its b2World"

    def close(self):
        self.w.close()

    @property
    def n_bodies(self):
        return self.L.b2hip_body_count(self.p)

    def step(self):
        """One step through the drop-in b2World (the scene's own per-step script included)."""
        self.w.step(1)

    def step_to_solve(self):
        """The phases of a step up to the island solve: behind it contacts() is the list the solve will see."""
        self.L.b2hip_step_begin(self.p, C.c_float(DT), self.w.vel_iters, self.w.pos_iters)
        self.L.b2hip_collide(self.p)

    def step_from_solve(self):
        for phase in (self.L.b2hip_solve, self.L.b2hip_sync_fixtures, self.L.b2hip_find_new_contacts, self.L.b2hip_solve_toi, self.L.b2hip_step_end):
            phase(self.p)

    def states(self):
        """[bodies, 10] raw words: position, angle, velocity, spin, centre, flags, sleep time."""
        out = np.zeros(self.n_bodies, b2hip.BODY_STATE_DTYPE)
        self.L.b2hip_get_body_states(self.p, 0, self.n_bodies, out.ctypes.data_as(C.c_void_p))
        return out.view(np.uint32).reshape(-1, 10)

    def contacts(self):
        cap = max(self.L.b2hip_contact_count(self.p), 1)
        out = np.zeros(cap, b2hip.CONTACT_DTYPE)
        n = self.L.b2hip_get_contacts(self.p, cap, out.ctypes.data_as(C.c_void_p))
        return out[:n]

    def labels(self):
        out = np.zeros(self.n_bodies, np.int32)
        self.L.b2hip_get_island_labels(self.p, self.n_bodies, out.ctypes.data_as(C.c_void_p))
        return out

    def set_order(self, entries, large, joints_by_id=True):
        entries = np.ascontiguousarray(entries, ORDER_DTYPE)
        large = np.ascontiguousarray(large, np.uint8)
        self.L.b2o_shim_set_solve_order(self.p, len(entries), entries.ctypes.data_as(C.c_void_p), len(large), large.ctypes.data_as(C.c_void_p), int(joints_by_id))

    def errors(self):
        out = np.zeros(2, np.int32)
        self.L.b2o_shim_get_solve_order_errors(self.p, out.ctypes.data_as(C.c_void_p))
        return out.tolist()

    def record(self, enable=True):
        self.L.b2o_shim_record_solve_order(self.p, int(enable))

    def recorded(self):
        n = self.L.b2o_shim_get_recorded_solve_order(self.p, 0, None)
        out = np.zeros(max(n, 1), ORDER_DTYPE)
        self.L.b2o_shim_get_recorded_solve_order(self.p, n, out.ctypes.data_as(C.c_void_p))
        return out[:n]


def contact_words(c):
    """A contact list as raw words, sorted by its fixture ids (ids, flags, manifold, warm-start impulses, material)."""
    order = np.lexsort((c["fixture_b"], c["fixture_a"]))
    return np.ascontiguousarray(c[order]).view(np.uint32).reshape(len(c), -1)


PILES = [("pyramid 20", bh.PYRAMID, dict(p0=20, p1=1)), ("machines under boxes", bh.MACHINES, dict(p0=120, p1=4, seed=3))]


@pytest.mark.parametrize("case", PILES, ids=[c[0] for c in PILES])
def test_ranks_of_the_reference_order_change_nothing(oracle, case):
    _, scene, kw = case
    plain, hooked = HookedOracle(oracle, scene, **kw), HookedOracle(oracle, scene, **kw)
    try:
        plain.record()
        ranked = reordered = 0
        for step in range(60):
            plain.step()
            rec = plain.recorded()
            # handed over in another order than visited: the hook has to sort
            hooked.set_order(rec[::-1], plain.labels() >= 0, joints_by_id=False)
            hooked.step()
            assert hooked.errors() == [0, 0], "step %d" % step
            assert np.array_equal(plain.states(), hooked.states()), "step %d" % step
            ranked += len(rec)
            reordered += int(len(rec) > 1)
        assert np.array_equal(contact_words(plain.contacts()), contact_words(hooked.contacts()))
        assert ranked > 1000 and reordered > 30, (ranked, reordered)
    finally:
        plain.close()
        hooked.close()


def coloured_order(contacts, states, rng=None):
    """(entries, large, colours in use) for the contact list the solve is about to see: islands by union-find over the solid
    contacts (an island is solved when one of its bodies is awake), greedy colours in contact order, the rows of a body with
    more than 30 rows as the hub group in contact order. `rng`: the ranks of a colour are a random permutation of its rows."""
    n = len(states)
    moving = (states[:, 8] & 3) != 0
    awake = (states[:, 8] & BF_AWAKE) != 0
    solid = (contacts["flags"] & 3) == 3
    a, b = contacts["body_a"].astype(np.int64), contacts["body_b"].astype(np.int64)
    live = solid & (moving[a] | moving[b])
    parent = np.arange(n)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in np.flatnonzero(live & moving[a] & moving[b]):
        ra, rb = find(a[i]), find(b[i])
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) for i in range(n)])
    solved = np.zeros(n, bool)
    solved[root[moving & awake]] = True
    first = np.where(moving[a], a, b)
    rows = np.flatnonzero(live & solved[root[first]])
    large = moving & solved[root]
    deg = np.bincount(a[rows][moving[a[rows]]], minlength=n) + np.bincount(b[rows][moving[b[rows]]], minlength=n)
    used = np.zeros(n, np.uint64)
    colour = np.zeros(len(rows), np.int64)
    for k, i in enumerate(rows):
        ends = [q for q in (a[i], b[i]) if moving[q]]
        if any(deg[q] > HUB_DEGREE for q in ends):
            colour[k] = HUB_RANK
            continue
        taken = 0
        for q in ends:
            taken |= int(used[q])
        c = 0
        while taken >> c & 1:
            c += 1
        assert c < HUB_RANK
        colour[k] = c
        for q in ends:
            used[q] |= np.uint64(1 << c)
    entries = np.zeros(len(rows), ORDER_DTYPE)
    entries["fixture_a"], entries["fixture_b"] = contacts["fixture_a"][rows], contacts["fixture_b"][rows]
    place = np.zeros(len(rows), np.int64)
    for c in np.unique(colour):
        of = np.flatnonzero(colour == c)
        place[of] = np.arange(len(of)) if (rng is None or c == HUB_RANK) else rng.permutation(len(of))
    entries["rank"] = colour * (len(rows) + 1) + place
    return entries, large.astype(np.uint8), len(np.unique(colour))


def coloured_run(oracle, scene, kw, steps, seed):
    w = HookedOracle(oracle, scene, **kw)
    rng = None if seed is None else np.random.default_rng(seed)
    try:
        out, colours = [], 0
        for step in range(steps):
            w.step_to_solve()
            entries, large, nc = coloured_order(w.contacts(), w.states(), rng)
            colours = max(colours, nc)
            w.set_order(entries, large)
            w.step_from_solve()
            assert w.errors() == [0, 0], "step %d" % step
            out.append(w.states().copy())
        return out, contact_words(w.contacts()), colours
    finally:
        w.close()


def test_the_order_inside_a_colour_cannot_be_observed(oracle):
    kw = dict(p0=20, p1=1)
    runs = [coloured_run(oracle, bh.PYRAMID, kw, 60, seed) for seed in (None, 1, 2, 3)]
    base, base_contacts, colours = runs[0]
    assert colours > 4, "the pile was coloured with %d colours" % colours
    for states, contacts, _ in runs[1:]:
        for step, (x, y) in enumerate(zip(base, states)):
            assert np.array_equal(x, y), "step %d" % step
        assert np.array_equal(base_contacts, contacts)
    # ... and the colours are another sweep than the reference's: not vacuous
    plain = HookedOracle(oracle, bh.PYRAMID, **kw)
    try:
        for _ in range(60):
            plain.step()
        assert not np.array_equal(plain.states(), base[59]), "the coloured order gave the reference order's bits"
    finally:
        plain.close()


def test_the_hook_is_used_once(oracle):
    kw = dict(p0=20, p1=1)
    plain, hooked = HookedOracle(oracle, bh.PYRAMID, **kw), HookedOracle(oracle, bh.PYRAMID, **kw)
    try:
        plain.record()
        for _ in range(SETTLE):
            plain.step()
            hooked.step()
        plain.step()
        assert len(plain.recorded()) > 300
        hooked.set_order(plain.recorded(), plain.labels() >= 0)
        hooked.step()
        for step in range(5):  # no order set again: the reference's
            plain.step()
            hooked.step()
            assert hooked.errors() == [0, 0]
            assert np.array_equal(plain.states(), hooked.states()), "step %d" % step
    finally:
        plain.close()
        hooked.close()


def test_it_refuses_to_guess(oracle):
    kw = dict(p0=20, p1=1)
    twin, w = HookedOracle(oracle, bh.PYRAMID, **kw), HookedOracle(oracle, bh.PYRAMID, **kw)
    try:
        twin.record()

        def next_order():
            twin.step()
            return twin.recorded(), (twin.labels() >= 0).astype(np.uint8)

        def lockstep():
            # (whatever the hook was handed, the two stay the same world only while the order is the reference's: asserted)
            assert np.array_equal(twin.states(), w.states())

        for _ in range(SETTLE):
            twin.step()
            w.step()
        rec, large = next_order()
        assert len(rec) > 300 and large.sum() == 210
        w.set_order(rec[1:], large, joints_by_id=False)  # one rank missing
        w.step()
        assert w.errors() == [1, 0]
        twin.close()
        w.close()

        twin, w = HookedOracle(oracle, bh.PYRAMID, **kw), HookedOracle(oracle, bh.PYRAMID, **kw)
        twin.record()
        for _ in range(SETTLE):
            twin.step()
            w.step()
        rec, large = next_order()
        bogus = np.zeros(1, ORDER_DTYPE)
        bogus["fixture_a"], bogus["fixture_b"], bogus["rank"] = 100000, 100001, 5
        w.set_order(np.concatenate([rec, bogus]), large, joints_by_id=False)  # a ranked contact that does not exist
        w.step()
        assert w.errors() == [0, 1]
        lockstep()

        rec, large = next_order()
        part = large.copy()
        part[np.flatnonzero(large)[0]] = 0
        w.set_order(np.zeros(0, ORDER_DTYPE), part, joints_by_id=False)  # a partly flagged island: counted, the reference's order kept
        w.step()
        assert w.errors() == [0, 1]
        lockstep()

        rec, large = next_order()
        w.set_order(rec, part, joints_by_id=False)  # ... and its ranked contacts are ranks nothing took
        w.step()
        assert w.errors() == [0, 1 + len(rec)]
        lockstep()
    finally:
        twin.close()
        w.close()


def test_ranks_from_a_plan():
    """solve_order_ref on a hand-made plan: colour, then the place in the hub list; contacts named by their fixtures; a plan
    that does not describe the contact list is refused."""
    contacts = np.zeros(5, b2hip.CONTACT_DTYPE)
    contacts["fixture_a"], contacts["fixture_b"] = [10, 11, 12, 13, 14], [20, 21, 22, 23, 24]
    contacts["body_a"], contacts["body_b"] = [1, 2, 0, 1, 3], [2, 3, 1, 3, 4]
    num = dict.fromkeys(pr.PLAN_FIELDS, 0)
    num.update(solver=pr.SOLVER_LAUNCHES, hub_rows=2)
    z = np.zeros(5, np.int64)

    def plan(li_ref, colours, hub_list, **over):
        return pr.Plan(dict(num, **over), {"large_island_contacts": len(li_ref)}, li_ref=np.array(li_ref), row_color=np.array(colours), deg=z,
                       body_color_mask=z, body_active=z, body_rest=z, b_blk1=z, eff_blk=z, blk_row_start=z, census=z, hub_list=np.array(hub_list))

    flags = np.array([pr.BT_STATIC, 2 | pr.BF_LARGE, 2 | pr.BF_LARGE, 2 | pr.BF_LARGE, 2], np.uint32)
    # rows: contact 3 (colour 63, second in the hub list), contact 0 (colour 1), contact 2 (body 0 static: -(0 + 1)), contact 1 (63, first)
    rows = [[3, 1, 3, 1], [0, 1, 2, 1], [2, -1, 1, 1], [1, 2, 3, 1]]
    entries, large = so.solve_order(plan(rows, [63, 1, 0, 63], [3, 0]), contacts, flags)
    assert large.tolist() == [0, 1, 1, 1, 0]
    assert entries["fixture_a"].tolist() == [13, 10, 12, 11] and entries["fixture_b"].tolist() == [23, 20, 22, 21]
    assert entries["rank"].tolist() == [64, 1, 0, 63]
    for bad in (plan(rows, [63, 1, 0, 63], [3, 3]),                      # the hub list is no permutation of the rows of colour 63
                plan(rows, [63, 1, 0, 63], [3, 0], hub_rows=1),          # ... or shorter than they are
                plan([[3, 1, 2, 1]] + rows[1:], [63, 1, 0, 63], [3, 0]),  # a row whose bodies are not its contact's
                plan([[7, 1, 3, 1]] + rows[1:], [63, 1, 0, 63], [3, 0]),  # a contact outside the list
                plan([rows[1]] + rows[1:], [63, 1, 0, 63], [3, 0]),       # a contact with two rows
                plan(rows, [63, 1, 0, 63], [3, 0], solver=pr.SOLVER_EXACT)):
        with pytest.raises(so.PlanMismatch):
            so.solve_order(bad, contacts, flags)
