"""GPU: batched body destruction and activation sets on the device (include/b2hip.h, block I: b2hip_destroy_bodies,
b2hip_set_actives).

The reference is the project's own single-body path - b2hip_destroy_body and b2hip_set_active, made entry by entry as the
header's definition by equivalence says - run on a TWIN world: built by the same script and stepped the same number of times.
Every comparison is bit for bit: tobytes() of contacts() (read first: the single route applies its queued contact operations
to the device when somebody reads the contacts, and only then do the body states show the bodies that the destroyed contacts
woke), of body_states(), of the destroyed marks of every body and fixture and of the fat AABBs of the live proxies. The
330-body world of tests/test_gpu_body_transforms.py is restated here; each test asserts that its batch holds what it is about."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import b2hip

AWAKE, ACTIVE = 4, 64  # b2hip_body_state.flags
SETTLE_STEPS = 40      # the stacks that were put down have gone to sleep, the ones that were dropped are still awake
STACKS, LEVELS, DROPPED_FROM = 80, 4, 64  # the 16 x 20 grid as 80 stacks of 4; stacks 64.. start 1.5 m up
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
f32 = np.float32
SIZES = (1, 63, 64, 65, 257, 0)  # 0: every body without a joint


def _check(rc):
    assert rc == 0, b2hip.lib().b2hip_last_error()


def box_at(hx, hy, cx, cy):
    """a box fixture shape centred at (cx, cy) of its body"""
    s = b2hip.box_shape(hx, hy)
    for i in range(4):
        s.verts[2 * i] += cx
        s.verts[2 * i + 1] += cy
    s.centroid[0], s.centroid[1] = cx, cy
    return s


def build_world(lazy=False, steps=SETTLE_STEPS, inactive=True, events=False):
    """a static ground; a 16 x 20 grid of small dynamic boxes and circles on it, as 80 stacks of four of which the last 16
    are dropped from 1.5 m; a kinematic body; a fixed-rotation body; a body with two fixtures; a weightless body far away;
    an inactive body; a body with three fixtures whose centre of mass is off its origin; two boxes joined by a revolute joint.
    Sleep is allowed; stepped until the stacks that were put down sleep. inactive=False leaves the inactive body active (and
    ids["inactive"] is -1: no such body).
    Returns (world, names -> body ids; "fixtures": body id -> its fixture ids)."""
    w = b2hip.World(allow_sleep=True)
    if lazy:
        w.set_lazy_readback(True)
    if events:
        w.enable_contact_events(True)
    ids = {"fixtures": {}}

    def fixture(body, shape, **kw):
        ids["fixtures"].setdefault(body, []).append(w.create_fixture(body, shape, **kw))

    ids["ground"] = w.create_body(b2hip.STATIC, (0.0, -0.5))
    fixture(ids["ground"], b2hip.box_shape(40.0, 0.5))
    ids["grid"] = []
    for r in range(16):
        for c in range(20):
            stack, level = c + 20 * (r // LEVELS), r % LEVELS
            y = 0.25 + 0.5 * level + (1.5 if stack >= DROPPED_FROM else 0.0)
            b = w.create_body(b2hip.DYNAMIC, (-28.0 + 0.7 * stack, y))
            if level == LEVELS - 1 and c % 3 == 0:
                fixture(b, b2hip.circle_shape(0.25), density=1.0 + c % 3, friction=0.6)
            else:
                fixture(b, b2hip.box_shape(0.25, 0.25), density=1.0 + c % 3, friction=0.6)
            ids["grid"].append(b)
    ids["kinematic"] = w.create_body(b2hip.KINEMATIC, (35.0, 5.0), velocity=(0.25, 0.0), omega=0.3)
    fixture(ids["kinematic"], b2hip.box_shape(0.5, 0.25))
    ids["fixedrot"] = w.create_body(b2hip.DYNAMIC, (32.0, 0.25), fixed_rotation=True)
    fixture(ids["fixedrot"], b2hip.box_shape(0.25, 0.25), density=2.0)
    ids["two"] = w.create_body(b2hip.DYNAMIC, (30.0, 0.25))
    fixture(ids["two"], b2hip.box_shape(0.25, 0.25), density=1.0)
    fixture(ids["two"], box_at(0.25, 0.25, 0.5, 0.0), density=3.0)
    ids["far"] = w.create_body(b2hip.DYNAMIC, (100.0, 50.0), gravity_scale=0.0)
    fixture(ids["far"], b2hip.box_shape(0.5, 0.5), density=1.0)
    ids["inactive"] = w.create_body(b2hip.DYNAMIC, (38.0, 3.0))
    fixture(ids["inactive"], b2hip.box_shape(0.25, 0.25), density=1.0)
    if inactive:
        w.set_active(ids["inactive"], False)
    else:
        ids["inactive"] = -1
    ids["three"] = w.create_body(b2hip.DYNAMIC, (-36.0, 0.25))
    fixture(ids["three"], b2hip.box_shape(0.25, 0.25), density=1.0)
    fixture(ids["three"], box_at(0.25, 0.25, 0.5, 0.0), density=3.0)
    fixture(ids["three"], b2hip.circle_shape(0.2, 0.25, 0.45), density=2.0)
    ids["pair"] = [w.create_body(b2hip.DYNAMIC, (-33.0, 0.25)), w.create_body(b2hip.DYNAMIC, (-32.4, 0.25))]
    for b in ids["pair"]:
        fixture(b, b2hip.box_shape(0.25, 0.25), density=1.0, friction=0.6)
    ids["joint"] = w.create_revolute_joint(ids["pair"][0], ids["pair"][1], anchor_a=(0.3, 0.0), anchor_b=(-0.3, 0.0))
    for _ in range(steps):
        w.step()
    return w, ids


def twins(lazy=False, inactive=True, events=False):
    a, ids = build_world(lazy=lazy, inactive=inactive, events=events)
    b, _ = build_world(lazy=lazy, inactive=inactive, events=events)
    return a, b, ids


def grid_body(ids, stack, level):
    return ids["grid"][20 * (LEVELS * (stack // 20) + level) + stack % 20]


def destroyed_marks(w):
    nb, nf = w.body_count, w.L.b2hip_fixture_count(w.p)
    return (np.asarray([w.L.b2hip_body_is_destroyed(w.p, i) for i in range(nb)], np.int8),
            np.asarray([w.L.b2hip_fixture_is_destroyed(w.p, i) for i in range(nf)], np.int8))


def fat_aabbs(w):
    """every fixture's fat AABB as the device holds it once the pending edits are uploaded (the read of one live body's row
    does that)"""
    alive = next(i for i in range(w.body_count) if not w.L.b2hip_body_is_destroyed(w.p, i))
    w.body_states_of(np.asarray([alive], np.int32))
    n = w.L.b2hip_fixture_count(w.p)
    out = np.zeros((n, 4), f32)
    _check(w.L.b2hip_get_fat_aabbs(w.p, 0, n, out.ctypes.data_as(C.c_void_p)))
    return out


def live_fixtures(w, ids):
    """the fixtures that have a proxy: of bodies that are neither destroyed nor inactive"""
    s = w.body_states()
    dead, _ = destroyed_marks(w)
    out = [f for body, fs in ids["fixtures"].items() if not dead[body] and (s["flags"][body] & ACTIVE) for f in fs]
    return np.asarray(sorted(out), np.int64)


def same(a, b, what, ids=None):
    ca, cb = a.contacts(), b.contacts()
    assert len(ca) == len(cb), "%s: %d contacts against the twin's %d" % (what, len(ca), len(cb))
    assert ca.tobytes() == cb.tobytes(), "%s: contacts differ" % what
    sa, sb = a.body_states(), b.body_states()
    if sa.tobytes() != sb.tobytes():
        bad = [n for n in sa.dtype.names if sa[n].tobytes() != sb[n].tobytes()]
        who = np.flatnonzero(np.any([sa[n].view(np.uint32) != sb[n].view(np.uint32) for n in sa.dtype.names], axis=0))
        raise AssertionError("%s: body states differ in %s, bodies %s" % (what, bad, who[:8].tolist()))
    assert not any(np.isnan(sa[n]).any() for n in sa.dtype.names if n != "flags"), "%s: NaN in the states" % what
    (da, fa), (db, fb) = destroyed_marks(a), destroyed_marks(b)
    assert da.tobytes() == db.tobytes() and fa.tobytes() == fb.tobytes(), "%s: the destroyed marks differ" % what
    if ids is not None:
        live = live_fixtures(a, ids)
        assert live.tobytes() == live_fixtures(b, ids).tobytes()
        xa, xb = fat_aabbs(a)[live], fat_aabbs(b)[live]
        if xa.tobytes() != xb.tobytes():
            who = live[np.flatnonzero(np.any(xa.view(np.uint32) != xb.view(np.uint32), axis=1))]
            raise AssertionError("%s: fat AABBs differ, fixtures %s" % (what, who[:8].tolist()))


def step_and_compare(a, b, what, ids, steps=3):
    for k in range(steps):
        a.step()
        b.step()
        same(a, b, "%s, step %d" % (what, k + 1), ids)


def asleep(w):
    return (w.body_states()["flags"] & AWAKE) == 0


def sleeping_stack(w, ids):
    """a stack of the grid whose four bodies sleep"""
    sl = asleep(w)
    for stack in range(DROPPED_FROM):
        if all(sl[grid_body(ids, stack, lv)] for lv in range(LEVELS)):
            return stack
    raise AssertionError("no stack of the grid sleeps")


def awake_grid_body(w, ids):
    sl = asleep(w)
    awake = [b for b in ids["grid"] if not sl[b]]
    assert awake, "no body of the grid is awake"
    return awake[0]


def batch_of(w, ids, size, seed, jointed=False):
    """`size` body ids in a shuffled order (0: every body without a joint). A batch of one is the bottom of a sleeping stack;
    from 63 on the batch holds the static ground - whose contacts are all the stack bottoms' - the kinematic, the three-fixture
    and the inactive body, a sleeping and an awake grid body, and two bodies that touch each other (the two lowest of a
    sleeping stack). None of the jointed pair, unless asked for."""
    stack = sleeping_stack(w, ids)
    bottom, second = grid_body(ids, stack, 0), grid_body(ids, stack, 1)
    if size == 1:
        return np.asarray([bottom], np.int32)
    rng = np.random.default_rng(seed)
    must = [ids["ground"], ids["kinematic"], ids["three"], ids["inactive"], bottom, second, awake_grid_body(w, ids)]
    must = [m for m in must if m >= 0] + ([ids["pair"][1]] if jointed else [])
    pool = np.setdiff1d(np.arange(w.body_count), must + ids["pair"])
    size = size or len(pool) + len(must)
    bodies = rng.permutation(np.concatenate([must, rng.permutation(pool)[:size - len(must)]]).astype(np.int32))
    assert len(bodies) == size and len(np.unique(bodies)) == size
    touching = w.contacts()
    touching = touching[(touching["flags"] & 1) != 0]
    assert (((touching["body_a"] == bottom) & (touching["body_b"] == second)) | ((touching["body_a"] == second) & (touching["body_b"] == bottom))).any()
    assert np.count_nonzero((touching["body_a"] == ids["ground"]) | (touching["body_b"] == ids["ground"])) > 64
    return bodies


def ids_of(bodies):
    return np.ascontiguousarray(bodies, np.int32)


def single_destroys(w, bodies):
    for b in np.asarray(bodies).tolist():
        w.destroy_body(b)


def single_actives(w, bodies, flags):
    for b, f in zip(np.asarray(bodies).tolist(), np.broadcast_to(flags, (len(bodies),)).tolist()):
        w.set_active(b, bool(f))


def woken_survivors(before_asleep, w, bodies):
    dead, _ = destroyed_marks(w)
    now_awake = ~asleep(w)
    survivors = np.setdiff1d(np.flatnonzero(dead == 0), bodies)
    return survivors[before_asleep[survivors] & now_awake[survivors]]


# ---- 1. destroy equals the loop ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
@pytest.mark.parametrize("size", SIZES)
def test_destroy_equals_the_single_calls_on_a_twin(size, lazy):
    a, b, ids = twins(lazy)
    bodies = batch_of(a, ids, size, 10 + size)
    if size == 0:
        assert len(bodies) == a.body_count - 2
    before_asleep, n_before = asleep(a), len(a.contacts())
    a.destroy_bodies(bodies)
    single_destroys(b, bodies)
    same(a, b, "after the call", ids)
    dead, fdead = destroyed_marks(a)
    assert dead[bodies].all() and dead.sum() == len(bodies)
    assert all(fdead[f] for q in bodies.tolist() for f in ids["fixtures"][q]) and fdead.sum() == sum(len(ids["fixtures"][q]) for q in bodies.tolist())
    assert len(a.contacts()) < n_before
    s = a.body_states()
    assert (s["flags"][bodies] & (ACTIVE | 3)).max() == 0 and not s["vx"][bodies].any() and not s["vy"][bodies].any() and not s["w"][bodies].any()
    assert len(woken_survivors(before_asleep, a, bodies)) > 0, "no surviving neighbour that slept was woken"
    step_and_compare(a, b, "destroy", ids)
    a.close()
    b.close()


# ---- 2. the jointed pair in the batch ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_batch_with_a_jointed_body_equals_the_single_calls():
    a, b, ids = twins()
    bodies = batch_of(a, ids, 64, 20, jointed=True)
    assert ids["pair"][1] in bodies and ids["pair"][0] not in bodies and not a.joint_is_destroyed(ids["joint"])
    a.destroy_bodies(bodies)
    single_destroys(b, bodies)
    assert a.joint_is_destroyed(ids["joint"]) and b.joint_is_destroyed(ids["joint"])
    same(a, b, "after the call", ids)
    step_and_compare(a, b, "a jointed body in the batch", ids)
    # ... and with the joint gone the other body of the pair goes through the batched route
    rest = ids_of([ids["pair"][0], grid_body(ids, 70, 3)])
    rest = rest[[not a.L.b2hip_body_is_destroyed(a.p, int(q)) for q in rest]]
    a.destroy_bodies(rest)
    single_destroys(b, rest)
    same(a, b, "the other body of the pair", ids)
    step_and_compare(a, b, "the other body of the pair", ids, 2)
    a.close()
    b.close()


# ---- 3. set-actives equals the loop --------------------------------------------------------------------------------------------
def active_flags(w, ids, bodies):
    """mixed flags: a third of the entries False; the inactive body activated; the two lowest bodies of a sleeping stack - they
    touch - deactivated; the ground stays (True: an entry that has the requested state already)."""
    flags = (np.arange(len(bodies)) % 3) != 0
    stack = sleeping_stack(w, ids)
    for body, f in ((ids["inactive"], True), (ids["ground"], True), (grid_body(ids, stack, 0), False), (grid_body(ids, stack, 1), False)):
        flags[bodies == body] = f
    return flags


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
@pytest.mark.parametrize("size", SIZES)
def test_set_actives_equal_the_single_calls_on_a_twin(size, lazy):
    a, b, ids = twins(lazy)
    bodies = batch_of(a, ids, size, 30 + size)
    flags = active_flags(a, ids, bodies) if size != 1 else np.asarray([False])
    was_active = (a.body_states()["flags"][bodies] & ACTIVE) != 0
    if size != 1:
        assert (was_active == flags).any() and (was_active & ~flags).sum() >= 2 and (~was_active & flags).sum() == 1
    before_asleep = asleep(a)
    a.set_actives(bodies, flags)
    single_actives(b, bodies, flags)
    same(a, b, "after the call", ids)
    s = a.body_states()
    assert (((s["flags"][bodies] & ACTIVE) != 0) == flags).all()
    off = bodies[was_active & ~flags]
    assert len(woken_survivors(before_asleep, a, off)) > 0, "no neighbour that slept was woken by a deactivation"
    step_and_compare(a, b, "set_actives", ids)
    # a second batch switches on again what the first switched off, in another order: the proxy ids come back last in, first out
    back = np.random.default_rng(5).permutation(off)[::-1].copy()
    if len(back) > 2:
        assert back.tolist() != off.tolist() and back.tolist() != off[::-1].tolist()
    a.set_actives(back)
    single_actives(b, back, True)
    same(a, b, "switched on again", ids)
    assert ((a.body_states()["flags"][back] & ACTIVE) != 0).all()
    step_and_compare(a, b, "switched on again", ids, 5)
    a.close()
    b.close()


@pytest.mark.gpu
def test_a_snapshot_carries_the_activation_sets():
    """(the world without its inactive body, and everything active again at the end: a snapshot of a world that holds a
    deactivated body is not loaded - its fixtures have no proxy id, which the loader takes for corruption)"""
    a, b, ids = twins(inactive=False)
    bodies = batch_of(a, ids, 257, 51)
    flags = active_flags(a, ids, bodies)
    off = bodies[~flags]
    a.set_actives(bodies, flags)
    single_actives(b, bodies, flags)
    step_and_compare(a, b, "switched off", ids, 2)
    back = np.random.default_rng(6).permutation(off)
    a.set_actives(back, np.ones(len(back), bool))
    single_actives(b, back, True)
    assert ((a.body_states()["flags"] & ACTIVE) != 0).all()
    r = b2hip.World.from_snapshot(a.save_snapshot())
    same(r, b, "the restored world", ids)
    for k in range(3):
        r.step()
        b.step()
        a.step()
        same(r, b, "step %d of the restored world" % (k + 1), ids)
        same(a, b, "step %d of the world the snapshot was taken of" % (k + 1), ids)
    for w in (a, b, r):
        w.close()


# ---- 4. order against other edits ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ("single destroy before the batch", "single set_active after the batch", "two batches", "a new body",
                                  "forces, then off, then on"))
def test_batches_keep_their_order_with_other_edits(case):
    a, b, ids = twins()
    bodies = batch_of(a, ids, 64, 41)
    flags = active_flags(a, ids, bodies)
    x = awake_grid_body(a, ids)
    assert x in bodies
    if case == "single destroy before the batch":
        # a body that rests on the ground, which the batch names: its queued operation destroys a touching contact with a
        # body of the batch. The batch sends that operation to the device before its own rows (the header's "Order"); the twin
        # reads its contact count between the single call and the loop, which does the same.
        lone = ids["fixedrot"] if ids["fixedrot"] not in bodies else ids["two"]
        assert lone not in bodies and ids["ground"] in bodies
        con = a.contacts()
        assert ((con["flags"] & 1) != 0)[((con["body_a"] == lone) & (con["body_b"] == ids["ground"])) | ((con["body_b"] == lone) & (con["body_a"] == ids["ground"]))].any()
        for w in (a, b):
            w.destroy_body(lone)
        b.contact_count  # noqa: B018
        a.destroy_bodies(bodies)
        single_destroys(b, bodies)
        assert a.L.b2hip_body_is_destroyed(a.p, lone)
    elif case == "single set_active after the batch":
        a.set_actives(bodies, flags)
        single_actives(b, bodies, flags)
        off, on = int(bodies[~flags][0]), int(bodies[flags & (bodies != ids["ground"])][0])
        for w in (a, b):
            w.set_active(off, True)   # (the host's copy of the bit says "inactive": the call acts)
            w.set_active(on, False)
            w.set_active(ids["inactive"], False)
        s = a.body_states()["flags"]
        assert (s[off] & ACTIVE) and not (s[on] & ACTIVE) and not (s[ids["inactive"]] & ACTIVE)
    elif case == "two batches":
        second = batch_of(a, ids, 65, 42)
        flags2 = ~active_flags(a, ids, second)
        flags2[second == ids["ground"]] = True
        assert len(np.intersect1d(bodies, second)) > 7
        # A call sends the pending edits to the device first, queued contact operations included, and the definition by
        # equivalence is per call. The twin reads its contact count between the loops, which does the same: without that its
        # three loops' rows are uploaded together before any of their contacts goes, and a body that the first loop's
        # destroyed contacts wake and the third loop destroys ends with another awake bit.
        a.set_actives(bodies, flags)
        a.set_actives(second, flags2)
        single_actives(b, bodies, flags)
        b.contact_count  # noqa: B018 (a read that applies the queued operations)
        single_actives(b, second, flags2)
        b.contact_count  # noqa: B018
        gone = second[::3]
        a.destroy_bodies(gone)
        single_destroys(b, gone)
    elif case == "a new body":
        for w in (a, b):
            n = w.create_body(b2hip.DYNAMIC, (-10.15, 2.3))  # (above a stack)
            f = w.create_fixture(n, b2hip.box_shape(0.25, 0.25), density=1.0)
            m = w.create_body(b2hip.DYNAMIC, (-5.0, 9.0))
            g = w.create_fixture(m, b2hip.circle_shape(0.25), density=1.0)
        ids["fixtures"][n], ids["fixtures"][m] = [f], [g]
        a.set_actives([x, n], [False, False])
        single_actives(b, [x, n], False)
        a.destroy_bodies([m, int(bodies[0])])
        single_destroys(b, [m, int(bodies[0])])
        a.set_actives([n])
        single_actives(b, [n], True)
        assert a.body_states()["flags"][n] & ACTIVE and a.L.b2hip_body_is_destroyed(a.p, m)
    else:
        some = ids_of([x, grid_body(ids, 3, 3), grid_body(ids, 70, 2)])
        a.apply_forces(some, (3.0, 40.0), 0.25)
        for q in some.tolist():
            b.apply_force(q, (3.0, 40.0), 0.25)
        a.set_actives(some, False)
        single_actives(b, some, False)
        same(a, b, case + ", switched off", ids)
        a.set_actives(some[::-1], True)
        single_actives(b, some[::-1], True)
    same(a, b, case + ", before the step", ids)
    step_and_compare(a, b, case, ids)
    a.close()
    b.close()


# ---- 5. queries see the batch before any step ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_queries_see_the_batch_before_any_step():
    a, b, ids = twins()
    s = a.body_states()
    grid = np.asarray(ids["grid"])
    gone, off = grid[5:60:5].astype(np.int32), grid[7:60:5].astype(np.int32)
    on = ids_of([ids["inactive"]])
    watch = np.concatenate([gone, off, on])
    # (a short ray into each body from the gap between its stack and the next: 0.2 m wide, the bodies 0.25 m to each side)
    p1 = np.stack([s["px"][watch] - 0.34, s["py"][watch]], axis=1).astype(f32)
    p2 = np.stack([s["px"][watch], s["py"][watch]], axis=1).astype(f32)
    lower, upper = (np.stack([s["px"][watch], s["py"][watch]], axis=1) - 0.05).astype(f32), (np.stack([s["px"][watch], s["py"][watch]], axis=1) + 0.05).astype(f32)
    hits_before = a.ray_cast_closest(p1, p2)
    assert (hits_before["body"][:len(gone) + len(off)] == watch[:len(gone) + len(off)]).all() and hits_before["body"][-1] != on[0]
    a.destroy_bodies(gone)
    a.set_actives(np.concatenate([off, on]), np.concatenate([np.zeros(len(off), bool), [True]]))
    single_destroys(b, gone)
    single_actives(b, off, False)
    single_actives(b, on, True)
    ha, hb = a.ray_cast_closest(p1, p2), b.ray_cast_closest(p1, p2)
    assert ha.tobytes() == hb.tobytes(), "ray_cast_closest differs"
    assert not np.isin(ha["body"], np.concatenate([gone, off])).any(), "a ray hits a body that is destroyed or inactive"
    assert ha["body"][-1] == on[0], "the ray across the activated body misses it"
    (oa, ia), (ob, ib) = a.query_aabbs(lower, upper), b.query_aabbs(lower, upper)
    assert oa.tobytes() == ob.tobytes() and ia.tobytes() == ib.tobytes(), "query_aabbs differs"
    assert not np.isin(ia["body"], np.concatenate([gone, off])).any() and on[0] in ia["body"][oa[-2]:oa[-1]]
    same(a, b, "after the queries", ids)
    step_and_compare(a, b, "after the queries", ids)
    a.close()
    b.close()


# ---- 6. contact events -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_end_events_of_destroyed_contacts_are_delivered_with_the_next_step():
    a, b, ids = twins(events=True)
    bodies = batch_of(a, ids, 65, 61)
    flags = active_flags(a, ids, bodies)
    for call_a, call_b in ((lambda: a.set_actives(bodies, flags), lambda: single_actives(b, bodies, flags)),
                           (lambda: a.destroy_bodies(bodies[::2]), lambda: single_destroys(b, bodies[::2]))):
        call_a()
        call_b()
        a.step()
        b.step()
        ea, eb = a.contact_events(), b.contact_events()
        # rows (fixture_a, fixture_b, kind, contact_index), sorted by fixture pair and kind
        key = lambda e: np.lexsort((e[:, 2], e[:, 1], e[:, 0]))  # noqa: E731
        ea, eb = ea[key(ea)], eb[key(eb)]
        assert ((ea[:, 2] == 1) & (ea[:, 3] == -1)).any(), "no end event of a destroyed contact"
        assert ea.tobytes() == eb.tobytes(), "the events differ from the twin's"
        same(a, b, "after the step", ids)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ("destroy", "activate only", "jointed"))
def test_the_end_events_of_a_single_call_underneath_a_batch_are_delivered(batch):
    """b2hip_destroy_body(x), then a batch, then a step: the batch applies x's queued operation between steps, and its end
    events must reach the next step's list as the batch's own do - also when the batch itself destroys no contact, and when it
    takes the loop of single calls for a jointed body."""
    a, b, ids = twins(events=True)
    stack = sleeping_stack(a, ids)
    x = grid_body(ids, stack, 1)
    for w in (a, b):
        w.destroy_body(x)
    if batch == "activate only":
        a.set_actives([ids["inactive"]])
        b.set_active(ids["inactive"], True)
    else:
        bodies = ids_of([grid_body(ids, stack + 1, 0), ids["three"]] + ([ids["pair"][0]] if batch == "jointed" else []))
        a.destroy_bodies(bodies)
        single_destroys(b, bodies)
    a.step()
    b.step()
    ea, eb = a.contact_events(), b.contact_events()
    key = lambda e: np.lexsort((e[:, 2], e[:, 1], e[:, 0]))  # noqa: E731
    ea, eb = ea[key(ea)], eb[key(eb)]
    fx = ids["fixtures"][x][0]
    assert (((ea[:, 0] == fx) | (ea[:, 1] == fx)) & (ea[:, 2] == 1)).sum() >= 2, "the end events of the single call's contacts are missing"
    assert ea.tobytes() == eb.tobytes(), "the events differ from the twin's"
    a.close()
    b.close()


# ---- 7. the TOI partition --------------------------------------------------------------------------------------------------------
def bullet_world():
    """continuous physics: a floor, a wall of static and dynamic boxes in turn, a dozen bullets - some in flight towards the wall,
    some at rest against its foot. Returns (world, the dynamic bodies)."""
    w = b2hip.World(gravity=(0.0, -10.0), allow_sleep=True, continuous=True)
    ground = w.create_body(b2hip.STATIC, (0.0, -0.5))
    w.create_fixture(ground, b2hip.box_shape(40.0, 0.5))
    movable = []
    for k in range(8):
        kind = b2hip.STATIC if k % 2 == 0 else b2hip.DYNAMIC
        q = w.create_body(kind, (10.0, 0.25 + 0.5 * k))
        w.create_fixture(q, b2hip.box_shape(0.1, 0.25), density=2.0, friction=0.5)
        if kind == b2hip.DYNAMIC:
            movable.append(q)
    for k in range(12):
        if k % 2 == 0:  # in flight, one behind the other and at several heights
            q = w.create_body(b2hip.DYNAMIC, (-2.0 - 1.5 * k, 0.6 + 0.25 * k), velocity=(60.0 + 5.0 * k, 0.0), bullet=True, gravity_scale=0.0)
        else:           # at rest on the floor, the first against the wall's foot
            q = w.create_body(b2hip.DYNAMIC, (9.75 - 0.35 * (k // 2), 0.1), bullet=True)
        w.create_fixture(q, b2hip.circle_shape(0.1), density=1.0, restitution=0.3)
        movable.append(q)
    for _ in range(4):
        w.step()
    return w, np.asarray(movable, np.int32)


def toi_slots(w):
    """SnapHeader::nToiOrder of a snapshot taken now (b2hip_api_snapshot.h): magic, six sizes, then the counts"""
    return struct.unpack_from("<I", w.save_snapshot(), 8 + 4 * 12)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("sort_max", (None, 2))
def test_the_toi_partition_is_given_back_in_the_loops_order(sort_max):
    """sort_max 2: B2HIP_TEST_LIFECYCLE_SORT_MAX lowers the one-workgroup sort's capacity, so that the list of this small world
    goes through the radix sort (b2hip_debug_read 29 counts those)."""
    if sort_max is not None:
        os.environ["B2HIP_TEST_LIFECYCLE_SORT_MAX"] = str(sort_max)
    try:
        (a, movable), (b, _), (c, _) = bullet_world(), bullet_world(), bullet_world()
    finally:
        os.environ.pop("B2HIP_TEST_LIFECYCLE_SORT_MAX", None)
    snapshots_agree = a.save_snapshot() == b.save_snapshot()
    assert toi_slots(a) >= 6
    con = a.contacts()
    first = {int(q): int(np.flatnonzero((con["body_a"] == q) | (con["body_b"] == q))[0]) for q in movable.tolist()
             if ((con["body_a"] == q) | (con["body_b"] == q)).any()}
    with_contacts = sorted(first, key=lambda q: first[q])
    assert len(with_contacts) >= 4
    # neither ascending nor descending in contact index: the second of them first, then the last, then the first, the rest shuffled
    head = [with_contacts[1], with_contacts[-1], with_contacts[0]]
    rest = np.random.default_rng(7).permutation(np.setdiff1d(movable, head))[:5]
    bodies = ids_of(head + rest.tolist())
    order = [first[q] for q in bodies.tolist() if q in first]
    assert order != sorted(order) and order != sorted(order)[::-1]
    # the twin of the twin says how many slots every entry gives back: at least three, from at least two entries
    freed, have = [], toi_slots(c)
    for q in bodies.tolist():
        c.destroy_body(q)
        now = toi_slots(c)
        freed.append(have - now)
        have = now
    assert sum(freed) >= 3 and np.count_nonzero(freed) >= 2, freed
    c.close()
    before = toi_slots(a)
    a.destroy_bodies(bodies)
    single_destroys(b, bodies)
    same(a, b, "after the call")
    assert before - toi_slots(a) == sum(freed) and toi_slots(b) == toi_slots(a)
    if snapshots_agree:
        assert a.save_snapshot() == b.save_snapshot(), "the snapshots differ"
    long_sorts = C.c_longlong(0)
    _check(a.L.b2hip_debug_read(a.p, 29, 0, 1, C.byref(long_sorts)))
    assert (long_sorts.value >= 1) == (sort_max is not None), long_sorts.value
    for k in range(25):
        a.step()
        b.step()
        same(a, b, "continuous, step %d" % (k + 1))
    a.close()
    b.close()


# ---- 8. refusals apply nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_calls_name_the_offender_and_apply_nothing():
    a, b, ids = twins()
    n = a.body_count
    victim = ids["grid"][7]
    for w in (a, b):
        w.destroy_body(victim)
    con_before = a.contacts()  # (first: the read applies the single call's queued operation, which wakes the victim's neighbours)
    before = a.body_states()
    good = np.asarray(ids["grid"][20:30], np.int32)

    def refused(bodies, words):
        bodies = np.asarray(bodies, np.int32)
        for call in (lambda: a.destroy_bodies(bodies), lambda: a.set_actives(bodies, False), lambda: a.set_actives(bodies, True)):
            with pytest.raises(b2hip.B2HipError) as e:
                call()
            for word in words:
                assert word in str(e.value), (word, str(e.value))
        assert a.body_states().tobytes() == before.tobytes() and a.contacts().tobytes() == con_before.tobytes()

    bad = good.copy()
    bad[6] = n
    refused(bad, ("entry 6", "body %d" % n))
    bad[6] = -1
    refused(bad, ("entry 6", "body -1"))
    bad = good.copy()
    bad[8] = good[2]
    refused(bad, ("entry 8", "body %d" % good[2]))
    bad = good.copy()
    bad[3] = victim
    refused(bad, ("entry 3", "body %d" % victim, "destroyed"))
    # inside a step
    _check(a.L.b2hip_step_begin(a.p, C.c_float(1.0 / 60.0), 8, 3))
    for call in (lambda: a.destroy_bodies(good), lambda: a.set_actives(good, False)):
        with pytest.raises(b2hip.B2HipError) as e:
            call()
        assert "inside a step" in str(e.value)
    for fn in ("b2hip_collide", "b2hip_solve", "b2hip_sync_fixtures", "b2hip_find_new_contacts", "b2hip_solve_toi", "b2hip_step_end"):
        _check(getattr(a.L, fn)(a.p))
    b.step()
    same(a, b, "a step after the refused calls", ids)
    # n == 0 succeeds
    none = np.zeros(0, np.int32)
    a.destroy_bodies(none)
    a.set_actives(none, np.zeros(0, bool))
    a.step()
    b.step()
    same(a, b, "after the empty calls", ids)
    a.close()
    b.close()


@pytest.mark.gpu
def test_the_move_buffer_is_guarded():
    a, b, ids = twins()
    bodies = np.random.default_rng(7).permutation(np.setdiff1d(np.arange(a.body_count), [ids["inactive"]])).astype(np.int32)
    refusals = 0
    for k in range(10):
        flag = k % 2 == 1
        before, con_before = a.body_states(), a.contacts()
        rc = a.L.b2hip_set_actives(a.p, len(bodies), bodies.ctypes.data_as(C.c_void_p), np.full(len(bodies), flag, np.uint8).ctypes.data_as(C.c_void_p))
        if k < 2:
            assert rc == 0, "switching every body of a freshly stepped world off and on again must fit"
        if rc == 0:
            single_actives(b, bodies, flag)
            continue
        refusals += 1
        assert rc == ERR_UNSUPPORTED and flag, rc
        msg = a.L.b2hip_last_error().decode()
        assert "step" in msg and "move buffer" in msg, msg
        assert a.body_states().tobytes() == before.tobytes() and a.contacts().tobytes() == con_before.tobytes(), "a refused call changed the world"
        break
    assert refusals == 1, "ten rounds of activations fitted a buffer of 2 x fixtures + 64 moves"
    same(a, b, "after the calls that were accepted", ids)
    a.step()
    b.step()
    same(a, b, "step 1", ids)
    a.set_actives(bodies, True)  # (the step emptied the buffer)
    single_actives(b, bodies, True)
    step_and_compare(a, b, "after the guard", ids, 2)
    a.close()
    b.close()


# ---- 9. a world emptied and refilled ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_world_emptied_and_refilled():
    a, b, ids = twins()
    everybody = np.setdiff1d(np.arange(a.body_count), [ids["inactive"]]).astype(np.int32)
    a.set_actives(everybody, False)
    single_actives(b, everybody, False)
    same(a, b, "emptied", ids)
    assert len(a.contacts()) == 0 and len(live_fixtures(a, ids)) == 0
    one = int(everybody[17])
    before = a.body_states()
    rc_b = b.L.b2hip_set_active(b.p, one, 1)
    rc_a = a.L.b2hip_set_actives(a.p, 1, ids_of([one]).ctypes.data_as(C.c_void_p), np.ones(1, np.uint8).ctypes.data_as(C.c_void_p))
    assert rc_a == rc_b and rc_b in (0, ERR_UNSUPPORTED), (rc_a, rc_b)
    if rc_b == ERR_UNSUPPORTED:
        msg = a.L.b2hip_last_error().decode()
        assert "entry 0" in msg and "body %d" % one in msg and "not modelled" in msg, msg
        assert a.body_states().tobytes() == before.tobytes() and len(a.contacts()) == 0 and len(live_fixtures(a, ids)) == 0
        a.step()  # (the refused batch left the world as it was: it still steps)
        assert a.body_states().tobytes() == before.tobytes()
    else:
        same(a, b, "one body switched on again", ids)
        step_and_compare(a, b, "refilled", ids)
    a.close()
    b.close()
