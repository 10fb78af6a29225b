"""GPU: batched forces, impulses and velocity sets on the device, and the gather of body-state rows (include/b2hip.h, block F).

The reference is the project's own single-body path - b2hip_apply_force, b2hip_set_velocity, the three b2hip_apply_*_impulse
calls, made entry by entry as the header's definition by equivalence says - run on a TWIN world: built by the same script
and stepped the same number of times. Every comparison is bit for bit: tobytes() of body_states(), and of contacts() after
stepping. One hand-made world of 325 bodies serves all tests; each test asserts that its batch holds what it is about."""
import ctypes as C

import numpy as np
import pytest

import b2hip

AWAKE = 4          # b2hip_body_state.flags: the awake bit
SETTLE_STEPS = 40  # the stacks that were put down have gone to sleep, the ones that were dropped are still awake
STACKS, LEVELS, DROPPED_FROM = 80, 4, 64  # the 16 x 20 grid as 80 stacks of 4; stacks 64.. start 1.5 m up
f32 = np.float32


def box_at(hx, hy, cx, cy):
    """a box fixture shape centred at (cx, cy) of its body"""
    s = b2hip.box_shape(hx, hy)
    for i in range(4):
        s.verts[2 * i] += cx
        s.verts[2 * i + 1] += cy
    s.centroid[0], s.centroid[1] = cx, cy
    return s


def build_world(library=None, lazy=False, steps=SETTLE_STEPS):
    """a static ground; a 16 x 20 grid of small dynamic boxes and circles on it, as 80 stacks of four of which the last 16
    are dropped from 1.5 m; a kinematic body; a fixed-rotation body; a body with two fixtures (its centre of mass is not its
    origin); a weightless body far away. Sleep is allowed; stepped until the stacks that were put down sleep.
    Returns (world, names -> body ids)."""
    w = b2hip.World(allow_sleep=True, library=library)
    if lazy:
        w.set_lazy_readback(True)
    ids = {}
    ids["ground"] = w.create_body(b2hip.STATIC, (0.0, -0.5))
    w.create_fixture(ids["ground"], b2hip.box_shape(40.0, 0.5))
    ids["grid"] = []
    for r in range(16):
        for c in range(20):
            stack, level = c + 20 * (r // LEVELS), r % LEVELS
            y = 0.25 + 0.5 * level + (1.5 if stack >= DROPPED_FROM else 0.0)
            b = w.create_body(b2hip.DYNAMIC, (-28.0 + 0.7 * stack, y))
            if level == LEVELS - 1 and c % 3 == 0:
                w.create_fixture(b, b2hip.circle_shape(0.25), density=1.0 + c % 3, friction=0.6)
            else:
                w.create_fixture(b, b2hip.box_shape(0.25, 0.25), density=1.0 + c % 3, friction=0.6)
            ids["grid"].append(b)
    ids["kinematic"] = w.create_body(b2hip.KINEMATIC, (35.0, 5.0), velocity=(0.25, 0.0), omega=0.3)
    w.create_fixture(ids["kinematic"], b2hip.box_shape(0.5, 0.25))
    ids["fixedrot"] = w.create_body(b2hip.DYNAMIC, (32.0, 0.25), fixed_rotation=True)
    w.create_fixture(ids["fixedrot"], b2hip.box_shape(0.25, 0.25), density=2.0)
    ids["two"] = w.create_body(b2hip.DYNAMIC, (30.0, 0.25))
    w.create_fixture(ids["two"], b2hip.box_shape(0.25, 0.25), density=1.0)
    w.create_fixture(ids["two"], box_at(0.25, 0.25, 0.5, 0.0), density=3.0)
    ids["far"] = w.create_body(b2hip.DYNAMIC, (100.0, 50.0), gravity_scale=0.0)
    w.create_fixture(ids["far"], b2hip.box_shape(0.5, 0.5), density=1.0)
    for _ in range(steps):
        w.step()
    return w, ids


def twins(lazy=False):
    a, ids = build_world(lazy=lazy)
    b, _ = build_world(lazy=lazy)
    return a, b, ids


_control = {}


def control(step):
    """body_states() of the untouched world `step` steps after SETTLE_STEPS (computed once, shared, never written)"""
    if not _control:
        w, _ = build_world()
        _control[0] = w.body_states()
        for k in (1, 2, 3):
            w.step()
            _control[k] = w.body_states()
        w.close()
    return _control[step]


def same(a, b, what, contacts=True):
    sa, sb = a.body_states(), b.body_states()
    if sa.tobytes() != sb.tobytes():
        bad = [n for n in sa.dtype.names if sa[n].tobytes() != sb[n].tobytes()]
        who = np.flatnonzero(np.any([sa[n].view(np.uint32) != sb[n].view(np.uint32) for n in sa.dtype.names], axis=0))
        raise AssertionError("%s: body states differ in %s, bodies %s" % (what, bad, who[:8].tolist()))
    if contacts:
        assert a.contacts().tobytes() == b.contacts().tobytes(), "%s: contacts differ" % what


def asleep(w):
    return (w.body_states()["flags"] & AWAKE) == 0


def batch_of(w, ids, size, seed, wake=1):
    """`size` body ids in a shuffled order; from 63 on the batch holds the static ground, the kinematic body, the fixed-rotation
    body, the two-fixture body, the far body, a sleeping and an awake body of the grid. A batch of one is a body the call acts on."""
    n = w.body_count
    sl = asleep(w)
    grid = np.asarray(ids["grid"])
    sleeping, awake = grid[sl[grid]], grid[~sl[grid]]
    assert len(sleeping) > 0 and len(awake) > 0, "the world holds %d sleeping and %d awake grid bodies" % (len(sleeping), len(awake))
    rng = np.random.default_rng(seed)
    if size == 1:
        return np.asarray([ids["two"] if wake else awake[0]], np.int32)
    must = [ids["ground"], ids["kinematic"], ids["fixedrot"], ids["two"], ids["far"], int(sleeping[0]), int(awake[0])]
    rest = np.setdiff1d(np.arange(n), must)
    bodies = np.concatenate([must, rng.permutation(rest)[:size - len(must)]]).astype(np.int32)
    bodies = rng.permutation(bodies)
    assert len(bodies) == min(size, n) and len(np.unique(bodies)) == len(bodies)
    assert sl[bodies].any() and (~sl[bodies]).any()
    return bodies


def pushes_of(w, bodies, seed, scale):
    """a BODY_PUSH_DTYPE record per body, every other one at a world point near the body; some zeros and a negative zero"""
    rng = np.random.default_rng(seed)
    n = len(bodies)
    s = w.body_states()[bodies]
    p = np.zeros(n, b2hip.BODY_PUSH_DTYPE)
    p["x"], p["y"] = rng.uniform(-scale, scale, n), rng.uniform(0.0, 2.0 * scale, n)
    p["angular"] = rng.uniform(-0.1 * scale, 0.1 * scale, n)
    p["at_point"] = (np.arange(n) + seed) % 2
    p["px"], p["py"] = s["px"] + rng.uniform(-0.3, 0.3, n).astype(f32), s["py"] + rng.uniform(-0.3, 0.3, n).astype(f32)
    p["angular"][::5] = 0.0
    p["angular"][2::7] = -0.0
    if n > 1:
        assert (p["at_point"] == 0).any() and (p["at_point"] == 1).any()
    return p


def single_forces(w, bodies, p, wake):
    s = w.body_states()
    for b, q in zip(bodies.tolist(), p):
        t = q["angular"]
        if q["at_point"]:
            t = f32(q["angular"] + f32(f32(f32(q["px"] - s["cx"][b]) * q["y"]) - f32(f32(q["py"] - s["cy"][b]) * q["x"])))
        w.apply_force(b, (float(q["x"]), float(q["y"])), float(t), wake)


def single_impulses(w, bodies, p, wake):
    for b, q in zip(bodies.tolist(), p):
        if q["at_point"]:
            w.apply_linear_impulse(b, (float(q["x"]), float(q["y"])), (float(q["px"]), float(q["py"])), wake)
        else:
            w.apply_linear_impulse_to_center(b, (float(q["x"]), float(q["y"])), wake)
        w.apply_angular_impulse(b, float(q["angular"]), wake)


def single_velocities(w, bodies, v3, mask):
    s = w.body_states()
    for b, v in zip(bodies.tolist(), v3):
        vx, vy = (v[0], v[1]) if mask & 1 else (s["vx"][b], s["vy"][b])
        om = v[2] if mask & 2 else s["w"][b]
        w.set_velocity(b, (float(vx), float(vy)), float(om))


def velocities_of(bodies, seed):
    rng = np.random.default_rng(seed)
    v3 = rng.uniform(-2.0, 2.0, (len(bodies), 3)).astype(f32)
    v3[::4] = 0.0  # (a zero velocity does not wake)
    return v3


def step_and_compare(a, b, what, steps=3):
    for k in range(steps):
        a.step()
        b.step()
        same(a, b, "%s, step %d" % (what, k + 1))


SIZES = (1, 63, 64, 65, 257, 0)  # 0: every body


def must_change(a, size, what):
    """the large batches change at least one body in at least one field against the world nobody touched"""
    if size == 257 or size == 0:
        assert a.body_states().tobytes() != control(1).tobytes(), "%s changed nothing" % what


@pytest.mark.gpu
@pytest.mark.parametrize("wake", (0, 1))
@pytest.mark.parametrize("size", SIZES)
def test_forces_equal_the_single_calls_on_a_twin(size, wake):
    a, b, ids = twins()
    bodies = batch_of(a, ids, size or a.body_count, 10 + size, wake)
    p = pushes_of(a, bodies, size + wake, 40.0)
    a.apply_forces(bodies, p, wake=wake)
    single_forces(b, bodies, p, wake)
    same(a, b, "after the call", contacts=False)
    a.step()
    b.step()
    same(a, b, "step 1")
    must_change(a, size, "forces")
    step_and_compare(a, b, "forces", 2)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wake", (0, 1))
@pytest.mark.parametrize("size", SIZES)
def test_impulses_equal_the_single_calls_on_a_twin(size, wake):
    a, b, ids = twins()
    bodies = batch_of(a, ids, size or a.body_count, 20 + size, wake)
    p = pushes_of(a, bodies, size + wake, 1.0)
    before = a.body_states()
    a.apply_impulses(bodies, p, wake=wake)
    single_impulses(b, bodies, p, wake)
    same(a, b, "after the call", contacts=False)
    assert a.body_states().tobytes() != before.tobytes(), "the impulses changed nothing"
    a.step()
    b.step()
    same(a, b, "step 1")
    must_change(a, size, "impulses")
    step_and_compare(a, b, "impulses", 2)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", (1, 2, 3))
@pytest.mark.parametrize("size", SIZES)
def test_velocities_equal_the_single_calls_on_a_twin(size, mask):
    a, b, ids = twins()
    bodies = batch_of(a, ids, size or a.body_count, 30 + size)
    v3 = velocities_of(bodies, size + mask)
    if size == 1:
        v3[0] = (0.5, 1.0, -2.0)
    before = a.body_states()
    a.set_velocities(bodies, v3[:, :2] if mask & 1 else None, v3[:, 2] if mask & 2 else None)
    single_velocities(b, bodies, v3, mask)
    same(a, b, "after the call", contacts=False)
    assert a.body_states().tobytes() != before.tobytes(), "the velocities changed nothing"
    if size != 1:
        s = a.body_states()
        assert s["vx"][ids["ground"]] == 0 and s["w"][ids["ground"]] == 0, "the static body was given a velocity"
        k = int(np.flatnonzero(bodies == ids["kinematic"])[0])
        if mask & 2:
            assert s["w"][ids["kinematic"]] == v3[k, 2], "the kinematic body was skipped"
    a.step()
    b.step()
    same(a, b, "step 1")
    must_change(a, size, "velocities")
    step_and_compare(a, b, "velocities", 2)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ("forces", "impulses"))
def test_sleepers_are_left_alone_or_woken_at_once(family):
    a, b, ids = twins()
    sl = asleep(a)
    grid = np.asarray(ids["grid"])
    # the lowest box of every sleeping stack: its neighbours above it sleep too
    bottoms = np.asarray([g for k, g in enumerate(grid) if (k // 20) % LEVELS == 0 and sl[g]], np.int32)
    assert len(bottoms) >= 16, "only %d sleeping stacks" % len(bottoms)
    above = bottoms + 20  # (the grid was created row by row: the next level of the same stack)
    assert sl[above].all()
    bodies = bottoms[::2]
    p = pushes_of(a, bodies, 5, 30.0 if family == "forces" else 0.5)
    batched = a.apply_forces if family == "forces" else a.apply_impulses
    single = single_forces if family == "forces" else single_impulses
    before = a.body_states()
    batched(bodies, p, wake=0)
    single(b, bodies, p, 0)
    assert a.body_states().tobytes() == before.tobytes(), "wake = 0 touched a sleeping body"
    same(a, b, "wake 0, after the call", contacts=False)
    a.step()
    b.step()
    same(a, b, "wake 0, step 1")
    assert asleep(a)[bodies].all() and asleep(a)[above].all(), "wake = 0: a sleeping body woke up"
    assert a.body_states()[bodies].tobytes() == before[bodies].tobytes()
    batched(bodies, p, wake=1)
    single(b, bodies, p, 1)
    s = a.body_states()
    assert (s["flags"][bodies] & AWAKE).all() and (s["sleep_time"][bodies] == 0).all(), "wake = 1: not awake at once"
    assert asleep(a)[above[::2]].all(), "the neighbours woke before a step"
    same(a, b, "wake 1, after the call", contacts=False)
    a.step()
    b.step()
    same(a, b, "wake 1, step 1")
    assert not asleep(a)[above[::2]].any(), "the neighbours did not wake with the step"
    assert asleep(a)[above[1::2]].all(), "a stack nobody pushed woke up"
    step_and_compare(a, b, "wake 1", 2)
    a.close()
    b.close()


def awake_body(w, ids):
    grid = np.asarray(ids["grid"])
    return int(grid[~asleep(w)[grid]][0])


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
def test_single_edits_before_and_after_a_batch(lazy):
    """single apply_force on x, batched forces including x, single apply_force on x, step; then the same with set_velocity,
    batched impulses and a single angular impulse, compared before any step"""
    a, b, ids = twins(lazy)
    x = awake_body(a, ids)
    bodies = batch_of(a, ids, 65, 41)
    bodies[0] = x if x not in bodies else bodies[0]
    assert x in bodies
    p = pushes_of(a, bodies, 3, 40.0)
    for w, batched in ((a, True), (b, False)):
        w.apply_force(x, (3.0, 50.0), 0.25)
        if batched:
            w.apply_forces(bodies, p)
        else:
            single_forces(w, bodies, p, 1)
        w.apply_force(x, (-1.0, 20.0), -0.125)
    same(a, b, "forces, before the step", contacts=False)
    step_and_compare(a, b, "single force, batched forces, single force", 2)
    assert a.body_states()[x].tobytes() != control(2)[x].tobytes()
    q = pushes_of(a, bodies, 4, 1.0)
    for w, batched in ((a, True), (b, False)):
        w.set_velocity(x, (0.5, 2.0), 1.0)
        if batched:
            w.apply_impulses(bodies, q)
        else:
            single_impulses(w, bodies, q, 1)
        w.apply_angular_impulse(x, 0.05)
    same(a, b, "set_velocity, batched impulses, single angular impulse", contacts=False)
    step_and_compare(a, b, "impulses between single edits", 2)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
def test_a_batched_velocity_survives_set_transform_and_reaches_a_new_body(lazy):
    a, b, ids = twins(lazy)
    x = awake_body(a, ids)
    bodies = batch_of(a, ids, 64, 43)
    if x not in bodies:
        bodies[0] = x
    v3 = velocities_of(bodies, 9)
    v3[int(np.flatnonzero(bodies == x)[0])] = (1.5, 2.5, -0.75)
    for w, batched in ((a, True), (b, False)):
        if batched:
            w.set_velocities(bodies, v3[:, :2], v3[:, 2])
        else:
            single_velocities(w, bodies, v3, 3)
        _check(w.L.b2hip_set_transform(w.p, x, C.c_float(-27.5), C.c_float(6.0), C.c_float(0.5)))
    s = a.body_states()
    assert (s["vx"][x], s["vy"][x], s["w"][x]) == (1.5, 2.5, -0.75) and s["py"][x] == 6.0, "the velocity did not survive set_transform"
    same(a, b, "velocities, set_transform", contacts=False)
    step_and_compare(a, b, "velocities, set_transform", 2)
    # a body created after the last step, a batched velocity set on it, a single force on it
    for w, batched in ((a, True), (b, False)):
        n = w.create_body(b2hip.DYNAMIC, (-20.0, 8.0))
        w.create_fixture(n, b2hip.box_shape(0.25, 0.25), density=1.0)
        both = np.asarray([x, n], np.int32)
        v = np.asarray([[0.0, 1.0, 0.5], [2.0, -1.0, 3.0]], f32)
        if batched:
            w.set_velocities(both, v[:, :2], v[:, 2])
        else:
            single_velocities(w, both, v, 3)
        w.apply_force(n, (5.0, 0.0), 0.5)
    s = a.body_states()
    assert (s["vx"][n], s["vy"][n], s["w"][n]) == (2.0, -1.0, 3.0), "the new body did not keep the batch's velocity"
    same(a, b, "a new body", contacts=False)
    step_and_compare(a, b, "a new body", 2)
    a.close()
    b.close()


def _check(rc):
    assert rc == 0, b2hip.lib().b2hip_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
def test_two_batched_force_calls_add_and_are_cleared_once(lazy):
    a, b, ids = twins(lazy)
    x = awake_body(a, ids)
    first = batch_of(a, ids, 63, 45)
    second = batch_of(a, ids, 65, 46)
    for bodies in (first, second):
        if x not in bodies:
            bodies[0] = x
    p, q = pushes_of(a, first, 6, 40.0), pushes_of(a, second, 7, 40.0)
    a.apply_forces(first, p)
    a.apply_forces(second, q)
    single_forces(b, first, p, 1)
    single_forces(b, second, q, 1)
    a.step()
    b.step()
    same(a, b, "two batched force calls, step 1")
    # ... and against a world that got only the second call: the first one's force was not replaced
    c, _ = build_world(lazy=lazy)
    c.apply_forces(second, q)
    c.step()
    assert c.body_states()[x].tobytes() != a.body_states()[x].tobytes(), "the second call replaced the first call's force"
    c.close()
    # the forces were cleared once and only once: the second step is the twin's
    step_and_compare(a, b, "after the forces were cleared", 1)
    # ... and a single force on a body of the batches starts from zero again
    for w in (a, b):
        w.apply_force(x, (2.0, 30.0), 0.125)
    step_and_compare(a, b, "a single force a step after the batches", 2)
    a.close()
    b.close()


@pytest.mark.gpu
def test_body_states_of_equals_the_rows_of_the_table():
    a, ids = build_world(lazy=True)
    rng = np.random.default_rng(11)
    bodies = rng.permutation(a.body_count).astype(np.int32)
    bodies = np.concatenate([bodies, bodies[:40], bodies[5:6]])  # (a read: ids may occur again)
    got = a.body_states_of(bodies)  # directly after a step, the table still on the device
    assert got.tobytes() == a.body_states()[bodies].tobytes()
    a.step()
    grid = np.asarray(ids["grid"], np.int32)
    a.set_velocities(grid[::3], (0.5, 1.0), 0.25)
    got = a.body_states_of(bodies)  # directly after a write call
    table = a.body_states()
    assert got.tobytes() == table[bodies].tobytes()
    assert (table["vy"][grid[::3]] == 1.0).all()
    assert a.body_states_of(np.zeros(0, np.int32)).shape == (0,)
    a.close()


@pytest.mark.gpu
def test_refused_calls_apply_nothing():
    a, b, ids = twins()
    n = a.body_count
    victim = ids["grid"][7]
    for w in (a, b):
        w.destroy_body(victim)
    before = a.body_states()
    good = np.asarray(ids["grid"][20:30], np.int32)
    p = pushes_of(a, good, 1, 40.0)
    v = np.ones((len(good), 2), f32)

    def refused(bodies, words):
        bodies = np.asarray(bodies, np.int32)
        for call in (lambda: a.apply_forces(bodies, p), lambda: a.apply_impulses(bodies, p), lambda: a.set_velocities(bodies, v)):
            with pytest.raises(b2hip.B2HipError) as e:
                call()
            for word in words:
                assert word in str(e.value), (word, str(e.value))
        assert a.body_states().tobytes() == before.tobytes()

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
    with pytest.raises(b2hip.B2HipError) as e:
        a.body_states_of(bad)
    assert "entry 3" in str(e.value)
    # inside a step
    _check(a.L.b2hip_step_begin(a.p, C.c_float(1.0 / 60.0), 8, 3))
    for call in (lambda: a.apply_forces(good, p), lambda: a.apply_impulses(good, p), lambda: a.set_velocities(good, v),
                 lambda: a.body_states_of(good)):
        with pytest.raises(b2hip.B2HipError) as e:
            call()
        assert "inside a step" in str(e.value)
    for fn in ("b2hip_collide", "b2hip_solve", "b2hip_sync_fixtures", "b2hip_find_new_contacts", "b2hip_solve_toi", "b2hip_step_end"):
        _check(getattr(a.L, fn)(a.p))
    b.step()
    same(a, b, "a step after the refused calls")
    # n == 0 succeeds
    none = np.zeros(0, np.int32)
    a.apply_forces(none, np.zeros(0, b2hip.BODY_PUSH_DTYPE))
    a.apply_impulses(none, np.zeros((0, 2), f32))
    a.set_velocities(none, np.zeros((0, 2), f32))
    step_and_compare(a, b, "after the empty calls", 1)
    a.close()
    b.close()


@pytest.mark.gpu
def test_a_snapshot_carries_the_batched_writes():
    a, b, ids = twins()
    bodies = batch_of(a, ids, 257, 51)
    p, q = pushes_of(a, bodies, 8, 40.0), pushes_of(a, bodies, 9, 1.0)
    a.apply_forces(bodies, p)
    a.apply_impulses(bodies, q)
    single_forces(b, bodies, p, 1)
    single_impulses(b, bodies, q, 1)
    r = b2hip.World.from_snapshot(a.save_snapshot())
    same(r, b, "the restored world", contacts=False)
    x = awake_body(b, ids)
    for w in (r, b, a):  # (a single force on top: the restored host mirror knows the batch's forces)
        w.apply_force(x, (1.0, 2.0), 0.5)
    r.step()
    b.step()
    a.step()
    same(r, b, "one step of the restored world")
    same(a, b, "one step of the world the snapshot was taken of")
    assert r.body_states().tobytes() != control(1).tobytes()
    for w in (a, b, r):
        w.close()
