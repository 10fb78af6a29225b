"""GPU: batched teleports and sleep / wake sets on the device (include/b2hip.h, block H: b2hip_set_transforms, b2hip_set_awakes).

The reference is the project's own single-body path - b2hip_set_transform and b2hip_set_awake, made entry by entry as the
header's definition by equivalence says - run on a TWIN world: built by the same script and stepped the same number of times.
Every comparison is bit for bit: tobytes() of body_states(), of the fat AABBs of the live proxies (b2hip_get_fat_aabbs, after
a read that uploads the single route's pending edits: that call itself does not upload them) and of contacts() after
stepping. One hand-made world of 330 bodies serves all tests but the continuous one; each test asserts that its batch holds
what it is about."""
import ctypes as C

import numpy as np
import pytest

import b2hip

AWAKE = 4          # b2hip_body_state.flags: the awake bit
SETTLE_STEPS = 40  # the stacks that were put down have gone to sleep, the ones that were dropped are still awake
STACKS, LEVELS, DROPPED_FROM = 80, 4, 64  # the 16 x 20 grid as 80 stacks of 4; stacks 64.. start 1.5 m up
EXTENSION = np.float32(0.1)  # B2D_AABB_EXTENSION (b2_aabbExtension)
ERR_UNSUPPORTED = -4
f32 = np.float32
PI = f32(np.pi)
ANGLES = np.asarray([0.0, -0.0, 1e-5, PI, -PI, -2.5, 200.0], f32)  # (200: the large-argument path of the sine and cosine)


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


def build_world(lazy=False, steps=SETTLE_STEPS, inactive=True):
    """a static ground; a 16 x 20 grid of small dynamic boxes and circles on it, as 80 stacks of four of which the last 16
    are dropped from 1.5 m; a kinematic body; a fixed-rotation body; a body with two fixtures; a weightless body far away;
    an inactive body; a body with three fixtures whose centre of mass is off its origin; two boxes joined by a revolute joint.
    Sleep is allowed; stepped until the stacks that were put down sleep. inactive=False leaves the inactive body active (and
    ids["inactive"] is -1: no such body).
    Returns (world, names -> body ids; "fixtures": body id -> its fixture ids)."""
    w = b2hip.World(allow_sleep=True)
    if lazy:
        w.set_lazy_readback(True)
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
        _check(w.L.b2hip_set_active(w.p, ids["inactive"], 0))
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


def twins(lazy=False, inactive=True):
    a, ids = build_world(lazy=lazy, inactive=inactive)
    b, _ = build_world(lazy=lazy, inactive=inactive)
    return a, b, ids


def live_fixtures(ids, but=()):
    """the fixtures that have a proxy: every one but those of the inactive body (and of the bodies of `but`)"""
    out = [f for body, fs in ids["fixtures"].items() if body != ids["inactive"] and body not in but for f in fs]
    return np.asarray(sorted(out), np.int64)


def fat_aabbs(w):
    """every fixture's fat AABB as the device holds it once the pending edits are uploaded (the read of one row does that)"""
    w.body_states_of(np.zeros(1, np.int32))
    n = w.L.b2hip_fixture_count(w.p)
    out = np.zeros((n, 4), f32)
    _check(w.L.b2hip_get_fat_aabbs(w.p, 0, n, out.ctypes.data_as(C.c_void_p)))
    return out


def same(a, b, what, ids=None, contacts=True):
    sa, sb = a.body_states(), b.body_states()
    if sa.tobytes() != sb.tobytes():
        bad = [n for n in sa.dtype.names if sa[n].tobytes() != sb[n].tobytes()]
        who = np.flatnonzero(np.any([sa[n].view(np.uint32) != sb[n].view(np.uint32) for n in sa.dtype.names], axis=0))
        raise AssertionError("%s: body states differ in %s, bodies %s" % (what, bad, who[:8].tolist()))
    assert not any(np.isnan(sa[n]).any() for n in sa.dtype.names if n != "flags"), "%s: NaN in the states" % what
    if ids is not None:
        live = live_fixtures(ids)
        fa, fb = fat_aabbs(a)[live], fat_aabbs(b)[live]
        if fa.tobytes() != fb.tobytes():
            who = live[np.flatnonzero(np.any(fa.view(np.uint32) != fb.view(np.uint32), axis=1))]
            raise AssertionError("%s: fat AABBs differ, fixtures %s" % (what, who[:8].tolist()))
    if contacts:
        assert a.contacts().tobytes() == b.contacts().tobytes(), "%s: contacts differ" % what


def step_and_compare(a, b, what, ids, steps=3):
    for k in range(steps):
        a.step()
        b.step()
        same(a, b, "%s, step %d" % (what, k + 1), ids)


def asleep(w):
    return (w.body_states()["flags"] & AWAKE) == 0


def grid_sleeping_and_awake(w, ids):
    sl = asleep(w)
    grid = np.asarray(ids["grid"])
    sleeping, awake = grid[sl[grid]], grid[~sl[grid]]
    assert len(sleeping) > 0 and len(awake) > 0, "the world holds %d sleeping and %d awake grid bodies" % (len(sleeping), len(awake))
    return sleeping, awake


def batch_of(w, ids, size, seed):
    """`size` body ids in a shuffled order; from 63 on the batch holds the static ground, the kinematic body, the
    three-fixture body, the inactive body, a body of the jointed pair, a sleeping and an awake body of the grid.
    A batch of one is the three-fixture body."""
    n = w.body_count
    sleeping, awake = grid_sleeping_and_awake(w, ids)
    rng = np.random.default_rng(seed)
    if size == 1:
        return np.asarray([ids["three"]], np.int32)
    must = [ids["ground"], ids["kinematic"], ids["three"], ids["inactive"], ids["pair"][0], int(sleeping[0]), int(awake[0])]
    must = [m for m in must if m >= 0]
    rest = np.setdiff1d(np.arange(n), must)
    bodies = np.concatenate([must, rng.permutation(rest)[:size - len(must)]]).astype(np.int32)
    bodies = rng.permutation(bodies)
    assert len(bodies) == min(size, n) and len(np.unique(bodies)) == len(bodies)
    sl = asleep(w)
    for name in ("ground", "kinematic", "three", "inactive"):
        assert ids[name] in bodies or ids[name] < 0, name
    assert sl[bodies].any() and (~sl[bodies]).any()
    return bodies


def poses_of(w, ids, bodies, seed):
    """(pose3, kind) for `bodies`, four kinds of displacement dealt in turn: 0 - 0.03 m sideways at the body's own angle (its
    proxies stay inside their fat boxes: nothing is buffered); 1 - exactly the AABB extension; 2 - 4.9 m sideways, seven
    stacks on, onto another stack; 3 - far away. Kinds 1 to 3 take their angles from ANGLES in turn. The ground moves by the
    extension and keeps its angle, so that the stacks keep something to stand on."""
    s = w.body_states()[bodies]
    n = len(bodies)
    kind = (np.arange(n) + seed) % 4
    if n == 1:
        kind[:] = 2
    kind[bodies == ids["ground"]] = 1
    pose = np.zeros((n, 3), f32)
    step = np.asarray([0.03, EXTENSION, 4.9, 0.0], f32)
    pose[:, 0] = s["px"] + step[kind]
    pose[:, 1] = s["py"]
    pose[:, 2] = ANGLES[(np.arange(n) + seed) % len(ANGLES)]
    keep = (kind == 0) | (bodies == ids["ground"])
    pose[keep, 2] = s["angle"][keep]
    far = kind == 3
    pose[far, 0] = 200.0 + 2.0 * np.arange(n)[far]
    pose[far, 1] = 300.0
    if n > 1:
        assert all((kind == k).any() for k in range(4))
        used = pose[~keep, 2]
        assert all((used.view(np.uint32) == a.view(np.uint32)).any() for a in ANGLES.reshape(-1, 1)), "an angle of ANGLES is missing"
    return pose, kind


def batched_transforms(w, bodies, pose3, mask):
    bodies = np.ascontiguousarray(bodies, np.int32)
    pose3 = np.ascontiguousarray(pose3, f32)
    return w.L.b2hip_set_transforms(w.p, len(bodies), bodies.ctypes.data_as(C.c_void_p), pose3.ctypes.data_as(C.c_void_p), mask)


def single_transforms(w, bodies, pose3, mask):
    s = w.body_states()
    for b, p in zip(np.asarray(bodies).tolist(), pose3):
        x, y = (p[0], p[1]) if mask & 1 else (s["px"][b], s["py"][b])
        a = p[2] if mask & 2 else s["angle"][b]
        w.set_transform(b, (float(x), float(y)), float(a))


def single_awakes(w, bodies, flags):
    for b, f in zip(np.asarray(bodies).tolist(), np.broadcast_to(flags, (len(bodies),)).tolist()):
        w.set_awake(b, bool(f))


SIZES = (1, 63, 64, 65, 257, 0)  # 0: every body


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
@pytest.mark.parametrize("size", SIZES)
def test_transforms_equal_the_single_calls_on_a_twin(size, lazy):
    a, b, ids = twins(lazy)
    bodies = batch_of(a, ids, size or a.body_count, 10 + size)
    pose, kind = poses_of(a, ids, bodies, size)
    before_states, before_fat = b.body_states(), fat_aabbs(b)
    _check(batched_transforms(a, bodies, pose, 3))
    single_transforms(b, bodies, pose, 3)
    same(a, b, "after the call", ids, contacts=False)
    s, fat = b.body_states(), fat_aabbs(b)
    assert s["px"][bodies].tobytes() == pose[:, 0].tobytes() and s["angle"][bodies].tobytes() == pose[:, 2].tobytes()
    moved = np.any(fat.view(np.uint32) != before_fat.view(np.uint32), axis=1)
    assert moved[live_fixtures(ids)].any(), "no proxy left its fat box"
    if size != 1:
        stayed = [f for bd in bodies[kind == 0].tolist() if bd != ids["inactive"] for f in ids["fixtures"][bd] if not moved[f]]
        assert stayed, "no proxy of a nudged body stayed inside its fat box"
        assert (s["px"][bodies[kind == 0]] != before_states["px"][bodies[kind == 0]]).all()
        assert s["py"][ids["inactive"]] == pose[int(np.flatnonzero(bodies == ids["inactive"])[0]), 1]
    step_and_compare(a, b, "transforms", ids)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", (1, 2))
def test_masks_leave_the_other_half_alone(mask):
    a, b, ids = twins()
    bodies = batch_of(a, ids, 65, 21)
    pose, _ = poses_of(a, ids, bodies, 2)
    before = a.body_states()
    sent = pose.copy()
    if mask == 1:
        sent[:, 2] = np.nan
    else:
        sent[:, :2] = np.nan
    _check(batched_transforms(a, bodies, sent, mask))
    single_transforms(b, bodies, pose, mask)
    s = a.body_states()
    if mask == 1:
        assert s["angle"][bodies].tobytes() == before["angle"][bodies].tobytes() and s["px"][bodies].tobytes() == pose[:, 0].tobytes()
    else:
        assert s["px"][bodies].tobytes() == before["px"][bodies].tobytes() and s["angle"][bodies].tobytes() == pose[:, 2].tobytes()
    same(a, b, "mask %d, after the call" % mask, ids, contacts=False)
    step_and_compare(a, b, "mask %d" % mask, ids)
    # ... and the Python wrapper derives the same mask from what it is given
    pose2, _ = poses_of(a, ids, bodies, 3)
    if mask == 1:
        a.set_transforms(bodies, position=pose2[:, :2])
    else:
        a.set_transforms(bodies, angle=pose2[:, 2])
    single_transforms(b, bodies, pose2, mask)
    same(a, b, "mask %d through World.set_transforms" % mask, ids, contacts=False)
    step_and_compare(a, b, "mask %d through World.set_transforms" % mask, ids, 1)
    a.close()
    b.close()


@pytest.mark.gpu
def test_a_teleport_changes_the_pose_and_nothing_else():
    a, b, ids = twins()
    sleeping, _ = grid_sleeping_and_awake(a, ids)
    for w in (a, b):  # (a stack at rest, woken: awake with a sleep timer that runs)
        w.set_awake(int(sleeping[-1]), True)
        for _ in range(5):
            w.step()
    sleeping, awake = grid_sleeping_and_awake(a, ids)
    before = a.body_states()
    mover = int(awake[np.argmax(np.abs(before["vy"][awake]))])
    resting = int(awake[np.argmax(before["sleep_time"][awake])])
    assert before["vy"][mover] != 0.0, "no awake body moves"
    assert before["sleep_time"][resting] > 0.0 and resting != mover, "no awake body has a running sleep timer"
    bodies = np.asarray([int(sleeping[0]), mover, ids["kinematic"], resting], np.int32)
    pose = np.asarray([[-20.0, 12.0, 0.5], [-10.0, 14.0, -2.5], [0.0, 16.0, 200.0], [10.0, 18.0, 1e-5]], f32)
    a.set_transforms(bodies, pose[:, :2], pose[:, 2])
    single_transforms(b, bodies, pose, 3)
    s = a.body_states()
    for name in ("vx", "vy", "w", "flags", "sleep_time"):
        assert s[name][bodies].tobytes() == before[name][bodies].tobytes(), name
    assert (s["flags"][bodies[0]] & AWAKE) == 0 and s["sleep_time"][resting] == before["sleep_time"][resting]
    assert s["px"][bodies].tobytes() == pose[:, 0].tobytes() and s["py"][bodies].tobytes() == pose[:, 1].tobytes()
    others = np.setdiff1d(np.arange(a.body_count), bodies)
    assert s[others].tobytes() == before[others].tobytes(), "a body nobody named changed"
    same(a, b, "after the call", ids, contacts=False)
    a.step()
    b.step()
    same(a, b, "step 1", ids)
    assert (a.body_states()["flags"][bodies[0]] & AWAKE) == 0, "the sleeping body woke in mid-air: it must stay asleep"
    step_and_compare(a, b, "a teleport", ids, 2)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
def test_awakes_equal_the_single_calls_on_a_twin(lazy):
    a, b, ids = twins(lazy)
    sleeping, awake = grid_sleeping_and_awake(a, ids)
    before = a.body_states()
    bodies = np.concatenate([sleeping[:40], awake[:40], [ids["ground"], ids["kinematic"], ids["far"], ids["inactive"], ids["three"]],
                             ids["pair"]]).astype(np.int32)
    bodies = np.random.default_rng(3).permutation(bodies)
    flags = (np.arange(len(bodies)) % 3 != 0)
    sl = asleep(a)[bodies]
    for want_sleeping in (False, True):
        for want_flag in (False, True):
            assert ((sl == want_sleeping) & (flags == want_flag)).any()
    assert (np.abs(before["vy"][bodies[~flags]]) > 0).any(), "no moving body is put to sleep"
    a.set_awakes(bodies, flags)
    single_awakes(b, bodies, flags)
    s = a.body_states()
    assert ((s["flags"][bodies] & AWAKE) != 0).tolist() == flags.tolist()
    assert (s["sleep_time"][bodies] == 0).all() and (s["vy"][bodies[~flags]] == 0).all() and (s["w"][bodies[~flags]] == 0).all()
    assert s["vx"][ids["kinematic"]] == (0.25 if flags[int(np.flatnonzero(bodies == ids["kinematic"])[0])] else 0.0)
    same(a, b, "after the call", ids, contacts=False)
    step_and_compare(a, b, "awakes", ids)
    # a scalar broadcasts
    a.set_awakes(bodies[:65], False)
    single_awakes(b, bodies[:65], False)
    same(a, b, "awake = False for all", ids, contacts=False)
    a.set_awakes(bodies[10:30])
    single_awakes(b, bodies[10:30], True)
    step_and_compare(a, b, "awake scalars", ids, 2)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
def test_a_single_wake_after_a_batch_that_put_the_ground_to_sleep(lazy):
    """b2hip_set_awake(w, ground, 1) leaves a static body that is awake already untouched, and decides that from the host's
    copy of the flag: a batch that put the ground to sleep must have cleared that copy too, or the single call does nothing
    and the ground stays asleep. The other way round - woken by a batch, put to sleep by the single call - as well."""
    a, b, ids = twins(lazy)
    ground = ids["ground"]
    sleeping, awake = grid_sleeping_and_awake(a, ids)
    bodies = np.asarray([int(awake[0]), ground, int(sleeping[0]), ids["kinematic"]], np.int32)
    assert (a.body_states()["flags"][ground] & AWAKE) != 0, "the ground starts awake"
    a.set_awakes(bodies, False)
    single_awakes(b, bodies, False)
    assert (a.body_states()["flags"][ground] & AWAKE) == 0
    same(a, b, "the ground put to sleep", ids, contacts=False)
    for w in (a, b):
        w.set_awake(ground, True)
    assert (a.body_states()["flags"][ground] & AWAKE) != 0, "the single call believed a stale flag"
    same(a, b, "the ground woken by the single call", ids, contacts=False)
    step_and_compare(a, b, "single wake after the batch", ids, 2)
    for w in (a, b):
        w.set_awake(ground, False)
    a.set_awakes(bodies, True)
    single_awakes(b, bodies, True)
    same(a, b, "the ground woken by the batch", ids, contacts=False)
    for w in (a, b):
        w.set_awake(ground, True)   # (awake already: untouched)
        w.set_awake(int(bodies[0]), False)
    same(a, b, "single calls after the waking batch", ids, contacts=False)
    step_and_compare(a, b, "single calls after the waking batch", ids, 2)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ("force after sleep", "sleep after forces"))
def test_awakes_and_forces_keep_their_order(order):
    a, b, ids = twins()
    _, awake = grid_sleeping_and_awake(a, ids)
    bodies = awake[:33].astype(np.int32)
    x = int(bodies[5])
    if order == "force after sleep":
        a.set_awakes(bodies, False)
        single_awakes(b, bodies, False)
        for w in (a, b):
            w.apply_force(x, (3.0, 40.0), 0.25)
        s = a.body_states()
        assert (s["flags"][x] & AWAKE) != 0 and (s["flags"][bodies[6]] & AWAKE) == 0
    else:
        push = np.zeros(len(bodies), b2hip.BODY_PUSH_DTYPE)
        push["x"], push["y"], push["angular"] = 3.0, 40.0, 0.25
        a.apply_forces(bodies, push)
        for q in bodies.tolist():
            b.apply_force(q, (3.0, 40.0), 0.25)
        a.set_awakes(bodies[::2], False)
        single_awakes(b, bodies[::2], False)
    same(a, b, order + ", before the step", ids, contacts=False)
    step_and_compare(a, b, order, ids)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("after set_velocities", "single after the batch", "two batches", "a new body"))
def test_transforms_keep_their_order_with_other_edits(case):
    a, b, ids = twins()
    bodies = batch_of(a, ids, 64, 31)
    pose, _ = poses_of(a, ids, bodies, 1)
    _, awake = grid_sleeping_and_awake(a, ids)
    x = int(awake[0])
    assert x in bodies
    if case == "after set_velocities":
        v3 = np.random.default_rng(4).uniform(-2.0, 2.0, (len(bodies), 3)).astype(f32)
        a.set_velocities(bodies, v3[:, :2], v3[:, 2])
        b.set_velocities(bodies, v3[:, :2], v3[:, 2])
        _check(batched_transforms(a, bodies, pose, 3))
        single_transforms(b, bodies, pose, 3)
        k = int(np.flatnonzero(bodies == x)[0])
        s = a.body_states()
        assert (s["vx"][x], s["vy"][x], s["w"][x]) == tuple(v3[k]) and s["px"][x] == pose[k, 0]
    elif case == "single after the batch":
        _check(batched_transforms(a, bodies, pose, 3))
        single_transforms(b, bodies, pose, 3)
        for w in (a, b):
            w.set_transform(x, (-27.5, 6.0), 0.5)
            w.set_transform(ids["three"], (-20.0, 9.0), -1.0)
        assert a.body_states()["py"][x] == 6.0
    elif case == "two batches":
        second = batch_of(a, ids, 65, 32)
        pose2, _ = poses_of(a, ids, second, 2)  # (from the states before either batch, for both worlds)
        assert len(np.intersect1d(bodies, second)) > 7
        _check(batched_transforms(a, bodies, pose, 3))
        _check(batched_transforms(a, second, pose2, 1))
        single_transforms(b, bodies, pose, 3)
        single_transforms(b, second, pose2, 1)
    else:
        for w in (a, b):
            n = w.create_body(b2hip.DYNAMIC, (-20.0, 8.0))
            f = w.create_fixture(n, b2hip.box_shape(0.25, 0.25), density=1.0)
        ids["fixtures"][n] = [f]
        both = np.asarray([x, n], np.int32)
        p2 = np.asarray([[-27.5, 6.0, 0.5], [-10.15, 0.3, 0.25]], f32)  # (the new body lands in a stack)
        _check(batched_transforms(a, both, p2, 3))
        single_transforms(b, both, p2, 3)
        assert a.body_states()["px"][n] == p2[1, 0]
    same(a, b, case + ", before the step", ids, contacts=False)
    step_and_compare(a, b, case, ids)
    a.close()
    b.close()


@pytest.mark.gpu
def test_queries_see_the_batch_before_any_step():
    a, b, ids = twins()
    bodies = batch_of(a, ids, 257, 41)
    pose, kind = poses_of(a, ids, bodies, 3)
    before = a.body_states()
    p1 = np.stack([pose[:, 0], pose[:, 1] + 3.0], axis=1)  # (down on every body where it is now: from above its new place)
    p2 = np.stack([pose[:, 0], pose[:, 1] - 3.0], axis=1)
    lower, upper = pose[:, :2] - 0.4, pose[:, :2] + 0.4
    hits_before = a.ray_cast_closest(p1, p2)
    _check(batched_transforms(a, bodies, pose, 3))
    single_transforms(b, bodies, pose, 3)
    ha, hb = a.ray_cast_closest(p1, p2), b.ray_cast_closest(p1, p2)
    assert ha.tobytes() == hb.tobytes(), "ray_cast_closest differs"
    assert ha.tobytes() != hits_before.tobytes(), "the rays see the world as it was before the batch"
    far = np.flatnonzero((kind == 3) & (bodies != ids["inactive"]))
    assert (ha["body"][far] == bodies[far]).all(), "a ray down on a body that was sent far away misses it"
    (oa, ia), (ob, ib) = a.query_aabbs(lower, upper), b.query_aabbs(lower, upper)
    assert oa.tobytes() == ob.tobytes() and ia.tobytes() == ib.tobytes(), "query_aabbs differs"
    assert all(bodies[k] in ia["body"][oa[k]:oa[k + 1]] for k in far)
    assert a.body_states().tobytes() != before.tobytes()
    same(a, b, "after the queries", ids, contacts=False)
    step_and_compare(a, b, "after the queries", ids)
    a.close()
    b.close()


@pytest.mark.gpu
def test_a_snapshot_carries_the_batch():
    """(the world without its inactive body: a snapshot of a world that holds a deactivated body is not loaded - its fixtures
    have no proxy id, which the loader takes for corruption - whoever moved the bodies)"""
    a, b, ids = twins(inactive=False)
    bodies = batch_of(a, ids, 257, 51)
    pose, _ = poses_of(a, ids, bodies, 1)
    flags = np.arange(len(bodies)) % 2 == 0
    _check(batched_transforms(a, bodies, pose, 3))
    a.set_awakes(bodies, flags)
    single_transforms(b, bodies, pose, 3)
    single_awakes(b, bodies, flags)
    r = b2hip.World.from_snapshot(a.save_snapshot())
    same(r, b, "the restored world", ids, contacts=False)
    for k in range(3):
        r.step()
        b.step()
        a.step()
        same(r, b, "step %d of the restored world" % (k + 1), ids)
        same(a, b, "step %d of the world the snapshot was taken of" % (k + 1), ids)
    for w in (a, b, r):
        w.close()


def bullet_world():
    """a thin static wall, a floor, and a fast bullet on its way to the wall; continuous physics on"""
    w = b2hip.World(gravity=(0.0, -10.0), allow_sleep=True, continuous=True)
    ground = w.create_body(b2hip.STATIC, (0.0, -0.5))
    w.create_fixture(ground, b2hip.box_shape(40.0, 0.5))
    wall = w.create_body(b2hip.STATIC, (10.0, 2.0))
    w.create_fixture(wall, b2hip.box_shape(0.05, 2.0))
    bullet = w.create_body(b2hip.DYNAMIC, (-20.0, 1.0), velocity=(100.0, 0.0), bullet=True, gravity_scale=0.0)
    w.create_fixture(bullet, b2hip.circle_shape(0.1), density=1.0, restitution=0.5)
    crate = w.create_body(b2hip.DYNAMIC, (12.0, 0.25))
    w.create_fixture(crate, b2hip.box_shape(0.25, 0.25), density=1.0)
    for _ in range(2):
        w.step()
    return w, bullet, wall


@pytest.mark.gpu
def test_a_bullet_teleported_in_mid_flight_still_meets_the_wall():
    (a, bullet, wall), (b, _, _) = bullet_world(), bullet_world()
    s = a.body_states()
    assert s["vx"][bullet] == 100.0 and -17.5 < s["px"][bullet] < -16.0, "the bullet is not in mid-flight"
    bodies = np.asarray([bullet], np.int32)
    pose = np.asarray([[7.0, 2.5, 0.25]], f32)  # (one and a bit steps in front of the wall, on another height)
    _check(batched_transforms(a, bodies, pose, 3))
    single_transforms(b, bodies, pose, 3)
    same(a, b, "after the call", contacts=False)
    for k in range(5):
        a.step()
        b.step()
        same(a, b, "continuous, step %d" % (k + 1))
    s = a.body_states()
    assert s["px"][bullet] < 10.0 and s["vx"][bullet] < 0.0, "the bullet went through the wall"
    a.close()
    b.close()


@pytest.mark.gpu
def test_refused_calls_name_the_offender_and_apply_nothing():
    a, b, ids = twins()
    n = a.body_count
    victim = ids["grid"][7]
    for w in (a, b):
        w.destroy_body(victim)
    before = a.body_states()
    good = np.asarray(ids["grid"][20:30], np.int32)
    pose = np.zeros((len(good), 3), f32)
    pose[:, 1] = 20.0

    def refused(bodies, words):
        bodies = np.asarray(bodies, np.int32)
        for call in (lambda: a.set_transforms(bodies, pose[:, :2], pose[:, 2]), lambda: a.set_transforms(bodies, angle=1.0),
                     lambda: a.set_awakes(bodies, False)):
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
    # inside a step
    _check(a.L.b2hip_step_begin(a.p, C.c_float(1.0 / 60.0), 8, 3))
    for call in (lambda: a.set_transforms(good, pose[:, :2]), lambda: a.set_awakes(good)):
        with pytest.raises(b2hip.B2HipError) as e:
            call()
        assert "inside a step" in str(e.value)
    for fn in ("b2hip_collide", "b2hip_solve", "b2hip_sync_fixtures", "b2hip_find_new_contacts", "b2hip_solve_toi", "b2hip_step_end"):
        _check(getattr(a.L, fn)(a.p))
    b.step()
    same(a, b, "a step after the refused calls")
    # n == 0 succeeds
    none = np.zeros(0, np.int32)
    a.set_transforms(none, np.zeros((0, 2), f32))
    a.set_awakes(none, np.zeros(0, bool))
    a.step()
    b.step()
    same(a, b, "after the empty calls")
    a.close()
    b.close()


@pytest.mark.gpu
def test_the_move_buffer_is_guarded():
    a, b, ids = twins()
    n = a.body_count
    bodies = np.random.default_rng(7).permutation(n).astype(np.int32)
    s0 = a.body_states()[bodies]
    there = np.stack([s0["px"] + 300.0, s0["py"] + 50.0, s0["angle"]], axis=1).astype(f32)
    back = np.stack([s0["px"], s0["py"], s0["angle"]], axis=1).astype(f32)
    refusals = 0
    for k in range(8):
        pose = there if k % 2 == 0 else back
        before = a.body_states()
        rc = batched_transforms(a, bodies, pose, 3)
        if k == 0:
            assert rc == 0, "one batch over every body of a freshly stepped world must fit"
        if rc == 0:
            single_transforms(b, bodies, pose, 3)
            continue
        refusals += 1
        assert rc == ERR_UNSUPPORTED, rc
        msg = a.L.b2hip_last_error().decode()
        assert "step" in msg and "move buffer" in msg, msg
        assert a.body_states().tobytes() == before.tobytes(), "a refused call changed the states"
    if refusals == 0:
        pytest.skip("all 8 teleports of every body fitted: the host must have grown the move buffer")
    same(a, b, "after the calls that were accepted", ids, contacts=False)
    a.step()
    b.step()
    same(a, b, "step 1", ids)
    _check(batched_transforms(a, bodies, there, 3))  # (the step emptied the buffer)
    single_transforms(b, bodies, there, 3)
    step_and_compare(a, b, "after the guard", ids, 2)
    a.close()
    b.close()
