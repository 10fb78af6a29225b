"""GPU: batched joint motor targets and joint state reads on the device (include/b2hip.h, block G).

Writes: the reference is the project's own single-joint path - b2hip_joint_set_motor made entry by entry, as the header's
definition by equivalence says - run on a TWIN world: built by the same script and stepped the same number of times. Every
comparison is bit for bit: tobytes() of body_states(), of joint_states(every joint) and of contacts(), at once and after 1 and
3 steps. Reads: the reaction and the limit state against the single-joint calls bit for bit, the angular values against
float32 differences of body_states() bit for bit, translations, linear speeds and pulley lengths against the float64
reference of tests/joints_ref.py within 32 * 2^-24 * S. One hand-made world serves all tests; each test asserts that its batch
holds what it is about."""
import ctypes as C
import math

import numpy as np
import pytest

import b2hip
import joints_ref as jr

AWAKE = 4           # b2hip_body_state.flags: the awake bit
SETTLE_STEPS = 150  # the chain, the undriven cars and the hanging arms sleep; the driven cars, sliders and arms are at work
f32 = np.float32
REVOLUTE, DISTANCE, PRISMATIC, WELD, WHEEL, ROPE, FRICTION, MOTOR, PULLEY, MOUSE, GEAR = range(11)
LINKS, SLIDERS, CARS, ARMS = 40, 10, 8, 192
COS30, SIN30 = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))


def box_at(hx, hy, cx, cy):
    """a box fixture shape centred at (cx, cy) of its body"""
    s = b2hip.box_shape(hx, hy)
    for i in range(4):
        s.verts[2 * i] += cx
        s.verts[2 * i + 1] += cy
    s.centroid[0], s.centroid[1] = cx, cy
    return s


class Scene:
    """what the script made: names -> ids, every joint's definition, and the motor values each motor joint has now"""

    def __init__(self):
        self.ids = {}
        self.defs = {}   # joint id -> dict(type, body_a, body_b, anchor_a, anchor_b, ...)
        self.cur = {}    # motor joint id -> [enable, speed, max]

    def joint(self, j, type, a, b, motor=None, **more):
        self.defs[j] = dict(type=type, body_a=a, body_b=b, **more)
        if motor is not None:
            self.cur[j] = [int(motor[0]), f32(motor[1]), f32(motor[2])]
        return j

    def copy_cur(self):
        return {j: list(v) for j, v in self.cur.items()}

    @property
    def motor_joints(self):
        return np.asarray(sorted(self.cur), np.int32)


def build_world(library=None, lazy=False, steps=SETTLE_STEPS):
    """A static ground (origin at the world's, so its local anchors are world points) and, within 50 m of the origin:
    a 40-link chain of limited revolute joints lying on the ground, motors off (it sleeps), its first link pinned to the ground;
    ten prismatic sliders on the ground body with motor and limits, every other axis turned by 30 degrees, the first five
      running into their limit, none allowed to sleep;
    eight cars with two wheel joints on one chassis: four undriven (they sleep), four driven; one driven wheel's centre of
      mass is off its origin;
    192 one-link arms pinned to the ground body: half of them hanging with motors off (they sleep), a quarter driven into
      their limit, a quarter turning freely;
    one each of distance, weld, rope, friction, motor, pulley, mouse and gear joints (the gear couples a revolute and a
      prismatic joint); one joint destroyed after ten steps; one prismatic joint created after the last step."""
    w = b2hip.World(allow_sleep=True, library=library)
    if lazy:
        w.set_lazy_readback(True)
    sc = Scene()
    ids = sc.ids
    g = ids["ground"] = w.create_body(b2hip.STATIC, (0.0, 0.0))
    w.create_fixture(g, box_at(50.0, 0.5, 0.0, -0.5))

    def dyn(pos, shape, density=1.0, ghost=False, **kw):
        b = w.create_body(b2hip.DYNAMIC, pos, **kw)
        w.create_fixture(b, shape, density=density, friction=0.6, category=2 if ghost else 1, mask=0 if ghost else 0xFFFF)
        return b

    # ---- the chain
    ids["links"], ids["chain"] = [], []
    for i in range(LINKS):
        b = dyn((-9.75 + 0.5 * i, 0.1), b2hip.box_shape(0.25, 0.1))
        a, anchor_a = (g, (-10.0, 0.1)) if i == 0 else (ids["links"][-1], (0.25, 0.0))
        j = w.create_revolute_joint(a, b, anchor_a, (-0.25, 0.0), 0.0, True, -0.5, 0.5, False, 0.0, 10.0)
        ids["links"].append(b)
        ids["chain"].append(sc.joint(j, REVOLUTE, a, b, (0, 0.0, 10.0), ref=0.0))
    # ---- the sliders
    ids["slider_bodies"], ids["sliders"] = [], []
    for i in range(SLIDERS):
        y = 2.0 + 0.6 * i
        b = dyn((0.0, y), b2hip.box_shape(0.2, 0.2), ghost=True, allow_sleep=False)
        axis = (1.0, 0.0) if i % 2 == 0 else (COS30, SIN30)
        speed = 0.5 if i % 2 == 0 else -0.5
        limit = 0.75 if i < 5 else 5.0
        j = w.create_prismatic_joint(g, b, (0.0, y), (0.0, 0.0), axis, 0.0, True, -limit, limit, True, speed, 100.0)
        ids["slider_bodies"].append(b)
        ids["sliders"].append(sc.joint(j, PRISMATIC, g, b, (1, speed, 100.0), anchor_a=(0.0, y), anchor_b=(0.0, 0.0), axis=axis))
    # ---- the cars
    ids["chassis"], ids["wheel_bodies"], ids["wheels"] = [], [], []
    for k in range(CARS):
        x = 14.0 + 4.0 * k if k < 4 else 32.0 + 3.5 * (k - 4)
        driven = k >= 4
        chassis = dyn((x, 0.9), b2hip.box_shape(1.0, 0.2))
        ids["chassis"].append(chassis)
        for side in (-1.0, 1.0):
            wheel = w.create_body(b2hip.DYNAMIC, (x + 0.7 * side, 0.3))
            w.create_fixture(wheel, b2hip.circle_shape(0.3), density=1.0, friction=0.9)
            if k == 4 and side < 0.0:
                w.create_fixture(wheel, box_at(0.1, 0.1, 0.15, 0.0), density=4.0, friction=0.9)
                ids["offcentre"] = wheel
            motor = (1, -3.0, 20.0) if driven else (0, 0.0, 10.0)
            j = w.create_wheel_joint(chassis, wheel, (0.7 * side, -0.6), (0.0, 0.0), (0.0, 1.0), 4.0, 1.0, *motor)
            ids["wheel_bodies"].append(wheel)
            ids["wheels"].append(sc.joint(j, WHEEL, chassis, wheel, motor, anchor_a=(0.7 * side, -0.6), anchor_b=(0.0, 0.0),
                                          axis=(0.0, 1.0)))
    # ---- the arms
    ids["arm_bodies"], ids["arms"] = [], []
    for k in range(ARMS):
        x, y = -46.0 + 4.0 * (k % 24), 10.0 + 1.5 * (k // 24)
        kind = k % 4
        b = dyn((x, y - 0.4), b2hip.box_shape(0.05, 0.4), ghost=True, allow_sleep=kind != 1)
        motor = {0: (0, 0.0, 5.0), 1: (1, 1.0, 50.0), 2: (0, 0.0, 5.0), 3: (1, -2.0, 50.0)}[kind]
        j = w.create_revolute_joint(g, b, (x, y), (0.0, 0.4), 0.0, kind != 3, -1.0, 1.0, *motor)
        ids["arm_bodies"].append(b)
        ids["arms"].append(sc.joint(j, REVOLUTE, g, b, motor, ref=0.0))
    # ---- one of each other type
    box = b2hip.box_shape(0.25, 0.25)
    b = dyn((-14.0, 3.0), box)
    ids["distance"] = sc.joint(w.create_distance_joint(g, b, (-14.0, 5.0), (0.0, 0.0), 2.0), DISTANCE, g, b)
    b = dyn((-17.0, 3.0), box)
    ids["weld"] = sc.joint(w.create_weld_joint(g, b, (-17.5, 3.0), (-0.5, 0.0), 0.0), WELD, g, b)
    b = dyn((-20.0, 3.0), box)
    ids["rope"] = sc.joint(w.create_rope_joint(g, b, (-20.0, 5.0), (0.0, 0.0), 1.9), ROPE, g, b)
    b = dyn((-23.0, 0.25), box, velocity=(2.0, 0.0))
    ids["friction"] = sc.joint(w.create_friction_joint(g, b, (-23.0, 0.25), (0.0, 0.0), 1.0, 1.0), FRICTION, g, b)
    b = dyn((-26.0, 2.0), box)
    ids["motor"] = sc.joint(w.create_motor_joint(g, b, (-26.0, 2.0), 0.0, 100.0, 100.0), MOTOR, g, b)
    pa, pb = dyn((-31.0, 2.0), box), dyn((-29.0, 2.0), box, density=1.2)
    ids["pulley"] = sc.joint(w.create_pulley_joint(pa, pb, (-31.0, 5.0), (-29.0, 5.0), (0.0, 0.0), (0.0, 0.0), 3.0, 3.0, 1.0), PULLEY, pa, pb,
                             anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), ground_a=(-31.0, 5.0), ground_b=(-29.0, 5.0))
    b = dyn((-35.0, 2.0), box)
    ids["mouse"] = sc.joint(w.create_mouse_joint(g, b, (-35.0, 3.0), 250.0), MOUSE, g, b)
    disc = dyn((-39.0, 2.0), b2hip.circle_shape(0.5))
    ids["gear_revolute"] = sc.joint(w.create_revolute_joint(g, disc, (-39.0, 2.0), (0.0, 0.0), 0.0, False, 0.0, 0.0, True, 0.3, 100.0),
                                    REVOLUTE, g, disc, (1, 0.3, 100.0), ref=0.0)
    b = dyn((-42.0, 2.0), box)
    ids["gear_prismatic"] = sc.joint(w.create_prismatic_joint(g, b, (-42.0, 2.0), (0.0, 0.0), (0.0, 1.0), 0.0, True, -1.0, 1.0, False, 0.0, 10.0),
                                     PRISMATIC, g, b, (0, 0.0, 10.0), anchor_a=(-42.0, 2.0), anchor_b=(0.0, 0.0), axis=(0.0, 1.0))
    ids["gear"] = sc.joint(w.create_gear_joint(ids["gear_revolute"], ids["gear_prismatic"], 1.0), GEAR, disc, b)
    spare = dyn((-45.0, 0.25), box)
    ids["destroyed"] = w.create_revolute_joint(g, spare, (-45.0, 0.25), (0.0, 0.0), 0.0, False, 0.0, 0.0, True, 1.0, 10.0)
    sc.defs[ids["destroyed"]] = dict(type=-1, body_a=g, body_b=spare)
    late = ids["late_body"] = dyn((-47.5, 0.25), box)
    for k in range(steps):
        if k == 10:
            w.destroy_joint(ids["destroyed"])
        w.step()
    if steps > 10:
        ids["late"] = sc.joint(w.create_prismatic_joint(g, late, (-48.25, 0.25), (0.0, 0.0), (1.0, 0.0), 0.0, False, 0.0, 0.0, False, 0.0, 10.0),
                               PRISMATIC, g, late, (0, 0.0, 10.0), anchor_a=(-48.25, 0.25), anchor_b=(0.0, 0.0), axis=(1.0, 0.0))
    return w, sc


def twins(lazy=False):
    a, sc = build_world(lazy=lazy)
    b, _ = build_world(lazy=lazy)
    return a, b, sc


def all_joints(w):
    return np.arange(w.joint_count, dtype=np.int32)


def snapshot_of(w):
    """what a caller can observe: the three byte strings every comparison is made of"""
    return w.body_states().tobytes(), w.joint_states(all_joints(w)).tobytes(), w.contacts().tobytes()


def same(a, b, what):
    sa, sb = a.body_states(), b.body_states()
    if sa.tobytes() != sb.tobytes():
        bad = [n for n in sa.dtype.names if sa[n].tobytes() != sb[n].tobytes()]
        who = np.flatnonzero(np.any([sa[n].view(np.uint32) != sb[n].view(np.uint32) for n in sa.dtype.names], axis=0))
        raise AssertionError("%s: body states differ in %s, bodies %s" % (what, bad, who[:8].tolist()))
    ja, jb = a.joint_states(all_joints(a)), b.joint_states(all_joints(b))
    if ja.tobytes() != jb.tobytes():
        who = [i for i in range(len(ja)) if ja[i].tobytes() != jb[i].tobytes()]
        raise AssertionError("%s: joint states differ at joints %s" % (what, who[:8]))
    assert a.contacts().tobytes() == b.contacts().tobytes(), "%s: contacts differ" % what


def step_and_compare(a, b, what):
    """at once, after 1 step and after 3"""
    same(a, b, "%s, at once" % what)
    a.step()
    b.step()
    same(a, b, "%s, step 1" % what)
    for _ in range(2):
        a.step()
        b.step()
    same(a, b, "%s, step 3" % what)


_control = {}


def control(lazy, k):
    """snapshot_of() of the world nobody touched, k = 0, 1 or 3 steps after the script (computed once, shared, never written)"""
    if lazy not in _control:
        w, _ = build_world(lazy=lazy)
        got = {0: snapshot_of(w)}
        w.step()
        got[1] = snapshot_of(w)
        w.step()
        w.step()
        got[3] = snapshot_of(w)
        w.close()
        _control[lazy] = got
    return _control[lazy][k]


_shared = []


def shared():
    """the world of the tests that only read: built once, never written"""
    if not _shared:
        _shared.extend(build_world())
    return _shared


def asleep(w):
    return (w.body_states()["flags"] & AWAKE) == 0


def joint_sleeps(sc, sl, j):
    """both bodies of the joint sleep, the static ground not counting"""
    d = sc.defs[int(j)]
    return all(sl[b] for b in (d["body_a"], d["body_b"]) if b != sc.ids["ground"])


def batch_of(w, sc, size, seed):
    """`size` motor-joint ids in a shuffled order. From 64 on the batch holds a joint of the sleeping chain, the joint that pins
    the chain to the static ground, both wheel joints of a sleeping car (they share the chassis) and of a driven one, a slider
    at work and the joint created after the last step. A batch of one is a joint of the sleeping chain."""
    ids = sc.ids
    sl = asleep(w)
    assert sl[ids["links"]].all(), "the chain does not sleep"
    assert sl[ids["chassis"][1]] and sl[ids["wheel_bodies"][2]] and sl[ids["wheel_bodies"][3]], "car 1 does not sleep"
    assert not sl[ids["chassis"][5]], "car 5 is not awake"
    if size == 1:
        return np.asarray([ids["chain"][20]], np.int32)
    rng = np.random.default_rng(seed)
    must = [ids["chain"][20], ids["chain"][21], ids["chain"][0], ids["wheels"][2], ids["wheels"][3], ids["wheels"][10], ids["wheels"][11],
            ids["sliders"][6], ids["late"]]
    rest = np.setdiff1d(sc.motor_joints, must)
    joints = np.concatenate([must, rng.permutation(rest)[:size - len(must)]]).astype(np.int32)
    joints = rng.permutation(joints)
    assert len(joints) == min(size, len(sc.motor_joints)) == size and len(np.unique(joints)) == len(joints)
    sleeping = [joint_sleeps(sc, sl, j) for j in joints]
    assert any(sleeping) and not all(sleeping)
    bodies = [sc.defs[int(j)]["body_b"] for j in joints] + [sc.defs[int(j)]["body_a"] for j in joints]
    assert len(set(bodies)) < len(bodies), "no two joints of the batch share a body"
    return joints


def motors_of(sc, cur, joints, seed):
    """a JOINT_MOTOR_DTYPE record per joint; every fifth entry repeats what its joint has now (it changes nothing)"""
    rng = np.random.default_rng(seed)
    n = len(joints)
    m = np.zeros(n, b2hip.JOINT_MOTOR_DTYPE)
    m["enable_motor"] = rng.integers(0, 2, n)
    m["motor_speed"] = rng.uniform(-2.0, 2.0, n)
    m["max_motor"] = rng.uniform(5.0, 50.0, n)
    for i in range(0, n, 5):
        if n > 1:
            m["enable_motor"][i], m["motor_speed"][i], m["max_motor"][i] = cur[int(joints[i])]
    return m


def primed(cur, j, rec, mask):
    old = cur[int(j)]
    return [int(rec["enable_motor"] != 0) if mask & 1 else old[0], f32(rec["motor_speed"]) if mask & 2 else old[1],
            f32(rec["max_motor"]) if mask & 4 else old[2]]


def single_motors(w, cur, joints, motors, mask):
    """the definition: b2hip_joint_set_motor entry by entry, an unmasked value being the one the joint has now"""
    for j, rec in zip(joints.tolist(), motors):
        new = primed(cur, j, rec, mask)
        w.joint_set_motor(j, new[0], float(new[1]), float(new[2]))
        cur[j] = new


def batch_motors(w, cur, joints, motors, mask):
    w.joint_set_motors(joints, motors, mask=mask)
    for j, rec in zip(joints.tolist(), motors):
        cur[j] = primed(cur, j, rec, mask)


CASES = [(size, 7, False) for size in (1, 64, 65, 257, 0)] + [(65, mask, False) for mask in range(1, 7)] + [
    (0, 7, True), (65, 2, True), (1, 5, True)]  # size 0: every motor joint


@pytest.mark.gpu
@pytest.mark.parametrize("size,mask,lazy", CASES)
def test_a_batch_equals_the_single_calls_on_a_twin(size, mask, lazy):
    a, b, sc = twins(lazy)
    joints = batch_of(a, sc, size or len(sc.motor_joints), 100 + size)
    cur_a, cur_b = sc.copy_cur(), sc.copy_cur()
    m = motors_of(sc, cur_a, joints, 7 * size + mask)
    before = asleep(a)
    batch_motors(a, cur_a, joints, m, mask)
    single_motors(b, cur_b, joints, m, mask)
    assert cur_a == cur_b
    woken = before & ~asleep(a)
    assert woken.any(), "the batch woke nobody"
    step_and_compare(a, b, "size %d, mask %d" % (size, mask))
    assert snapshot_of(a)[0] != control(lazy, 3)[0], "the batch changed nothing"
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
def test_values_equal_to_the_current_ones_wake_nobody(lazy):
    a, sc = build_world(lazy=lazy)
    ids = sc.ids
    sl = asleep(a)
    joints = np.asarray([j for j in sc.motor_joints if joint_sleeps(sc, sl, j)], np.int32)
    assert set(ids["chain"][1:]) <= set(joints.tolist()) and ids["wheels"][2] in joints and len(joints) > 100
    assert not any(sc.cur[int(j)][0] for j in joints), "a motor is on in the sleeping part"
    m = np.zeros(len(joints), b2hip.JOINT_MOTOR_DTYPE)
    for i, j in enumerate(joints.tolist()):
        m["enable_motor"][i], m["motor_speed"][i], m["max_motor"][i] = sc.cur[j]
    a.joint_set_motors(joints, m, mask=7)
    junk = m.copy()
    junk["motor_speed"] = 9.0  # (not looked at: the mask leaves the speed out)
    a.joint_set_motors(joints, junk, mask=5)
    a.joint_set_motors(joints, enable=False)
    assert snapshot_of(a) == control(lazy, 0)
    assert np.array_equal(asleep(a), sl)
    a.step()
    assert snapshot_of(a) == control(lazy, 1)
    a.step()
    a.step()
    assert snapshot_of(a) == control(lazy, 3)
    a.close()


@pytest.mark.gpu
def test_one_changed_joint_in_the_sleeping_chain_wakes_exactly_its_two_bodies():
    a, b, sc = twins()
    j = sc.ids["chain"][20]
    pair = [sc.defs[j]["body_a"], sc.defs[j]["body_b"]]
    before = a.body_states()
    assert ((before["flags"][pair] & AWAKE) == 0).all()
    # in a batch whose other entries change nothing
    joints = np.asarray([sc.ids["chain"][5], j, sc.ids["chain"][30]], np.int32)
    a.joint_set_motors(joints, speed=[0.0, 1.5, 0.0], enable=[False, True, False])
    after = a.body_states()
    changed = np.flatnonzero((before["flags"] ^ after["flags"]) & AWAKE)
    assert sorted(changed.tolist()) == sorted(pair)
    assert (after["sleep_time"][pair] == 0.0).all()
    others = np.setdiff1d(np.arange(len(after)), pair)
    assert after[others].tobytes() == before[others].tobytes()
    b.joint_set_motor(j, True, 1.5, 10.0)
    step_and_compare(a, b, "one joint of the sleeping chain")
    assert not asleep(a)[sc.ids["links"]].any(), "the island of the chain did not wake in the step"
    a.close()
    b.close()


@pytest.mark.gpu
def test_both_wheel_joints_of_a_sleeping_car_share_the_chassis():
    a, b, sc = twins()
    ids = sc.ids
    car = [ids["chassis"][1], ids["wheel_bodies"][2], ids["wheel_bodies"][3]]
    joints = np.asarray([ids["wheels"][3], ids["wheels"][2]], np.int32)
    assert sc.defs[int(joints[0])]["body_a"] == sc.defs[int(joints[1])]["body_a"] == car[0]
    assert asleep(a)[car].all()
    a.joint_set_motors(joints, speed=-3.0, max_motor=20.0, enable=True)
    s = a.body_states()
    assert ((s["flags"][car] & AWAKE) != 0).all() and (s["sleep_time"][car] == 0.0).all()
    assert asleep(a)[ids["chassis"][0]] and asleep(a)[ids["chassis"][2]]
    for j in joints.tolist():
        b.joint_set_motor(j, True, -3.0, 20.0)
    step_and_compare(a, b, "both wheels of car 1")
    assert abs(a.joint_states(joints)["motor"]).min() > 0.0, "the motors did not work"
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ("single before", "limits after", "two batches", "after velocities"))
def test_edits_before_lie_underneath_and_edits_after_on_top(order):
    a, b, sc = twins()
    ids = sc.ids
    cur_a, cur_b = sc.copy_cur(), sc.copy_cur()
    joints = batch_of(a, sc, 65, 31)
    m = motors_of(sc, cur_a, joints, 32)
    if order == "single before":
        # the mask leaves the speed out: the single call's speed is kept
        j = ids["chain"][20]
        for w, cur in ((a, cur_a), (b, cur_b)):
            w.joint_set_motor(j, True, 1.25, 30.0)
            cur[j] = [1, f32(1.25), f32(30.0)]
        batch_motors(a, cur_a, joints, m, 5)
        single_motors(b, cur_b, joints, m, 5)
        assert cur_a[j][1] == f32(1.25) and cur_a == cur_b
    elif order == "limits after":
        # b2hip_joint_set_limits uploads the motor members again from the host's copy: the batch's must be in it
        batch_motors(a, cur_a, joints, m, 7)
        single_motors(b, cur_b, joints, m, 7)
        for w in (a, b):
            for j in (ids["chain"][20], ids["sliders"][6], ids["chain"][0]):
                assert j in joints
                w.joint_set_limits(j, True, -0.25, 0.3)
    elif order == "two batches":
        second = batch_of(a, sc, 64, 33)
        assert len(np.intersect1d(joints, second)) > 8
        m2 = motors_of(sc, cur_a, second, 34)
        batch_motors(a, cur_a, joints, m, 3)
        batch_motors(a, cur_a, second, m2, 6)
        single_motors(b, cur_b, joints, m, 3)
        single_motors(b, cur_b, second, m2, 6)
        assert cur_a == cur_b
    else:
        bodies = np.unique([sc.defs[int(j)]["body_b"] for j in joints]).astype(np.int32)
        v = np.random.default_rng(35).uniform(-1.0, 1.0, (len(bodies), 2)).astype(f32)
        for w in (a, b):
            w.set_velocities(bodies, velocity=v, omega=0.5)
        batch_motors(a, cur_a, joints, m, 7)
        single_motors(b, cur_b, joints, m, 7)
    step_and_compare(a, b, order)
    a.close()
    b.close()


@pytest.mark.gpu
def test_a_snapshot_taken_after_a_batch_carries_it():
    a, b, sc = twins()
    cur_a, cur_b = sc.copy_cur(), sc.copy_cur()
    joints = batch_of(a, sc, 257, 41)
    m = motors_of(sc, cur_a, joints, 42)
    batch_motors(a, cur_a, joints, m, 7)
    single_motors(b, cur_b, joints, m, 7)
    c = b2hip.World.from_snapshot(a.save_snapshot())
    same(c, b, "the loaded world, at once")
    for k in range(3):
        b.step()
        c.step()
        a.step()
    same(c, b, "the loaded world, step 3")
    same(a, b, "the saved world, step 3")
    # the host's copy of the loaded world holds the batch's values: one more batch that repeats them changes nothing
    c.joint_set_motors(joints, m, mask=7)
    same(c, b, "the loaded world, after repeating the batch")
    for w in (a, b, c):
        w.close()


# ---- reads ---------------------------------------------------------------------------------------------------------------

class MassData(C.Structure):
    _fields_ = [("mass", C.c_float), ("inertia", C.c_float), ("local_center", C.c_float * 2), ("inv_mass", C.c_float),
                ("inv_inertia", C.c_float)]


def local_center(w, body):
    md = MassData()
    w.L.b2hip_get_mass_data.argtypes = [C.c_void_p, C.c_int, C.POINTER(MassData)]
    assert w.L.b2hip_get_mass_data(w.p, body, C.byref(md)) == 0
    return (md.local_center[0], md.local_center[1])


@pytest.mark.gpu
def test_reaction_and_limit_state_equal_the_single_calls():
    w, sc = shared()
    ids = sc.ids
    for inv_dt in (60.0, 1.0, 37.5):
        s = w.joint_states(all_joints(w), inv_dt)
        assert s["pad"].tobytes() == bytes(8 * len(s))
        for j in range(w.joint_count):
            if j == ids["destroyed"]:
                continue
            assert s["type"][j] == sc.defs[j]["type"], j
            r = w.joint_reaction(j, inv_dt)
            got = np.asarray([s["force"][j][0], s["force"][j][1], s["torque"][j], s["motor"][j]], f32)
            assert got.tobytes() == r.tobytes(), "joint %d (type %d): %s, single call %s" % (j, s["type"][j], got, r)
            assert s["limit_state"][j] == w.joint_limit_state(j), j
    s = w.joint_states(all_joints(w))
    # motors and limits worked in the steps before
    assert (s["motor"][ids["sliders"][:5]] != 0.0).all() and (s["limit_state"][ids["sliders"][:5]] != 0).all()
    assert (s["limit_state"][ids["sliders"][5:]] == 0).all()
    pressed = [ids["arms"][k] for k in range(ARMS) if k % 4 == 1]
    assert (s["limit_state"][pressed] != 0).all() and (s["motor"][pressed] != 0.0).all()
    assert (s["motor"][ids["wheels"][8:]] != 0.0).all()
    for name in ("distance", "weld", "rope", "motor", "pulley", "mouse", "gear"):
        assert np.any(s["force"][ids[name]] != 0.0) or s["torque"][ids[name]] != 0.0, name
    assert s["limit_state"][ids["rope"]] == 2 and s["limit_state"][ids["distance"]] == 0
    assert s["torque"][ids["gear"]] != 0.0 or np.any(s["force"][ids["gear"]] != 0.0)
    # the destroyed joint; the joint created after the last step
    d = s[ids["destroyed"]]
    assert d["type"] == -1 and w.joint_is_destroyed(ids["destroyed"]) and not w.joint_is_destroyed(ids["late"])
    assert d.tobytes()[4:] == bytes(44)
    late = s[ids["late"]]
    assert late["type"] == PRISMATIC and late["limit_state"] == 0
    assert late["force"].tobytes() == bytes(8) and late["torque"] == 0.0 and late["motor"] == 0.0
    assert abs(late["coordinate"] - 0.75) < 0.01


@pytest.mark.gpu
def test_coordinates_and_speeds():
    w, sc = build_world()
    ids = sc.ids
    # body edits made since the step are seen: a wheel is given a speed along its axis, a chassis a spin
    st = w.body_states()
    car = 5
    wheel, chassis = ids["wheel_bodies"][2 * car], ids["chassis"][car]
    w.set_velocity(wheel, (float(st["vx"][wheel]), float(st["vy"][wheel]) + 1.0), float(st["w"][wheel]))
    w.set_velocities(np.asarray([chassis], np.int32), omega=0.75)
    st = w.body_states()
    s = w.joint_states(all_joints(w))
    assert st["w"][chassis] == f32(0.75)
    big = {}  # (type, value) -> the largest magnitude / bound seen
    lc = {ids["offcentre"]: local_center(w, ids["offcentre"])}
    assert abs(lc[ids["offcentre"]][0]) > 0.01
    for j, d in sc.defs.items():
        A, B = st[d["body_a"]], st[d["body_b"]]
        row = s[j]
        da, dw = f32(B["angle"] - A["angle"]), f32(B["w"] - A["w"])
        expect2 = (f32(0.0), f32(0.0))
        if d["type"] == REVOLUTE:
            assert f32(row["coordinate"]).tobytes() == f32(da - f32(d["ref"])).tobytes(), j
            assert f32(row["speed"]).tobytes() == dw.tobytes(), j
        elif d["type"] in (PRISMATIC, WHEEL):
            jd = dict(d, lc_a=lc.get(d["body_a"], (0.0, 0.0)), lc_b=lc.get(d["body_b"], (0.0, 0.0)))
            for name, (value, S) in (("coordinate", jr.translation(A, B, jd)), ("speed", jr.linear_speed(A, B, jd))):
                assert abs(float(row[name]) - value) <= jr.bound(S), "joint %d %s: %r, reference %r, bound %g" % (
                    j, name, row[name], value, jr.bound(S))
                key = (d["type"], name)
                big[key] = max(big.get(key, 0.0), abs(value) / jr.bound(S) if S > 0.0 else 0.0)
            if d["type"] == WHEEL:
                expect2 = (da, dw)
        elif d["type"] == PULLEY:
            (la, Sa), (lb, Sb) = jr.pulley_lengths(A, B, d)
            assert abs(float(row["coordinate"]) - la) <= jr.bound(Sa) and abs(float(row["coordinate2"]) - lb) <= jr.bound(Sb)
            assert row["speed"] == 0.0 and row["speed2"] == 0.0
            big[(PULLEY, "a")], big[(PULLEY, "b")] = la / jr.bound(Sa), lb / jr.bound(Sb)
            expect2 = None
        else:
            assert row["coordinate"] == 0.0 and row["speed"] == 0.0, j
        if expect2 is not None:
            assert f32(row["coordinate2"]).tobytes() == expect2[0].tobytes() and f32(row["speed2"]).tobytes() == expect2[1].tobytes(), j
    # a wrong formula cannot pass: of every kind, a value stands 1000 bounds above zero
    for key in ((PRISMATIC, "coordinate"), (PRISMATIC, "speed"), (WHEEL, "coordinate"), (WHEEL, "speed"), (PULLEY, "a"), (PULLEY, "b")):
        assert big[key] > 1000.0, "%s: the largest value is %g bounds" % (key, big[key])
    # ... and the angular values are not all zero, the off-centre wheel turns
    assert abs(s["coordinate"][ids["arms"]]).max() > 0.5 and abs(s["speed"][ids["arms"]]).max() > 1.0
    assert abs(s["speed2"][ids["wheels"][8:]]).min() > 1.0 and abs(s["coordinate2"][ids["wheels"][8:]]).min() > 1.0
    assert abs(st["w"][ids["offcentre"]]) > 1.0
    w.close()


@pytest.mark.gpu
def test_a_read_of_more_than_one_grid_pass_with_repeated_ids():
    w, sc = shared()
    small = w.joint_states(all_joints(w))
    n = 524288 + 65  # one pass of the grid is 2 048 workgroups of 256
    ids = np.random.default_rng(51).integers(0, w.joint_count, n).astype(np.int32)
    ids[-65:] = np.arange(65)[::-1]
    got = w.joint_states(ids)
    assert got.tobytes() == small[ids].tobytes()
    # the same ids in small calls
    for lo in (0, 524288 - 3, n - 65):
        part = ids[lo:lo + 65]
        assert w.joint_states(part).tobytes() == got[lo:lo + 65].tobytes()
    assert w.joint_states(np.zeros(0, np.int32)).shape == (0,)


@pytest.mark.gpu
def test_a_read_changes_nothing():
    a, b, sc = twins()
    joints = np.concatenate([all_joints(a), all_joints(a)[::-3]])
    for k in range(3):
        first = a.joint_states(joints)
        assert a.joint_states(joints).tobytes() == first.tobytes()
        a.joint_states(joints[:1], 1.0)
        a.step()
        b.step()
    same(a, b, "three steps with reads in between")
    a.close()
    b.close()


@pytest.mark.gpu
def test_refusals_name_the_first_offender_and_apply_nothing():
    a, b, sc = twins()
    ids = sc.ids
    good = np.asarray([ids["chain"][3], ids["wheels"][2], ids["sliders"][1], ids["arms"][7], ids["chain"][4]], np.int32)
    nj = a.joint_count

    def refused(call, *words):
        with pytest.raises(b2hip.B2HipError) as e:
            call()
        for word in words:
            assert word in str(e.value), str(e.value)

    def with_entry(k, j):
        bad = good.copy()
        bad[k] = j
        return bad

    for j in (nj, -1):
        refused(lambda: a.joint_set_motors(with_entry(3, j), speed=1.0), "entry 3", "joint %d" % j, "b2hip_joint_count")
        refused(lambda: a.joint_states(with_entry(2, j)), "entry 2", "joint %d" % j, "b2hip_joint_count")
    refused(lambda: a.joint_set_motors(with_entry(1, ids["destroyed"]), speed=1.0), "entry 1", "joint %d" % ids["destroyed"], "destroyed")
    refused(lambda: a.joint_set_motors(with_entry(4, ids["distance"]), speed=1.0), "entry 4", "joint %d" % ids["distance"], "no motor")
    refused(lambda: a.joint_set_motors(with_entry(2, ids["gear"]), speed=1.0), "entry 2", "no motor")
    refused(lambda: a.joint_set_motors(with_entry(4, good[0]), speed=1.0), "entry 4", "joint %d" % good[0], "second time")
    # the first offender is the one named: entry 1 is out of range, entry 3 repeats entry 0
    two = with_entry(3, good[0])
    two[1] = nj
    refused(lambda: a.joint_set_motors(two, speed=1.0), "entry 1", "joint %d" % nj, "b2hip_joint_count")
    assert a.joint_states(with_entry(4, good[0]))["type"][4] == REVOLUTE  # (a read may name a joint twice)
    same(a, b, "after the refused calls")
    # inside a step
    assert a.L.b2hip_step_begin(a.p, C.c_float(1.0 / 60.0), 8, 3) == 0, a.L.b2hip_last_error()
    refused(lambda: a.joint_set_motors(good, speed=1.0), "inside a step")
    refused(lambda: a.joint_states(good), "inside a step")
    for fn in ("b2hip_collide", "b2hip_solve", "b2hip_sync_fixtures", "b2hip_find_new_contacts", "b2hip_solve_toi", "b2hip_step_end"):
        assert getattr(a.L, fn)(a.p) == 0, a.L.b2hip_last_error()
    b.step()
    same(a, b, "a step after the refused calls")
    # the refused write left the host's copy alone too: the same batch, now accepted, equals the single calls
    cur_a, cur_b = sc.copy_cur(), sc.copy_cur()
    m = motors_of(sc, cur_a, good, 61)
    batch_motors(a, cur_a, good, m, 7)
    single_motors(b, cur_b, good, m, 7)
    step_and_compare(a, b, "an accepted batch after the refused ones")
    a.close()
    b.close()
