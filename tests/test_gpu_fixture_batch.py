"""GPU: batched fixture filter, sensor, thick-shape and material sets on the device (include/b2hip.h, block J:
b2hip_fixture_set_filters, b2hip_fixture_set_sensors, b2hip_fixture_set_thicks, b2hip_fixture_set_materials).

The reference is the project's own single-fixture path - b2hip_fixture_set_filter, _sensor, _thick and _material, made entry by
entry as the header's definition by equivalence says - run on a TWIN world: built by the same script and stepped the same
number of times. Every comparison is bit for bit: tobytes() of contacts() (read first: the single route applies its queued
contact operations to the device when somebody reads the contacts), of body_states(), of every fixture's fat AABB, of the
contact events where they are on, and of save_snapshot() - right after the call and after each of 20 later steps. (Snapshots
are compared but for what is no function of the world's history - alignment padding, time stamps, how full the contact-key
hash set is: snapshots_equal() says where these lie and why; the twins' snapshots must agree that way before the call too.)
The world of tests/test_gpu_body_lifecycle.py is restated here (without its jointed pair); each test asserts that its batch holds what it is
about."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import b2hip

AWAKE, ACTIVE = 4, 64  # b2hip_body_state.flags
TOUCHING = 1           # b2hip_contact.flags
SETTLE_STEPS = 40      # the stacks that were put down have gone to sleep, the ones that were dropped are still awake
STACKS, LEVELS, DROPPED_FROM = 80, 4, 64  # the 16 x 20 grid as 80 stacks of 4; stacks 64.. start 1.5 m up
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
STEPS = 20
f32 = np.float32
SIZES = (1, 63, 64, 65, 257, 0)  # 0: every fixture
CALLS = ("filters", "sensors", "thicks", "materials")


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


def build_world(events=False):
    """a static ground; a 16 x 20 grid of small dynamic boxes and circles on it, as 80 stacks of four of which the last 16
    are dropped from 1.5 m; a kinematic body; a fixed-rotation body; a body with two fixtures; a weightless body far away;
    an inactive body; a body with three fixtures whose centre of mass is off its origin. Sleep is allowed; stepped until the
    stacks that were put down sleep. Returns (world, names -> body ids; "fixtures": body id -> its fixture ids)."""
    w = b2hip.World(allow_sleep=True)
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
    w.set_active(ids["inactive"], False)
    ids["three"] = w.create_body(b2hip.DYNAMIC, (-36.0, 0.25))
    fixture(ids["three"], b2hip.box_shape(0.25, 0.25), density=1.0)
    fixture(ids["three"], box_at(0.25, 0.25, 0.5, 0.0), density=3.0)
    fixture(ids["three"], b2hip.circle_shape(0.2, 0.25, 0.45), density=2.0)
    for _ in range(SETTLE_STEPS):
        w.step()
    ids["body_of"] = np.zeros(w.L.b2hip_fixture_count(w.p), np.int32)
    for body, fs in ids["fixtures"].items():
        ids["body_of"][fs] = body
    return w, ids


def twins(events=False):
    a, ids = build_world(events)
    b, _ = build_world(events)
    return a, b, ids


def grid_body(ids, stack, level):
    return ids["grid"][20 * (LEVELS * (stack // 20) + level) + stack % 20]


def fix(ids, body):
    """the first fixture of a body"""
    return ids["fixtures"][body][0]


def fat_aabbs(w):
    """every fixture's fat AABB as the device holds it once the pending edits are uploaded (the read of one body's row does that)"""
    w.body_states_of(np.asarray([0], np.int32))
    n = w.L.b2hip_fixture_count(w.p)
    out = np.zeros((n, 4), f32)
    _check(w.L.b2hip_get_fat_aabbs(w.p, 0, n, out.ctypes.data_as(C.c_void_p)))
    return out


def sorted_events(w):
    e = w.contact_events()
    return e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))]


SNAP_HEADER = struct.Struct("<8s6I8I2I4i2f2i")  # SnapHeader (b2hip_api_snapshot.h)


def snapshot_regions(blob):
    """(start and end of the body rows, start and end of the device-state block) of a snapshot: the header, the world's
    definition, per body a HostBody row and a byte, the fixtures, the shapes, the free proxy ids (an int each), the 40-byte
    state rows, DState; device arrays from there on (b2hip_save_snapshot)"""
    h = SNAP_HEADER.unpack_from(blob)
    sz_dstate, sz_body, sz_fixture, sz_shape = h[2:6]
    nb, nf, ns, nfree, state_count = h[7], h[8], h[9], h[11], h[15]
    rows0 = SNAP_HEADER.size + C.sizeof(b2hip.WorldDef)
    rows1 = rows0 + nb * (sz_body + 1)
    d0 = rows1 + nf * sz_fixture + ns * sz_shape + nfree * 4 + state_count * 40
    return rows0, rows1, d0, d0 + sz_dstate


# What a snapshot holds that is no function of the world's history, by where it lies (csrc/b2hip_host_world.h: HostBody;
# csrc/b2d_world.h: Counters, DState). Nothing else may differ between twins.
#   the body rows     a HostBody row is 31 four-byte members and four bytes of alignment padding in front of a vector, copied
#                     out as they are: bytes 124 .. 127 of every row
#   the device state  DState ends with cur, stamps[6], gapClock[4], phaseClock[16], pubCount, dbgCensus[8], pubSeq, pubPad[3] -
#                     248 bytes behind Counters - and Counters with the contact-key set's ksValid, ksStale, ksMask, ksFill and
#                     ksStats[10], 96 bytes. The 20 clocks are time stamps of the last step's kernels. ksMask / ksFill say how
#                     full the kept hash set is: which of two keys inserted at once takes the earlier slot is a race, so where
#                     a later delete leaves its tombstone, and how many EMPTY slots later inserts use up, differs between two
#                     runs of one script (seen on the device: the same twins agree in one run and not in the next);
#                     b2hip_load_snapshot discards these four words and rebuilds the set. ksStats is compared.
SNAP_SZ_BODY, SNAP_SZ_DSTATE, SNAP_ROW_MEMBERS = 128, 1392, 124
SNAP_COUNTERS = SNAP_SZ_DSTATE - 248
SNAP_STATE_EXEMPT = np.concatenate([np.arange(SNAP_COUNTERS - 96, SNAP_COUNTERS - 80), np.arange(SNAP_COUNTERS + 32, SNAP_COUNTERS + 192)])


def snapshots_equal(x, y, what):
    """two snapshots byte for byte, but for the padding of the body rows, the clocks and the key set's fill (above)"""
    assert len(x) == len(y), "%s: the snapshots differ in length" % what
    rows0, rows1, d0, d1 = snapshot_regions(x)
    assert (rows0, rows1, d0, d1) == snapshot_regions(y), "%s: the snapshots' headers differ" % what
    h = SNAP_HEADER.unpack_from(x)
    assert (h[2], h[3]) == (SNAP_SZ_DSTATE, SNAP_SZ_BODY), "DState or HostBody has changed size: the offsets above want a look"
    at = np.flatnonzero(np.frombuffer(x, np.uint8) != np.frombuffer(y, np.uint8))
    in_rows, in_state = (at >= rows0) & (at < rows1), (at >= d0) & (at < d1)
    exempt = in_rows & ((at - rows0) % (SNAP_SZ_BODY + 1) >= SNAP_ROW_MEMBERS) & ((at - rows0) % (SNAP_SZ_BODY + 1) < SNAP_SZ_BODY)
    exempt |= in_state & np.isin(at - d0, SNAP_STATE_EXEMPT)
    bad = at[~exempt]
    where = "" if len(bad) == 0 else ("byte %d of body row %d" % ((bad[0] - rows0) % (SNAP_SZ_BODY + 1), (bad[0] - rows0) // (SNAP_SZ_BODY + 1)) if in_rows[~exempt][0]
                                      else "byte %d of the device state" % (bad[0] - d0) if in_state[~exempt][0] else "byte %d of %d" % (bad[0], len(x)))
    assert len(bad) == 0, "%s: the snapshots differ in %d bytes, the first at %s" % (what, len(bad), where)


def snapshot_noise(a, b):
    """the twins' snapshots agree before anything is done to them; returns True: same() compares them from here on"""
    snapshots_equal(a.save_snapshot(), b.save_snapshot(), "before anything was done")
    return True


def same(a, b, what, snapshots=False, events=False):
    ca, cb = a.contacts(), b.contacts()
    assert len(ca) == len(cb), "%s: %d contacts against the twin's %d" % (what, len(ca), len(cb))
    if ca.tobytes() != cb.tobytes():
        bad = [n for n in ca.dtype.names if ca[n].tobytes() != cb[n].tobytes()]
        raise AssertionError("%s: contacts differ in %s" % (what, bad))
    sa, sb = a.body_states(), b.body_states()
    if sa.tobytes() != sb.tobytes():
        bad = [n for n in sa.dtype.names if sa[n].tobytes() != sb[n].tobytes()]
        who = np.flatnonzero(np.any([sa[n].view(np.uint32) != sb[n].view(np.uint32) for n in sa.dtype.names], axis=0))
        raise AssertionError("%s: body states differ in %s, bodies %s" % (what, bad, who[:8].tolist()))
    assert not any(np.isnan(sa[n]).any() for n in sa.dtype.names if n != "flags"), "%s: NaN in the states" % what
    xa, xb = fat_aabbs(a), fat_aabbs(b)
    if xa.tobytes() != xb.tobytes():
        who = np.flatnonzero(np.any(xa.view(np.uint32) != xb.view(np.uint32), axis=1))
        raise AssertionError("%s: fat AABBs differ, fixtures %s" % (what, who[:8].tolist()))
    if events:
        assert sorted_events(a).tobytes() == sorted_events(b).tobytes(), "%s: the contact events differ" % what
    if snapshots:
        snapshots_equal(a.save_snapshot(), b.save_snapshot(), what)


def step_and_compare(a, b, what, steps=STEPS, snapshots=False, events=False):
    for k in range(steps):
        a.step()
        b.step()
        same(a, b, "%s, step %d" % (what, k + 1), snapshots, events)


def asleep(w):
    return (w.body_states()["flags"] & AWAKE) == 0


def sleeping_stack(w, ids, skip=0):
    """a stack of the grid whose four bodies sleep (the skip-th such)"""
    sl = asleep(w)
    for stack in range(DROPPED_FROM):
        if all(sl[grid_body(ids, stack, lv)] for lv in range(LEVELS)):
            if skip == 0:
                return stack
            skip -= 1
    raise AssertionError("no stack of the grid sleeps")


def awake_grid_body(w, ids):
    sl = asleep(w)
    awake = [b for b in ids["grid"] if not sl[b]]
    assert awake, "no body of the grid is awake"
    return awake[0]


def contact_between(con, fa, fb):
    return ((con["fixture_a"] == fa) & (con["fixture_b"] == fb)) | ((con["fixture_a"] == fb) & (con["fixture_b"] == fa))


def batch_of(w, ids, size, seed):
    """`size` fixture ids in a shuffled order (0: every fixture). A batch of one is the bottom of a sleeping stack; from 63 on
    the batch holds the ground's fixture - whose contacts are all the stack bottoms' - the kinematic body's, both fixtures of
    the two-fixture body, the inactive body's, an awake grid body's, and two that share a contact (the two lowest of a
    sleeping stack)."""
    stack = sleeping_stack(w, ids)
    bottom, second = fix(ids, grid_body(ids, stack, 0)), fix(ids, grid_body(ids, stack, 1))
    if size == 1:
        return np.asarray([bottom], np.int32)
    rng = np.random.default_rng(seed)
    must = [fix(ids, ids["ground"]), fix(ids, ids["kinematic"]), fix(ids, ids["inactive"]), bottom, second, fix(ids, awake_grid_body(w, ids))] + ids["fixtures"][ids["two"]]
    pool = np.setdiff1d(np.arange(len(ids["body_of"])), must)
    size = size or len(pool) + len(must)
    fixtures = rng.permutation(np.concatenate([must, rng.permutation(pool)[:size - len(must)]]).astype(np.int32))
    assert len(fixtures) == size and len(np.unique(fixtures)) == size
    assert fixtures.tolist() != sorted(fixtures.tolist()) and fixtures.tolist() != sorted(fixtures.tolist())[::-1]
    con = w.contacts()
    assert contact_between(con, bottom, second).any()
    assert np.count_nonzero((con["body_a"] == ids["ground"]) | (con["body_b"] == ids["ground"])) > 64
    return fixtures


def ids_of(fixtures):
    return np.ascontiguousarray(fixtures, np.int32)


# ---- the two routes ------------------------------------------------------------------------------------------------------------
def values_for(call, w, ids, fixtures, seed):
    """what the call sets, per entry: a mix that changes some entries and leaves others as they are"""
    n, rng = len(fixtures), np.random.default_rng(seed)
    if call == "filters":
        cat = np.asarray([1, 2, 4], np.uint16)[rng.integers(0, 3, n)]
        mask = np.asarray([0xFFFF, 0xFFFD, 0xFFFB], np.uint16)[rng.integers(0, 3, n)]
        group = np.asarray([0, 0, -1, 3], np.int16)[rng.integers(0, 4, n)]
        ground = fixtures == fix(ids, ids["ground"])  # (re-filtered with the filter it has: the piles stay on it)
        cat[ground], mask[ground], group[ground] = 1, 0xFFFF, 0
        return cat, mask, group
    if call in ("sensors", "thicks"):
        flag = (np.arange(n) % 3) != 1 if n > 1 else np.asarray([True])
        flag[fixtures == fix(ids, ids["ground"])] = False  # (an entry that has the requested value already)
        return (flag,)
    return rng.uniform(0.5, 3.0, n).astype(f32), rng.uniform(0.0, 1.0, n).astype(f32), rng.uniform(0.0, 0.6, n).astype(f32)


def batched(w, call, fixtures, values):
    if call == "filters":
        w.fixture_set_filters(fixtures, *values)
    elif call == "sensors":
        w.fixture_set_sensors(fixtures, *values)
    elif call == "thicks":
        w.fixture_set_thicks(fixtures, *values)
    else:
        w.fixture_set_materials(fixtures, *values)


def looped(w, call, fixtures, values):
    for i, f in enumerate(np.asarray(fixtures).tolist()):
        v = [np.broadcast_to(x, (len(fixtures),))[i] for x in values]
        if call == "filters":
            w.fixture_set_filter(f, int(v[0]), int(v[1]), int(v[2]))
        elif call == "sensors":
            w.fixture_set_sensor(f, bool(v[0]))
        elif call == "thicks":
            w.fixture_set_thick(f, bool(v[0]))
        else:
            w.fixture_set_material(f, float(v[0]), float(v[1]), float(v[2]))


# ---- 1. every call equals the loop, at every size --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("call", CALLS)
def test_a_batch_equals_the_single_calls_on_a_twin(call, size):
    a, b, ids = twins()
    fixtures = batch_of(a, ids, size, 10 + size)
    if size == 0:
        assert len(fixtures) == a.L.b2hip_fixture_count(a.p)
    values = values_for(call, a, ids, fixtures, 100 + size)
    snapshots = snapshot_noise(a, b)
    was_asleep = asleep(a)
    batched(a, call, fixtures, values)
    looped(b, call, fixtures, values)
    same(a, b, "after the call", snapshots)
    now_asleep = asleep(a)
    if call == "sensors":
        changed = ids["body_of"][fixtures[values[0]]]
        assert not now_asleep[changed].any() and was_asleep[changed].any(), "no sleeping body of a changed entry was woken"
        assert (a.body_states()["sleep_time"][changed] == 0.0).all()
        rest = np.setdiff1d(np.arange(a.body_count), changed)
        assert (now_asleep[rest] == was_asleep[rest]).all(), "a body woke whose fixture did not change"
    else:
        assert (now_asleep == was_asleep).all(), "a %s call woke or put to sleep a body" % call
    n_before = len(a.contacts())
    step_and_compare(a, b, call, snapshots=snapshots)
    if call == "filters" and size >= 63:
        assert len(a.contacts()) != n_before, "the new filters changed no contact"
    a.close()
    b.close()


# ---- 2. filters: contacts go and come back; a shared contact, many contacts, an inactive body; a user contact filter -------------
FILTER_BATCH_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32))


def install_filter(w, refused_pair, seen):
    """a user contact filter through b2hip_set_contact_filter_batch: the built-in rule, except that one pair is refused"""
    w.L.b2hip_default_should_collide.argtypes = [C.c_void_p, C.c_int, C.c_int]
    w.L.b2hip_set_contact_filter_batch.argtypes = [C.c_void_p, FILTER_BATCH_FN, C.c_void_p]

    def should_collide(user, count, pairs, verdict):
        for k in range(count):
            fa, fb = pairs[2 * k], pairs[2 * k + 1]
            seen.add((min(fa, fb), max(fa, fb)))
            verdict[k] = 0 if (min(fa, fb), max(fa, fb)) == refused_pair else w.L.b2hip_default_should_collide(w.p, fa, fb)

    fn = FILTER_BATCH_FN(should_collide)
    _check(w.L.b2hip_set_contact_filter_batch(w.p, fn, None))
    return fn  # (kept alive by the caller)


@pytest.mark.gpu
@pytest.mark.parametrize("user_filter", (False, True))
def test_filters_make_contacts_go_and_come_back(user_filter):
    a, b, ids = twins()
    ground = fix(ids, ids["ground"])
    s0, s1 = sleeping_stack(a, ids), sleeping_stack(a, ids, 1)
    stack = [fix(ids, grid_body(ids, s0, lv)) for lv in range(LEVELS)]
    other_bottom = fix(ids, grid_body(ids, s1, 0))
    refused = (min(ground, other_bottom), max(ground, other_bottom))
    seen_a, seen_b, keep = set(), set(), []
    if user_filter:
        keep = [install_filter(a, refused, seen_a), install_filter(b, refused, seen_b)]
    # the four fixtures of a sleeping stack stop colliding with each other (category 2, not in their mask) and keep the ground;
    # the ground and the bottom of another stack are re-filtered with the filter they have; the inactive body's fixture changes
    fixtures = ids_of([stack[2], ground, stack[0], fix(ids, ids["inactive"]), stack[3], other_bottom, stack[1]])
    cat = np.asarray([2, 1, 2, 4, 2, 1, 2], np.uint16)
    mask = np.asarray([0xFFFD, 0xFFFF, 0xFFFD, 0xFFFF, 0xFFFD, 0xFFFF, 0xFFFD], np.uint16)
    con = a.contacts()
    assert all(contact_between(con, stack[lv], stack[lv + 1]).any() for lv in range(LEVELS - 1))  # (contacts between two named fixtures)
    assert np.count_nonzero((con["fixture_a"] == ground) | (con["fixture_b"] == ground)) > 64      # (a fixture with many contacts)
    assert contact_between(con, ground, other_bottom).any()
    snapshots = snapshot_noise(a, b)
    moves_before = buffered_moves(a)
    was_asleep, fat_before = asleep(a), fat_aabbs(a)
    a.fixture_set_filters(fixtures, cat, mask, 0)
    looped(b, "filters", fixtures, (cat, mask, 0))
    same(a, b, "filters off", snapshots)
    assert (asleep(a) == was_asleep).all(), "somebody woke before the step"
    assert buffered_moves(a) - moves_before == len(fixtures) - 1  # (the inactive body's fixture buffers no move)
    assert buffered_moves(b) == buffered_moves(a)
    a.step()
    b.step()
    same(a, b, "filters off, step 1", snapshots)
    con = a.contacts()
    assert not any(contact_between(con, stack[lv], stack[lv + 1]).any() for lv in range(LEVELS - 1)), "contacts the filter refuses are still there"
    assert contact_between(con, ground, stack[0]).any()
    if user_filter:
        assert refused in seen_a and refused in seen_b, "the re-filtered contact did not reach the user's filter"
        assert (min(stack[0], stack[1]), max(stack[0], stack[1])) in seen_a
        assert not contact_between(con, ground, other_bottom).any(), "the contact the user's filter refused is still there"
    else:
        assert contact_between(con, ground, other_bottom).any()
    # ... and back: the bodies of the stack have not left their fat AABBs, so nothing but the touch of the re-filtered proxies -
    # the move buffer - can make the pairs form again
    assert fat_aabbs(a)[stack].tobytes() == fat_before[stack].tobytes(), "the stack's proxies moved by themselves"
    back = ids_of(stack[::-1])
    awake_before = asleep(a)
    a.fixture_set_filters(back, 1, 0xFFFF, 0)
    looped(b, "filters", back, (1, 0xFFFF, 0))
    same(a, b, "filters on again", snapshots)
    assert (asleep(a) == awake_before).all(), "somebody woke before a contact was made"
    a.step()
    b.step()
    same(a, b, "filters on again, step 1", snapshots)
    con = a.contacts()
    assert all(contact_between(con, stack[lv], stack[lv + 1]).any() for lv in range(LEVELS - 1)), "the contacts did not come back"
    step_and_compare(a, b, "filters on again", snapshots=snapshots)
    a.close()
    b.close()
    del keep


# ---- 3. sensors: who wakes, and the events ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sensors_wake_the_changed_and_the_events_equal_the_twins():
    a, b, ids = twins(events=True)
    s0, s1 = sleeping_stack(a, ids), sleeping_stack(a, ids, 1)
    ground = fix(ids, ids["ground"])
    on = [fix(ids, grid_body(ids, s0, 1)), fix(ids, grid_body(ids, s0, 2)), ids["fixtures"][ids["three"]][1], ground]
    unchanged = [fix(ids, grid_body(ids, s1, lv)) for lv in range(LEVELS)] + [fix(ids, ids["fixedrot"])]
    fixtures = ids_of([on[0], unchanged[0], unchanged[1], on[3], on[1], unchanged[2], unchanged[4], on[2], unchanged[3]])
    flag = np.isin(fixtures, on)
    was_asleep = asleep(a)
    assert was_asleep[ids["body_of"][on[:2]]].all() and was_asleep[ids["body_of"][unchanged[:LEVELS]]].all()
    a.fixture_set_sensors(fixtures, flag)
    looped(b, "sensors", fixtures, (flag,))
    same(a, b, "after the call")
    s, now_asleep = a.body_states(), asleep(a)
    changed = ids["body_of"][on]
    assert not now_asleep[changed].any() and (s["sleep_time"][changed] == 0.0).all(), "a changed entry's body did not wake"
    rest = np.setdiff1d(np.arange(a.body_count), changed)
    assert (now_asleep[rest] == was_asleep[rest]).all(), "a body woke whose fixture did not change"
    ends = begins = 0
    for k in range(STEPS):
        a.step()
        b.step()
        same(a, b, "sensors, step %d" % (k + 1), events=True)
        e = a.contact_events()
        ends, begins = ends + np.count_nonzero(e[:, 2] == 1), begins + np.count_nonzero(e[:, 2] == 0)
    # ... and off again, the ground first: whoever still overlaps it lands
    a.fixture_set_sensors(on[::-1], False)
    looped(b, "sensors", on[::-1], (False,))
    same(a, b, "off again")
    for k in range(STEPS):
        a.step()
        b.step()
        same(a, b, "off again, step %d" % (k + 1), events=True)
        e = a.contact_events()
        ends, begins = ends + np.count_nonzero(e[:, 2] == 1), begins + np.count_nonzero(e[:, 2] == 0)
    assert ends > 0 and begins > 0, "forty steps with the ground a sensor and solid again reported no event"
    a.close()
    b.close()


# ---- 4. materials ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_materials_reach_new_contacts_and_leave_existing_ones():
    a, b, ids = twins()
    fixtures = batch_of(a, ids, 65, 77)
    n = len(fixtures)
    rng = np.random.default_rng(3)
    snapshots = snapshot_noise(a, b)
    before = a.contacts()
    host = {int(q): [None, None, None] for q in fixtures}  # what the loop passes for a field that is left out: read back below
    for mask in (1, 2, 4, 3, 5, 6, 7):
        d, f, r = rng.uniform(0.5, 3.0, n).astype(f32), rng.uniform(0.1, 1.0, n).astype(f32), rng.uniform(0.3, 0.6, n).astype(f32)
        kw = {"density": d if mask & 1 else None, "friction": f if mask & 2 else None, "restitution": r if mask & 4 else None}
        a.fixture_set_materials(fixtures, **kw)
        # the twin: the single call with all three values, those left out as the fixture has them (the creation values, until a
        # round has set them)
        for i, q in enumerate(fixtures.tolist()):
            have = host[q]
            for k, (bit, v) in enumerate(((1, d), (2, f), (4, r))):
                if mask & bit:
                    have[k] = float(v[i])
            now = [float(have[k] if have[k] is not None else created_material(ids, q)[k]) for k in range(3)]
            b.fixture_set_material(q, *now)
        same(a, b, "mask %d" % mask, snapshots)
    after = a.contacts()
    assert after.tobytes() == before.tobytes(), "existing contacts changed their mixture"
    # new contacts: a box dropped onto a stack whose top is in the batch, a circle onto the ground
    top = int(ids["body_of"][fixtures[np.isin(ids["body_of"][fixtures], [grid_body(ids, s, 3) for s in range(DROPPED_FROM)])][0]])
    x = float(a.body_states()["px"][top])
    new = []
    for w in (a, b):
        q = w.create_body(b2hip.DYNAMIC, (x, 2.3))
        new = [w.create_fixture(q, b2hip.box_shape(0.25, 0.25), density=1.0, friction=0.3, restitution=0.2)]
        q = w.create_body(b2hip.DYNAMIC, (-39.0, 0.3))
        new.append(w.create_fixture(q, b2hip.circle_shape(0.25), density=1.0, friction=0.9))
    step_and_compare(a, b, "new contacts", snapshots=snapshots)
    con = a.contacts()
    fresh = con[np.isin(con["fixture_a"], new) | np.isin(con["fixture_b"], new)]
    named = fresh[np.isin(fresh["fixture_a"], fixtures) | np.isin(fresh["fixture_b"], fixtures)]
    assert len(named) >= 2, "no new contact with a fixture of the batch"
    top_f = fix(ids, top)
    k = int(np.flatnonzero(fixtures == top_f)[0])
    mine = named[(named["fixture_a"] == top_f) | (named["fixture_b"] == top_f)][0]
    # (the last round's values, mixed with the new box's 0.3 and 0.2: b2MixFriction is a square root, good to an ulp of float;
    # b2MixRestitution a maximum, exact)
    assert abs(mine["friction"] - np.sqrt(f32(0.3) * f[k])) <= 2.0 ** -23 and mine["restitution"] == r[k] > f32(0.2)
    # the host's copy followed: a later single call on the same fixtures gives equal twins
    for w in (a, b):
        w.fixture_set_material(top_f, 2.0, 0.0, 0.9)
        w.fixture_set_sensor(top_f, True)
        w.fixture_set_sensor(top_f, False)  # (an upload of the fixture's words from the host's copy)
        w.fixture_set_filter(int(fixtures[0]), 1, 0xFFFF, 0)
    same(a, b, "single calls on top")
    step_and_compare(a, b, "single calls on top", 5)
    a.close()
    b.close()


def created_material(ids, fixture):
    """(density, friction, restitution) the fixtures of build_world are created with"""
    body = int(ids["body_of"][fixture])
    if body in ids["grid"]:
        return (1.0 + (ids["grid"].index(body) % 20) % 3, f32(0.6), 0.0)
    k = ids["fixtures"][body].index(fixture)
    density = {ids["ground"]: [0.0], ids["kinematic"]: [0.0], ids["fixedrot"]: [2.0], ids["two"]: [1.0, 3.0], ids["far"]: [1.0], ids["inactive"]: [1.0],
               ids["three"]: [1.0, 3.0, 2.0]}[body][k]
    return (density, f32(0.2), 0.0)


# ---- 5. queries see the batch before any step; pending edits lie underneath --------------------------------------------------------
@pytest.mark.gpu
def test_queries_see_the_batch_and_pending_edits_lie_underneath():
    a, b, ids = twins()
    fixtures = batch_of(a, ids, 64, 5)
    s = a.body_states()
    lower = np.stack([s["px"] - 0.05, s["py"] - 0.05], axis=1).astype(f32)
    upper = np.stack([s["px"] + 0.05, s["py"] + 0.05], axis=1).astype(f32)
    # a single sensor call and a teleport right before the batch, on both twins: they lie underneath it
    lone = next(q for q in (fix(ids, grid_body(ids, sleeping_stack(a, ids, k), 0)) for k in range(2, 30)) if q not in fixtures)
    for w in (a, b):
        w.fixture_set_sensor(lone, True)
        w.set_transform(ids["fixedrot"], (31.0, 0.3), 0.1)
        w.fixture_set_sensor(int(fixtures[3]), True)  # (a fixture of the batch: the batch finds it a sensor already)
    flag = (np.arange(len(fixtures)) % 2) == 1
    assert flag[3]
    a.fixture_set_sensors(fixtures, flag)
    looped(b, "sensors", fixtures, (flag,))
    values = values_for("filters", a, ids, fixtures, 8)
    a.fixture_set_filters(fixtures, *values)
    looped(b, "filters", fixtures, values)
    for mask, sensors in ((0xFFFF, True), (0xFFFF, False), (2, True), (4, False)):
        (oa, ia), (ob, ib) = a.query_aabbs(lower, upper, mask=mask, sensors=sensors), b.query_aabbs(lower, upper, mask=mask, sensors=sensors)
        assert oa.tobytes() == ob.tobytes() and ia.tobytes() == ib.tobytes(), "query_aabbs differs (mask %d, sensors %s)" % (mask, sensors)
        if not sensors:
            assert not np.isin(ia["fixture"], fixtures[flag]).any(), "a query without sensors found a fixture the batch made one"
        if mask != 0xFFFF:
            cats = dict(zip(fixtures.tolist(), values[0].tolist()))
            assert all(cats.get(int(q), 1) == mask for q in ia["fixture"]), "a query found a fixture of another category"
            assert len(ia) > 0
    same(a, b, "after the queries")
    step_and_compare(a, b, "after the queries")
    a.close()
    b.close()


# ---- 6. the TOI partition --------------------------------------------------------------------------------------------------------
def bullet_world():
    """continuous physics: a floor, a wall of static and dynamic boxes in turn, a dozen bullets - some in flight towards the wall,
    some at rest against its foot (the bullet_world of tests/test_gpu_body_lifecycle.py) - of which some fixtures are created as
    sensors or thick shapes, so that a call can switch both ways. Every body has one fixture, with the body's id.
    Returns (world, the fixtures of the wall, those of the bullets at rest, those created as sensors, as thick shapes)."""
    w = b2hip.World(gravity=(0.0, -10.0), allow_sleep=True, continuous=True)
    ground = w.create_body(b2hip.STATIC, (0.0, -0.5))
    assert w.create_fixture(ground, b2hip.box_shape(40.0, 0.5)) == ground
    wall, resting, sensors, thicks = [], [], [], []
    for k in range(8):
        kind = b2hip.STATIC if k % 2 == 0 else b2hip.DYNAMIC
        q = w.create_body(kind, (10.0, 0.25 + 0.5 * k))
        assert w.create_fixture(q, b2hip.box_shape(0.1, 0.25), density=2.0, friction=0.5, sensor=k == 2, thick=k in (4, 5)) == q
        wall.append(q)
        sensors += [q] if k == 2 else []
        thicks += [q] if k in (4, 5) else []
    for k in range(12):
        if k % 2 == 0:  # in flight, one behind the other and at several heights
            q = w.create_body(b2hip.DYNAMIC, (-2.0 - 1.5 * k, 0.6 + 0.25 * k), velocity=(60.0 + 5.0 * k, 0.0), bullet=True, gravity_scale=0.0)
        else:           # at rest on the floor, the first against the wall's foot
            q = w.create_body(b2hip.DYNAMIC, (9.75 - 0.35 * (k // 2), 0.1), bullet=True)
            resting.append(q)
        assert w.create_fixture(q, b2hip.circle_shape(0.1), density=1.0, restitution=0.3, sensor=k in (7, 9)) == q
        sensors += [q] if k in (7, 9) else []
    for _ in range(4):
        w.step()
    return w, wall, resting, sensors, thicks


def toi_slots(w):
    """SnapHeader::nToiOrder of a snapshot taken now (b2hip_api_snapshot.h): magic, six sizes, then the counts"""
    return struct.unpack_from("<I", w.save_snapshot(), 8 + 4 * 12)[0]


def buffered_moves(w):
    """SnapHeader::nMoves: the count behind nToiOrder"""
    return struct.unpack_from("<I", w.save_snapshot(), 8 + 4 * 13)[0]


def debug30(w):
    out = (C.c_longlong * 2)(0, 0)
    _check(w.L.b2hip_debug_read(w.p, 30, 0, 2, out))
    return out[0], out[1]


def out_of_order(w, fixtures, seed):
    """the fixtures in an order that is neither ascending nor descending in the index of their first contact"""
    con = w.contacts()
    first = {int(q): int(np.flatnonzero((con["fixture_a"] == q) | (con["fixture_b"] == q))[0]) for q in fixtures
             if ((con["fixture_a"] == q) | (con["fixture_b"] == q)).any()}
    by_contact = sorted(first, key=lambda q: first[q])
    assert len(by_contact) >= 4, "fewer than four of the fixtures have contacts"
    head = [by_contact[1], by_contact[-1], by_contact[0]]
    rest = np.random.default_rng(seed).permutation(np.setdiff1d(fixtures, head)).tolist()
    order = head + rest
    idx = [first[q] for q in order if q in first]
    assert idx != sorted(idx) and idx != sorted(idx)[::-1]
    return ids_of(order), con


@pytest.mark.gpu
@pytest.mark.parametrize("sort_max,room", ((None, None), (2, None), (2, 1)))
def test_the_toi_partition_follows_the_loops_order(sort_max, room):
    """sort_max 2: B2HIP_TEST_LIFECYCLE_SORT_MAX lowers the one-workgroup sort's capacity, so that the lists of this small world
    go through the radix sort; room 1: B2HIP_TEST_FIXTURE_LIST_ROOM gives the first listing room for one contact, so that the
    call lists a second time (b2hip_debug_read 30 counts both)."""
    env = {"B2HIP_TEST_LIFECYCLE_SORT_MAX": sort_max, "B2HIP_TEST_FIXTURE_LIST_ROOM": room}
    for k, v in env.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        (a, wall, resting, sensors, thicks), b, c = bullet_world(), bullet_world()[0], bullet_world()[0]
    finally:
        for k in env:
            os.environ.pop(k, None)
    snapshots = snapshot_noise(a, b)
    assert toi_slots(a) >= 6
    assert set(sensors) <= set(resting[:5] + wall[1:4]) and set(thicks) <= set(wall[1:7])
    for call, named in (("thicks", wall[1:7] + [0]), ("sensors", resting[:5] + wall[1:4])):
        fixtures, con = out_of_order(a, named, 7)
        have = np.zeros(a.L.b2hip_fixture_count(a.p), bool)
        have[sensors if call == "sensors" else thicks] = True      # (what bullet_world created as sensors / thick shapes)
        flag = ~have[fixtures]                                       # every entry changes: on and off mixed
        flag[-1] = have[fixtures[-1]]                                # ... but the last, which has the requested value already
        assert flag.any() and not flag.all()
        both = np.isin(con["fixture_a"], fixtures[:-1]) & np.isin(con["fixture_b"], fixtures[:-1])
        assert both.any(), "no contact lies between two named fixtures"
        # the twin of the twins says how many slots every entry frees (+) or adds (-)
        delta, slots = [], toi_slots(c)
        for q, v in zip(fixtures.tolist(), flag.tolist()):
            looped(c, call, [q], ([v],))
            now = toi_slots(c)
            delta.append(slots - now)
            slots = now
        assert np.count_nonzero(delta) >= 2 and min(delta) < 0 < max(delta), delta
        before = toi_slots(a)
        batched(a, call, fixtures, (flag,))
        looped(b, call, fixtures, (flag,))
        assert before - toi_slots(a) == sum(delta) and toi_slots(a) == toi_slots(b) == slots
        same(a, b, "after the %s call" % call, snapshots)
        for k in range(3):
            a.step()
            b.step()
            c.step()
            same(a, b, "continuous, %s, step %d" % (call, k + 1), snapshots)
    long_sorts, relists = debug30(a)
    assert (long_sorts >= 1) == (sort_max is not None) and (relists >= 1) == (room is not None), (long_sorts, relists)
    step_and_compare(a, b, "continuous", 25, snapshots)
    for w in (a, b, c):
        w.close()


# ---- 7. refusals apply nothing ---------------------------------------------------------------------------------------------------
def everything(w):
    return (w.contacts().tobytes(), w.body_states().tobytes(), fat_aabbs(w).tobytes(), w.save_snapshot())


@pytest.mark.gpu
def test_refused_calls_name_the_offender_and_apply_nothing():
    a, b, ids = twins()
    nf = a.L.b2hip_fixture_count(a.p)
    victim = ids["fixtures"][ids["three"]][2]
    for w in (a, b):
        w.destroy_fixture(victim)
    good = ids_of([fix(ids, q) for q in ids["grid"][20:30]])
    before = everything(a)  # (the contacts first: the read applies the single call's queued operation)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    filters, flags, materials = np.zeros(10, b2hip.FIXTURE_FILTER_DTYPE), np.ones(10, np.uint8), np.ones(10, b2hip.FIXTURE_MATERIAL_DTYPE)
    filters["category_bits"], filters["mask_bits"] = 2, 0xFFFD

    def calls(fixtures, mask=7):
        return (("b2hip_fixture_set_filters", lambda: a.L.b2hip_fixture_set_filters(a.p, len(fixtures), vp(fixtures), vp(filters))),
                ("b2hip_fixture_set_sensors", lambda: a.L.b2hip_fixture_set_sensors(a.p, len(fixtures), vp(fixtures), vp(flags))),
                ("b2hip_fixture_set_thicks", lambda: a.L.b2hip_fixture_set_thicks(a.p, len(fixtures), vp(fixtures), vp(flags))),
                ("b2hip_fixture_set_materials", lambda: a.L.b2hip_fixture_set_materials(a.p, len(fixtures), vp(fixtures), vp(materials), mask)))

    def refused(fixtures, words):
        for name, call in calls(ids_of(fixtures)):
            assert call() == ERR_INVALID, name
            msg = a.L.b2hip_last_error().decode()
            for word in (name,) + words:
                assert word in msg, (word, msg)
        assert everything(a) == before, "a refused call changed the world"

    bad = good.copy()
    bad[6] = nf
    refused(bad, ("entry 6", "fixture %d" % nf))
    bad[6] = -1
    refused(bad, ("entry 6", "fixture -1"))
    bad = good.copy()
    bad[8] = good[2]
    refused(bad, ("entry 8", "fixture %d" % good[2], "second time"))
    bad = good.copy()
    bad[3] = victim
    refused(bad, ("entry 3", "fixture %d" % victim, "destroyed"))
    for mask in (0, 8):
        name, call = calls(good, mask)[3]
        assert call() == ERR_INVALID
        assert name in a.L.b2hip_last_error().decode() and "mask" in a.L.b2hip_last_error().decode()
        assert everything(a) == before
    # inside a step
    _check(a.L.b2hip_step_begin(a.p, C.c_float(1.0 / 60.0), 8, 3))
    for name, call in calls(good):
        assert call() == ERR_INVALID
        assert "inside a step" in a.L.b2hip_last_error().decode()
    for fn in ("b2hip_collide", "b2hip_solve", "b2hip_sync_fixtures", "b2hip_find_new_contacts", "b2hip_solve_toi", "b2hip_step_end"):
        _check(getattr(a.L, fn)(a.p))
    b.step()
    same(a, b, "a step after the refused calls")
    # n == 0 succeeds, and a valid call afterwards still equals the twin
    none = np.zeros(0, np.int32)
    for name, call in calls(none):
        assert call() == 0, name
    for call in CALLS:
        values = values_for(call, a, ids, good, 9)
        batched(a, call, good, values)
        looped(b, call, good, values)
        same(a, b, "a valid %s call" % call)
    step_and_compare(a, b, "after the refused calls")
    a.close()
    b.close()


@pytest.mark.gpu
def test_the_move_buffer_is_guarded():
    a, b, ids = twins()
    fixtures = np.random.default_rng(7).permutation(a.L.b2hip_fixture_count(a.p)).astype(np.int32)
    bodies = np.setdiff1d(np.arange(a.body_count), [ids["inactive"]]).astype(np.int32)
    home = np.stack([a.body_states()["px"][bodies], a.body_states()["py"][bodies]], axis=1)
    cat, mask = (1 + (fixtures % 2)).astype(np.uint16), 0xFFFF
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rec = np.zeros(len(fixtures), b2hip.FIXTURE_FILTER_DTYPE)
    rec["category_bits"], rec["mask_bits"] = cat, mask
    refusals = 0
    for k in range(10):
        # a teleport out of every fat AABB and (next round) back, without a step: the buffer fills (the teleport has a guard of
        # its own: a round it does not fit is left out on both twins)
        pose3 = np.zeros((len(bodies), 3), f32)
        pose3[:, :2] = home + (0.5 if k % 2 == 0 else 0.0)
        rc = a.L.b2hip_set_transforms(a.p, len(bodies), vp(bodies), vp(pose3), 1)
        assert rc in (0, ERR_UNSUPPORTED) and (rc == 0 or k > 0), rc
        if rc == 0:
            b.set_transforms(bodies, position=pose3[:, :2])
        before = everything(a)
        rc = a.L.b2hip_fixture_set_filters(a.p, len(fixtures), vp(fixtures), vp(rec))
        if k == 0:
            assert rc == 0, "a teleport of every body and a batch over every fixture of a freshly stepped world must fit"
        if rc == 0:
            looped(b, "filters", fixtures, (cat, mask, 0))
            continue
        refusals += 1
        assert rc == ERR_UNSUPPORTED, rc
        msg = a.L.b2hip_last_error().decode()
        assert "b2hip_fixture_set_filters" in msg and "step" in msg and "move buffer" in msg, msg
        assert everything(a) == before, "a refused call changed the world"
        break
    assert refusals == 1, "ten rounds of teleports and re-filters fitted a buffer of 2 x fixtures + 64 moves"
    same(a, b, "after the calls that were accepted")
    a.step()
    b.step()
    same(a, b, "step 1")
    a.fixture_set_filters(fixtures, cat, mask, 0)  # (the step emptied the buffer)
    looped(b, "filters", fixtures, (cat, mask, 0))
    step_and_compare(a, b, "after the guard", 5)
    a.close()
    b.close()
