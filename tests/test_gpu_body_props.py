"""GPU: batched body property sets on the device (include/b2hip.h, block K: b2hip_set_types, b2hip_set_bullets,
b2hip_set_fixed_rotations, b2hip_set_sleeping_alloweds, b2hip_set_body_dampings, b2hip_set_mass_datas, b2hip_reset_mass_datas).

The reference is the project's own single-body path - b2hip_set_type, b2hip_set_bullet, b2hip_set_fixed_rotation,
b2hip_set_sleeping_allowed, b2hip_set_body_damping, b2hip_set_mass_data - made entry by entry as the header's definition by
equivalence says, on a TWIN world: built by the same script and stepped the same number of times. Every comparison is bit for
bit: tobytes() of contacts() (read first: the single route applies its queued contact operations to the device when somebody
reads the contacts), of body_states(), of the mass data of every body, of the destroyed marks, of the fat AABBs of the live
proxies, of the island labels, of the damping rows, and of save_snapshot() before the next step. The 330-body world of
tests/test_gpu_body_lifecycle.py is restated here with a bullet body, a body on a mouse joint and a spinning body whose centre
of mass is off its origin; each test asserts that its batch holds what it is about.

What of a snapshot is compared (snapshots_equal): everything but the parts that are a CACHE of device rows whose freshness the
two routes differ in by design - the single calls pull the host's row of a body and upload it, the batched calls edit the
device's row and mark the host's as not pulled (block K: "marked as not pulled", bodyWritesMirror). Those are, of a HostBody
row, the members the read-back refreshes (the awake bit, the pose, the sweep, the velocity, the forces, the sleep time and the
sweep-reset mark), the table of state rows the last read-back left (the single route's is older than its host rows, the batched
route's is newer), and HostFixture::fat (the device owns the fat AABB of an uploaded fixture; b2hip_set_type refreshes the
host's copy on the way). What these caches stand for is compared through body_states() and the fat AABBs. Everything the host
alone owns - type, bullet / fixed-rotation / auto-sleep / active bits, local centre, mass, inertia, dampings, seed-order slot,
dead mark - and every device array - the rows with the sweep origins, the proxies, the contacts with the continuous-collision
partition, the buffered moves - is compared byte for byte."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import b2hip

AWAKE, AUTOSLEEP, BULLET, FIXEDROT, ACTIVE = 4, 8, 16, 32, 64  # b2hip_body_state.flags
TOUCHING = 1
SETTLE_STEPS = 40      # the stacks that were put down have gone to sleep, the ones that were dropped are still awake
STACKS, LEVELS, DROPPED_FROM = 80, 4, 64  # the 16 x 20 grid as 80 stacks of 4; stacks 64.. start 1.5 m up
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
f32 = np.float32
SIZES = (1, 63, 64, 65, 257, 0)  # 0: every body


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


def build_world(lazy=False, events=False, continuous=False):
    """a static ground; a 16 x 20 grid of small dynamic boxes and circles on it, as 80 stacks of four of which the last 16
    are dropped from 1.5 m; a kinematic body; a fixed-rotation body; a body with two fixtures; a weightless body far away;
    an inactive body; a body with three fixtures whose centre of mass is off its origin; two boxes joined by a revolute joint;
    a bullet body; a body on a mouse joint; a weightless spinning body with an off-centre mass. Sleep is allowed; stepped until
    the stacks that were put down sleep.
    Returns (world, names -> body ids; "fixtures": body id -> its fixture ids; "damping": the (n, 3) damping rows as created)."""
    w = b2hip.World(allow_sleep=True, continuous=continuous)
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
    w.set_active(ids["inactive"], False)
    ids["three"] = w.create_body(b2hip.DYNAMIC, (-36.0, 0.25))
    fixture(ids["three"], b2hip.box_shape(0.25, 0.25), density=1.0)
    fixture(ids["three"], box_at(0.25, 0.25, 0.5, 0.0), density=3.0)
    fixture(ids["three"], b2hip.circle_shape(0.2, 0.25, 0.45), density=2.0)
    ids["pair"] = [w.create_body(b2hip.DYNAMIC, (-33.0, 0.25)), w.create_body(b2hip.DYNAMIC, (-32.4, 0.25))]
    for b in ids["pair"]:
        fixture(b, b2hip.box_shape(0.25, 0.25), density=1.0, friction=0.6)
    ids["joint"] = w.create_revolute_joint(ids["pair"][0], ids["pair"][1], anchor_a=(0.3, 0.0), anchor_b=(-0.3, 0.0))
    ids["bullet"] = w.create_body(b2hip.DYNAMIC, (33.5, 0.25), bullet=True)
    fixture(ids["bullet"], b2hip.box_shape(0.25, 0.25), density=1.0, friction=0.6)
    ids["mouse"] = w.create_body(b2hip.DYNAMIC, (26.5, 1.0))
    fixture(ids["mouse"], b2hip.box_shape(0.25, 0.25), density=1.5)
    ids["mouse_joint"] = w.create_mouse_joint(ids["ground"], ids["mouse"], (26.8, 1.6), 200.0)
    ids["spin"] = w.create_body(b2hip.DYNAMIC, (60.0, 30.0), velocity=(0.5, 0.25), omega=2.0, gravity_scale=0.0)
    fixture(ids["spin"], b2hip.box_shape(0.25, 0.25), density=1.0)
    fixture(ids["spin"], box_at(0.25, 0.25, 0.7, 0.2), density=4.0)
    for _ in range(SETTLE_STEPS):
        w.step()
    damping = np.zeros((w.body_count, 3), f32)
    damping[:, 2] = 1.0
    damping[[ids["far"], ids["spin"]], 2] = 0.0
    ids["damping"] = damping
    return w, ids


def twins(**kw):
    a, ids = build_world(**kw)
    b, _ = build_world(**kw)
    return a, b, ids


def grid_body(ids, stack, level):
    return ids["grid"][20 * (LEVELS * (stack // 20) + level) + stack % 20]


def ids_of(bodies):
    return np.ascontiguousarray(bodies, np.int32)


def destroyed_marks(w):
    nb, nf = w.body_count, w.L.b2hip_fixture_count(w.p)
    return (np.asarray([w.L.b2hip_body_is_destroyed(w.p, i) for i in range(nb)], np.int8),
            np.asarray([w.L.b2hip_fixture_is_destroyed(w.p, i) for i in range(nf)], np.int8))


def fat_aabbs(w):
    """every fixture's fat AABB as the device holds it once the pending edits are uploaded (the read of one body's row does that)"""
    w.body_states_of(np.asarray([0], np.int32))
    n = w.L.b2hip_fixture_count(w.p)
    out = np.zeros((n, 4), f32)
    _check(w.L.b2hip_get_fat_aabbs(w.p, 0, n, out.ctypes.data_as(C.c_void_p)))
    return out


def live_fixtures(w, ids):
    s = w.body_states()
    out = [f for body, fs in ids["fixtures"].items() if s["flags"][body] & ACTIVE for f in fs]
    return np.asarray(sorted(out), np.int64)


def mass_datas(w):
    return np.asarray([w.mass_data(i) for i in range(w.body_count)], b2hip.MASS_DATA_DTYPE)


def damping_rows(w):
    """the device's damping rows (b2hip_debug_read 5), behind the pending edits"""
    w.body_states_of(np.asarray([0], np.int32))
    out = np.zeros((w.body_count, 4), f32)
    _check(w.L.b2hip_debug_read(w.p, 5, 0, w.body_count, out.ctypes.data_as(C.c_void_p)))
    return out


def sorted_events(w):
    e = w.contact_events()
    return e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))]


# ---- snapshots (the head of this file says what is compared and why) -------------------------------------------------------------
SNAP_HEADER = struct.Struct("<8s6I8I2I4i2f2i")  # SnapHeader (b2hip_api_snapshot.h)
# HostBody (csrc/b2hip_host_world.h): 31 four-byte members and four bytes of padding, then one byte "dirty". Host-owned: type
# (0..4), of the flags byte 4 the bits above the awake bit, the local centre (48..56), mass, I, invMass, invI (80..96), the
# dampings (96..108), the seed-order slot and the dead mark (112..120), the dirty byte (128).
SNAP_SZ_BODY, SNAP_SZ_FIXTURE, SNAP_SZ_DSTATE = 128, 52, 1392
BODY_OWNED = np.concatenate([np.arange(0, 4), np.arange(48, 56), np.arange(80, 108), np.arange(112, 120), [128]])
FIXTURE_FAT = np.arange(32, 48)  # HostFixture::fat
# DState: the clocks and the fill of the contact-key set are no function of the world's history (tests/test_gpu_fixture_batch.py
# says where they lie and why)
SNAP_COUNTERS = SNAP_SZ_DSTATE - 248
# ... and dbgCensus[8], 32 bytes from byte 196 behind Counters: a diagnostic record of the FIRST large-island body k_block_census
# met without a block, taken with an atomicCAS by whichever lane comes first (csrc/b2d_kernels_solve_blocks.h) - a race between
# lanes, met here once the ground has turned dynamic and the whole world is one large island; nothing reads it but a debug print
SNAP_STATE_EXEMPT = np.concatenate([np.arange(SNAP_COUNTERS - 96, SNAP_COUNTERS - 80), np.arange(SNAP_COUNTERS + 32, SNAP_COUNTERS + 192),
                                    np.arange(SNAP_COUNTERS + 196, SNAP_COUNTERS + 228)])


# ... and `cur`, in the header (its 17th word) and first behind Counters: WHICH of the two contact buffers holds the array. It
# flips with every compaction, and the two routes compact at different moments by contract - a batch when it is made, behind the
# pending operations it applies first; the single calls' queued operations when somebody reads the contacts or steps - so that
# single calls mixed with batches compact a different number of times. The snapshot carries the array of the current buffer, and
# that is compared.
SNAP_HEADER_CUR = 16
SNAP_STATE_EXEMPT = np.concatenate([SNAP_STATE_EXEMPT, np.arange(SNAP_COUNTERS, SNAP_COUNTERS + 4)])


def snapshots_equal(x, y, what):
    assert len(x) == len(y), "%s: the snapshots differ in length" % what
    hx, hy = list(SNAP_HEADER.unpack_from(x)), list(SNAP_HEADER.unpack_from(y))
    hx[SNAP_HEADER_CUR] = hy[SNAP_HEADER_CUR] = 0
    assert hx == hy, "%s: the snapshots' headers differ: %s against %s" % (what, hx, hy)
    assert (hx[2], hx[3], hx[4]) == (SNAP_SZ_DSTATE, SNAP_SZ_BODY, SNAP_SZ_FIXTURE), "DState, HostBody or HostFixture has changed size"
    nb, nf, ns, nfree, state_count = hx[7], hx[8], hx[9], hx[11], hx[15]
    rows0 = SNAP_HEADER.size + C.sizeof(b2hip.WorldDef)
    rows1 = rows0 + nb * (SNAP_SZ_BODY + 1)
    fix1 = rows1 + nf * SNAP_SZ_FIXTURE
    state0 = fix1 + ns * hx[5] + nfree * 4
    d0 = state0 + state_count * 40
    d1 = d0 + SNAP_SZ_DSTATE
    ax, ay = np.frombuffer(x, np.uint8), np.frombuffer(y, np.uint8)
    assert ax[SNAP_HEADER.size:rows0].tobytes() == ay[SNAP_HEADER.size:rows0].tobytes(), "%s: the world definitions differ" % what
    bx, by = ax[rows0:rows1].reshape(nb, SNAP_SZ_BODY + 1), ay[rows0:rows1].reshape(nb, SNAP_SZ_BODY + 1)
    bad = np.flatnonzero((bx[:, BODY_OWNED] != by[:, BODY_OWNED]).any(axis=1) | ((bx[:, 4] & 0x78) != (by[:, 4] & 0x78)))
    assert len(bad) == 0, "%s: the host-owned members of the body rows differ, bodies %s" % (what, bad[:8].tolist())
    fx, fy = ax[rows1:fix1].reshape(nf, SNAP_SZ_FIXTURE).copy(), ay[rows1:fix1].reshape(nf, SNAP_SZ_FIXTURE).copy()
    fx[:, FIXTURE_FAT] = 0
    fy[:, FIXTURE_FAT] = 0
    bad = np.flatnonzero((fx != fy).any(axis=1))
    assert len(bad) == 0, "%s: the fixture rows differ, fixtures %s" % (what, bad[:8].tolist())
    assert ax[fix1:state0].tobytes() == ay[fix1:state0].tobytes(), "%s: the shapes or the free proxy ids differ" % what
    at = np.flatnonzero(ax[d0:d1] != ay[d0:d1])
    at = at[~np.isin(at, SNAP_STATE_EXEMPT)]
    assert len(at) == 0, "%s: the device state differs, the first at byte %d" % (what, at[0])
    at = np.flatnonzero(ax[d1:] != ay[d1:])
    assert len(at) == 0, "%s: the device arrays differ in %d bytes, the first at byte %d of %d behind the device state" % (
        what, len(at), at[0] if len(at) else -1, len(x) - d1)


def same(a, b, what, ids, snapshots=True, events=False):
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
    ma, mb = mass_datas(a), mass_datas(b)
    if ma.tobytes() != mb.tobytes():
        who = np.flatnonzero([ma[i].tobytes() != mb[i].tobytes() for i in range(len(ma))])
        raise AssertionError("%s: mass data differ, bodies %s" % (what, who[:8].tolist()))
    (da, fa), (db, fb) = destroyed_marks(a), destroyed_marks(b)
    assert da.tobytes() == db.tobytes() and fa.tobytes() == fb.tobytes(), "%s: the destroyed marks differ" % what
    live = live_fixtures(a, ids)
    assert live.tobytes() == live_fixtures(b, ids).tobytes()
    xa, xb = fat_aabbs(a)[live], fat_aabbs(b)[live]
    if xa.tobytes() != xb.tobytes():
        who = live[np.flatnonzero(np.any(xa.view(np.uint32) != xb.view(np.uint32), axis=1))]
        raise AssertionError("%s: fat AABBs differ, fixtures %s" % (what, who[:8].tolist()))
    assert a.island_labels().tobytes() == b.island_labels().tobytes(), "%s: the island labels differ" % what
    assert damping_rows(a).tobytes() == damping_rows(b).tobytes(), "%s: the damping rows differ" % what
    if events:
        assert sorted_events(a).tobytes() == sorted_events(b).tobytes(), "%s: the contact events differ" % what
    if snapshots:
        snapshots_equal(a.save_snapshot(), b.save_snapshot(), what)


def step_and_compare(a, b, what, ids, steps=3, events=False):
    for k in range(steps):
        a.step()
        b.step()
        same(a, b, "%s, step %d" % (what, k + 1), ids, events=events)


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


NAMED = ("ground", "kinematic", "fixedrot", "two", "far", "inactive", "three", "bullet", "mouse", "spin")


def batch_of(w, ids, size, seed, single="bottom"):
    """`size` body ids in a shuffled order (0: every body). A batch of one is ids[single], or the bottom of a sleeping stack;
    from 63 on the batch holds every named body of the world - the static ground, whose contacts are all the stack bottoms', the
    kinematic, the fixed-rotation, the two- and three-fixture, the far, the inactive, the bullet, the mouse-jointed and the
    spinning body, the jointed pair - a sleeping and an awake grid body, and two bodies that touch each other (the two lowest of
    a sleeping stack)."""
    stack = sleeping_stack(w, ids)
    bottom, second = grid_body(ids, stack, 0), grid_body(ids, stack, 1)
    if size == 1:
        return np.asarray([bottom if single == "bottom" else ids[single]], np.int32)
    rng = np.random.default_rng(seed)
    must = [ids[k] for k in NAMED] + ids["pair"] + [bottom, second, awake_grid_body(w, ids)]
    pool = np.setdiff1d(np.arange(w.body_count), must)
    size = size or w.body_count
    bodies = rng.permutation(np.concatenate([must, rng.permutation(pool)[:size - len(must)]]).astype(np.int32))
    assert len(bodies) == size and len(np.unique(bodies)) == size
    touching = w.contacts()
    touching = touching[(touching["flags"] & TOUCHING) != 0]
    assert (((touching["body_a"] == bottom) & (touching["body_b"] == second)) | ((touching["body_a"] == second) & (touching["body_b"] == bottom))).any()
    assert np.count_nonzero((touching["body_a"] == ids["ground"]) | (touching["body_b"] == ids["ground"])) > 64
    return bodies


def toi_slots(w):
    """SnapHeader::nToiOrder of a snapshot taken now (b2hip_api_snapshot.h): magic, six sizes, then the counts"""
    return struct.unpack_from("<I", w.save_snapshot(), 8 + 4 * 12)[0]


def buffered_moves(w):
    return struct.unpack_from("<I", w.save_snapshot(), 8 + 4 * 13)[0]


def debug_stats(w, which, count):
    out = (C.c_longlong * count)()
    _check(w.L.b2hip_debug_read(w.p, which, 0, count, out))
    return tuple(out)


# ---- 1. dampings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_dampings_equal_the_single_calls_for_every_mask(size):
    a, b, ids = twins()
    bodies = batch_of(a, ids, size, 100 + size)
    have = ids["damping"].copy()
    snapshots_equal(a.save_snapshot(), b.save_snapshot(), "before anything was done")
    asleep_before = asleep(a)
    assert asleep_before[bodies].any()
    rng = np.random.default_rng(size)
    for mask in range(1, 8):
        new = rng.uniform(0.0, 0.5, (len(bodies), 3)).astype(f32)
        kw = {name: new[:, k] for k, name in enumerate(("linear", "angular", "gravity_scale")) if mask & (1 << k)}
        before = damping_rows(a)
        a.set_body_dampings(bodies, **kw)
        for k in range(3):
            if mask & (1 << k):
                have[bodies, k] = new[:, k]
        for q in bodies.tolist():
            b.set_body_damping(q, float(have[q, 0]), float(have[q, 1]), float(have[q, 2]))
        rows = damping_rows(a)
        assert rows[:, :3].tobytes() == have.tobytes(), "mask %d: the device's rows are not what was set" % mask
        for k in range(3):  # a masked-out field keeps its bits
            if not mask & (1 << k):
                assert rows[:, k].tobytes() == before[:, k].tobytes()
        same(a, b, "mask %d" % mask, ids)
    assert (asleep(a) == asleep_before).all(), "a damping set woke somebody"
    step_and_compare(a, b, "dampings", ids)
    a.close()
    b.close()


# ---- 2. sleeping allowed ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_sleeping_alloweds_equal_the_single_calls(size):
    a, b, ids = twins()
    bodies = batch_of(a, ids, size, 200 + size)
    stack = sleeping_stack(a, ids)
    flags = (np.arange(len(bodies)) % 3) != 0
    flags[np.isin(bodies, [grid_body(ids, stack, 0), ids["ground"]])] = False   # a sleeping body must stay awake from now on
    flags[bodies == grid_body(ids, stack, 1)] = True                             # ... its neighbour is only told what it is told already
    before = a.body_states()
    a.set_sleeping_alloweds(bodies, flags)
    for q, f in zip(bodies.tolist(), flags.tolist()):
        b.set_sleeping_allowed(q, f)
    same(a, b, "after the call", ids)
    s = a.body_states()
    off, on = bodies[~flags], bodies[flags]
    assert ((before["flags"][off] & AWAKE) == 0).any(), "no sleeping body in the batch was told to stay awake"
    assert (s["flags"][off] & (AWAKE | AUTOSLEEP) == AWAKE).all() and not s["sleep_time"][off].any()
    if len(on):
        assert (s["flags"][on] & AUTOSLEEP).all()
        for name in s.dtype.names:  # true changes nothing but the bit
            x, y = s[name][on], before[name][on]
            assert ((x | AUTOSLEEP) == (y | AUTOSLEEP)).all() if name == "flags" else x.tobytes() == y.tobytes(), name
    step_and_compare(a, b, "sleeping allowed", ids)
    # and allowed again: the bodies may fall asleep once more
    a.set_sleeping_alloweds(bodies, True)
    for q in bodies.tolist():
        b.set_sleeping_allowed(q, True)
    same(a, b, "allowed again", ids)
    step_and_compare(a, b, "allowed again", ids, 2)
    a.close()
    b.close()


# ---- 3. bullets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_bullets_equal_the_single_calls_on_a_continuous_world(size):
    a, b, ids = twins(continuous=True)
    bodies = batch_of(a, ids, size, 300 + size)
    flags = np.ones(len(bodies), bool)
    flags[bodies == ids["bullet"]] = len(bodies) % 2 == 0  # (a no-op in the odd batches, switched off in the even ones)
    slots = toi_slots(a)
    assert slots > 64, "the ground's contacts are candidates already"
    a.set_bullets(bodies, flags)
    for q, f in zip(bodies.tolist(), flags.tolist()):
        b.set_bullet(q, f)
    same(a, b, "after the call", ids)
    assert toi_slots(a) == toi_slots(b)
    assert toi_slots(a) > slots, "no contact between two dynamic bodies became a candidate"
    s = a.body_states()
    assert (((s["flags"][bodies] & BULLET) != 0) == flags).all()
    step_and_compare(a, b, "bullets on", ids)
    # off again, in another order, with no-op entries among them (the ground and the kinematic body stay bullets)
    back = np.random.default_rng(3).permutation(bodies)
    off = ~np.isin(back, [ids["ground"], ids["kinematic"]])
    if size == 1:
        off[:] = True
    before = toi_slots(a)
    a.set_bullets(back, ~off)
    for q, f in zip(back.tolist(), (~off).tolist()):
        b.set_bullet(q, f)
    same(a, b, "bullets off", ids)
    assert toi_slots(a) < before
    step_and_compare(a, b, "bullets off", ids)
    a.close()
    b.close()


def bullet_world():
    """continuous physics: a floor, a wall of static and dynamic boxes in turn, sixteen balls - some in flight towards the wall,
    some at rest against its foot, some of them bullets (after the bullet_world of tests/test_gpu_fixture_batch.py).
    Returns (world, the bodies of the wall, the balls at rest, the bullets)."""
    w = b2hip.World(gravity=(0.0, -10.0), allow_sleep=True, continuous=True)
    ground = w.create_body(b2hip.STATIC, (0.0, -0.5))
    w.create_fixture(ground, b2hip.box_shape(40.0, 0.5))
    wall, resting, bullets = [], [], []
    for k in range(8):
        q = w.create_body(b2hip.STATIC if k % 2 == 0 else b2hip.DYNAMIC, (10.0, 0.25 + 0.5 * k))
        w.create_fixture(q, b2hip.box_shape(0.1, 0.25), density=2.0, friction=0.5)
        wall.append(q)
    for k in range(16):
        # (at rest: three bullets side by side, three plain balls side by side, a bullet, a plain ball - so that switching every
        # one of them changes the candidacy of the contacts INSIDE the runs and of no contact between them)
        is_bullet = k in (1, 3, 5, 13) if k % 2 else k % 4 == 0
        if k % 2 == 0:  # in flight, one behind the other and at several heights
            q = w.create_body(b2hip.DYNAMIC, (-2.0 - 1.5 * k, 0.6 + 0.25 * k), velocity=(60.0 + 5.0 * k, 0.0), bullet=is_bullet, gravity_scale=0.0)
        else:           # at rest on the floor, touching each other, the first against the wall's foot
            q = w.create_body(b2hip.DYNAMIC, (9.8 - 0.2 * (k // 2), 0.1), bullet=is_bullet)
            resting.append(q)
        w.create_fixture(q, b2hip.circle_shape(0.1), density=1.0, restitution=0.3)
        bullets += [q] if is_bullet else []
    for _ in range(4):
        w.step()
    return w, wall, resting, bullets


@pytest.mark.gpu
@pytest.mark.parametrize("sort_max,room", ((None, None), (2, None), (2, 1)))
def test_the_toi_partition_follows_the_loops_order(sort_max, room):
    """sort_max 2: B2HIP_TEST_LIFECYCLE_SORT_MAX lowers the one-workgroup sort's capacity, so that the list of this small world
    goes through the radix sort; room 1: B2HIP_TEST_FIXTURE_LIST_ROOM gives the first listing room for one contact, so that the
    call lists a second time (b2hip_debug_read 30 counts both: block K's contact pass shares block J's list)."""
    env = {"B2HIP_TEST_LIFECYCLE_SORT_MAX": sort_max, "B2HIP_TEST_FIXTURE_LIST_ROOM": room}
    for k, v in env.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        (a, wall, resting, bullets), b, c = bullet_world(), bullet_world()[0], bullet_world()[0]
    finally:
        for k in env:
            os.environ.pop(k, None)
    assert toi_slots(a) >= 6
    con = a.contacts()
    named = resting + wall[1:6]
    first = {int(q): int(np.flatnonzero((con["body_a"] == q) | (con["body_b"] == q))[0]) for q in named
             if ((con["body_a"] == q) | (con["body_b"] == q)).any()}
    by_contact = sorted(first, key=lambda q: first[q])
    assert len(by_contact) >= 4, "fewer than four of the bodies have contacts"
    head = [by_contact[1], by_contact[-1], by_contact[0]]
    assert wall[2] not in head
    bodies = ids_of(head + np.random.default_rng(7).permutation(np.setdiff1d(named, head + [wall[2]])).tolist() + [wall[2]])
    order = [first[q] for q in bodies.tolist() if q in first]
    assert order != sorted(order) and order != sorted(order)[::-1]
    both = np.isin(con["body_a"], bodies[:-1]) & np.isin(con["body_b"], bodies[:-1])
    assert both.any(), "no contact lies between two named bodies"
    have = np.zeros(a.body_count, bool)
    have[bullets] = True
    flag = ~have[bodies]            # every entry changes: on and off mixed
    flag[-1] = have[bodies[-1]]     # ... but the last, which has the requested value already
    assert flag.any() and not flag.all()
    # the batch as a whole changes at least three contacts between two balls at rest, some each way: more than the shrunk sort
    # takes, more than the shrunk room holds
    is_ball = np.isin(con["body_a"], resting) & np.isin(con["body_b"], resting)
    was = have[con["body_a"]] | have[con["body_b"]]
    assert np.count_nonzero(is_ball & was) >= 2 and np.count_nonzero(is_ball & ~was) >= 2
    # the twin of the twins says how many slots every entry frees (+) or adds (-)
    delta, slots = [], toi_slots(c)
    for q, v in zip(bodies.tolist(), flag.tolist()):
        c.set_bullet(q, v)
        now = toi_slots(c)
        delta.append(slots - now)
        slots = now
    assert np.count_nonzero(delta) >= 2 and min(delta) < 0 < max(delta), delta
    before = toi_slots(a)
    a.set_bullets(bodies, flag)
    for q, v in zip(bodies.tolist(), flag.tolist()):
        b.set_bullet(q, v)
    assert before - toi_slots(a) == sum(delta) and toi_slots(a) == toi_slots(b) == slots
    assert a.contacts().tobytes() == b.contacts().tobytes() and a.body_states().tobytes() == b.body_states().tobytes()
    snapshots_equal(a.save_snapshot(), b.save_snapshot(), "after the call")
    long_sorts, relists = debug_stats(a, 30, 2)
    assert (long_sorts >= 1) == (sort_max is not None) and (relists >= 1) == (room is not None), (long_sorts, relists)
    for k in range(25):
        a.step()
        b.step()
        assert a.contacts().tobytes() == b.contacts().tobytes(), "continuous, step %d: contacts differ" % (k + 1)
        assert a.body_states().tobytes() == b.body_states().tobytes(), "continuous, step %d: body states differ" % (k + 1)
    snapshots_equal(a.save_snapshot(), b.save_snapshot(), "after 25 continuous steps")
    for w in (a, b, c):
        w.close()


# ---- 4. fixed rotation and mass data ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_fixed_rotations_and_mass_datas_equal_the_single_calls(size):
    a, b, ids = twins(continuous=True)
    bodies = batch_of(a, ids, size, 400 + size, single="spin")
    assert ids["spin"] in bodies
    n = len(bodies)
    if size != 1:
        for name in ("fixedrot", "kinematic", "ground", "mouse", "inactive"):
            assert ids[name] in bodies
        assert asleep(a)[bodies].any()
    # -- fixed rotation: on for all but the fixed-rotation body, which is let go; every third keeps what it has (a no-op)
    has = (a.body_states()["flags"][bodies] & FIXEDROT) != 0
    flags = np.where(np.arange(n) % 3 == 2, has, ~has)
    flags[bodies == ids["spin"]] = True
    assert (flags != has).any() and (size == 1 or (flags == has).any())
    before = a.body_states()
    a.set_fixed_rotations(bodies, flags)
    for q, f in zip(bodies.tolist(), flags.tolist()):
        b.set_fixed_rotation(q, f)
    same(a, b, "fixed rotations", ids)
    s = a.body_states()
    assert before["w"][ids["spin"]] != 0.0 and s["w"][ids["spin"]] == 0.0
    assert (((s["flags"][bodies] & FIXEDROT) != 0) == flags).all()
    assert a.mass_data(ids["spin"])["inv_inertia"] == 0.0
    step_and_compare(a, b, "fixed rotations", ids, 2)
    a.set_fixed_rotations(bodies, has)
    for q, f in zip(bodies.tolist(), has.tolist()):
        b.set_fixed_rotation(q, f)
    a.set_velocities(ids_of([ids["spin"]]), omega=2.0)
    b.set_velocity(ids["spin"], (float(s["vx"][ids["spin"]]), float(s["vy"][ids["spin"]])), 2.0)
    same(a, b, "fixed rotations back", ids)
    # -- explicit mass data: the centre moves (the spinning body's velocity changes); mass <= 0, inertia == 0
    rng = np.random.default_rng(size)
    mass = rng.uniform(0.5, 3.0, n).astype(f32)
    inertia = rng.uniform(0.5, 2.0, n).astype(f32)
    center = rng.uniform(-0.2, 0.2, (n, 2)).astype(f32)
    mass[np.arange(n) % 5 == 1] = 0.0
    mass[np.arange(n) % 5 == 2] = -1.0
    inertia[np.arange(n) % 4 == 3] = 0.0
    at = int(np.flatnonzero(bodies == ids["spin"])[0])
    mass[at], inertia[at], center[at] = 2.0, 1.5, (-0.3, 0.4)
    before = a.body_states()
    a.set_mass_datas(bodies, mass, inertia, center)
    for q, m, i, c in zip(bodies.tolist(), mass.tolist(), inertia.tolist(), center.tolist()):
        b.set_mass_data(q, m, i, c)
    same(a, b, "mass data", ids)
    s = a.body_states()
    spin = ids["spin"]
    assert (s["vx"][spin], s["vy"][spin]) != (before["vx"][spin], before["vy"][spin]) and (s["cx"][spin], s["cy"][spin]) != (before["cx"][spin], before["cy"][spin])
    assert (s["px"][spin], s["py"][spin]) == (before["px"][spin], before["py"][spin])
    md = mass_datas(a)
    dynamic = (s["flags"][bodies] & 3) == b2hip.DYNAMIC
    assert (md["mass"][bodies[dynamic & (mass <= 0.0)]] == 1.0).all()
    assert (md["inv_inertia"][bodies[dynamic & (inertia == 0.0)]] == 0.0).all()
    if size != 1:
        for name in ("kinematic", "ground"):  # explicit mass data leave a body that is not dynamic alone
            assert md["mass"][ids[name]] == 0.0 and s[ids[name]].tobytes() == before[ids[name]].tobytes()
    step_and_compare(a, b, "mass data", ids, 3)  # (continuous steps: the sweep origin moved with the centre; the mouse joint reads the mass)
    # -- densities changed by the batched fixture call, then the bodies weighed again
    fixtures = ids_of([f for q in bodies.tolist() for f in ids["fixtures"][q]])
    density = np.random.default_rng(size + 1).uniform(0.5, 4.0, len(fixtures)).astype(f32)
    density[::7] = 0.0
    for w in (a, b):
        w.fixture_set_materials(fixtures, density=density)
    a.reset_mass_datas(bodies)
    for q in bodies.tolist():
        b.set_mass_data(q)
    same(a, b, "mass data reset", ids)
    assert mass_datas(a)[bodies].tobytes() != md[bodies].tobytes()
    step_and_compare(a, b, "mass data reset", ids, 3)
    a.close()
    b.close()


# ---- 5. types --------------------------------------------------------------------------------------------------------------------
def prepare_types(worlds, ids):
    """a second static and a second kinematic body, by single calls on every twin and a step: a batch can then hold all six
    transitions"""
    for w in worlds:
        w.set_type(ids["far"], b2hip.STATIC)
        w.set_type(ids["two"], b2hip.KINEMATIC)
        w.step()


def type_targets(w, ids, bodies):
    """all six transitions and same-type entries: by default dynamic bodies turn static, kinematic or stay in turn; the ground
    turns dynamic, the kinematic body static, a sleeping stack bottom static, an awake grid body kinematic, the jointed pair
    static and kinematic; after prepare_types the far body (static) turns kinematic and the two-fixture body (kinematic) dynamic"""
    s = w.body_states()
    have = (s["flags"][bodies] & 3).astype(np.uint8)
    want = np.where(np.arange(len(bodies)) % 3 == 0, b2hip.STATIC, np.where(np.arange(len(bodies)) % 3 == 1, b2hip.KINEMATIC, b2hip.DYNAMIC)).astype(np.uint8)
    stack = sleeping_stack(w, ids)
    for body, t in ((ids["ground"], b2hip.DYNAMIC), (ids["kinematic"], b2hip.STATIC), (grid_body(ids, stack, 0), b2hip.STATIC),
                    (awake_grid_body(w, ids), b2hip.KINEMATIC), (ids["pair"][0], b2hip.STATIC), (ids["pair"][1], b2hip.KINEMATIC),
                    (ids["inactive"], b2hip.KINEMATIC), (ids["three"], b2hip.STATIC), (ids["far"], b2hip.KINEMATIC), (ids["two"], b2hip.DYNAMIC)):
        want[bodies == body] = t
    return have, want


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
@pytest.mark.parametrize("size", SIZES)
def test_types_equal_the_single_calls_on_a_twin(size, lazy):
    a, b, ids = twins(continuous=True, lazy=lazy)
    prepare_types((a, b), ids)
    bodies = batch_of(a, ids, size, 500 + size)
    have, want = type_targets(a, ids, bodies)
    if size != 1:
        assert (have == want).any() and a.body_states()["flags"][ids["inactive"]] & ACTIVE == 0
        assert {(int(h), int(t)) for h, t in zip(have, want)} >= {(h, t) for h in range(3) for t in range(3) if h != t}, "not all six transitions"
        assert asleep(a)[bodies[want == b2hip.STATIC]].any() and (~asleep(a)[bodies[want == b2hip.KINEMATIC]]).any()
    n_before = len(a.contacts())
    moves_before = buffered_moves(a)
    a.set_types(bodies, want)
    for q, t in zip(bodies.tolist(), want.tolist()):
        b.set_type(q, t)
    same(a, b, "after the call", ids)
    s = a.body_states()
    assert ((s["flags"][bodies] & 3) == want).all()
    changed = bodies[have != want]
    assert (s["flags"][changed] & AWAKE).all() and not s["sleep_time"][changed].any()
    assert len(a.contacts()) < n_before
    active_changed = [f for q in changed.tolist() if s["flags"][q] & ACTIVE for f in ids["fixtures"][q]]
    assert buffered_moves(a) - moves_before == len(active_changed) == buffered_moves(b) - moves_before
    assert debug_stats(a, 32, 1) == (0,), "the to-static refit fall-back ran"
    step_and_compare(a, b, "types", ids, 3)
    # the second round undoes the first with later single calls on the same bodies mixed in: every body back to what it was
    half = len(bodies) // 2
    a.set_types(bodies[:half], have[:half])
    for q, t in zip(bodies[:half].tolist(), have[:half].tolist()):
        b.set_type(q, t)
    same(a, b, "half the types back", ids)  # (read here on both: each route has compacted the contact array once more)
    for w in (a, b):
        for q, t in zip(bodies[half:].tolist(), have[half:].tolist()):
            w.set_type(q, t)
    same(a, b, "types back", ids)
    assert ((a.body_states()["flags"][bodies] & 3) == have).all()
    step_and_compare(a, b, "types back", ids, 3)
    a.close()
    b.close()


@pytest.mark.gpu
def test_the_end_events_of_a_type_batch_are_delivered_with_the_next_step():
    """The ground turned dynamic: every stack bottom's contact ends. (Nothing is read between the calls and the step: the single
    route applies its queued operations inside that step, which is where its end events are delivered from; a read of the
    contacts in between would apply them early, and the step that follows starts its event list afresh.)"""
    a, b, ids = twins(events=True, continuous=True)
    prepare_types((a, b), ids)
    bodies = batch_of(a, ids, 65, 565)
    have, want = type_targets(a, ids, bodies)
    assert want[bodies == ids["ground"]] == b2hip.DYNAMIC
    a.set_types(bodies, want)
    for q, t in zip(bodies.tolist(), want.tolist()):
        b.set_type(q, t)
    a.step()
    b.step()
    ea, eb = sorted_events(a), sorted_events(b)
    ground = ids["fixtures"][ids["ground"]][0]
    ended = ((ea[:, 0] == ground) | (ea[:, 1] == ground)) & (ea[:, 2] == 1) & (ea[:, 3] == -1)
    assert ended.sum() >= STACKS, "the end events of the ground's contacts are missing"
    assert ea.tobytes() == eb.tobytes(), "the events differ from the twin's"
    # (no snapshot of THIS step: the batch's end events were fetched when it was made and are delivered by the host with this
    # step's list - block I's carried events - while the single route's operations append theirs on the device inside the step;
    # the device's count of the events it appended this step differs by exactly those. The next step starts the list afresh.)
    same(a, b, "after the step", ids, snapshots=False)
    step_and_compare(a, b, "types with events", ids, 3, events=True)
    a.close()
    b.close()


@pytest.mark.gpu
def test_the_move_buffer_is_guarded():
    a, b, ids = twins()
    bodies = ids_of(np.random.default_rng(7).permutation(a.body_count))
    s = a.body_states()
    have = (s["flags"][bodies] & 3).astype(np.uint8)
    other = np.where(have == b2hip.DYNAMIC, b2hip.KINEMATIC, b2hip.DYNAMIC).astype(np.uint8)
    refusals = 0
    for k in range(10):
        want = other if k % 2 == 0 else have
        before, con_before = a.body_states(), a.contacts()
        rc = a.L.b2hip_set_types(a.p, len(bodies), bodies.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p))
        if k == 0:
            assert rc == 0, "a type batch over every body of a freshly stepped world must fit"
        if rc == 0:
            for q, t in zip(bodies.tolist(), want.tolist()):
                b.set_type(q, t)
            continue
        refusals += 1
        assert rc == ERR_UNSUPPORTED, rc
        msg = a.L.b2hip_last_error().decode()
        assert "step" in msg and "move buffer" in msg, msg
        assert a.body_states().tobytes() == before.tobytes() and a.contacts().tobytes() == con_before.tobytes(), "a refused call changed the world"
        break
    assert refusals == 1, "ten rounds of type changes fitted a buffer of 2 x fixtures + 64 moves"
    same(a, b, "after the calls that were accepted", ids)
    step_and_compare(a, b, "after the guard", ids, 2)
    a.close()
    b.close()


# ---- 6. mixing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lazy", (False, True))
def test_single_calls_before_and_after_the_batches(lazy):
    a, b, ids = twins(lazy=lazy, continuous=True)
    bodies = batch_of(a, ids, 65, 665)
    stack = sleeping_stack(a, ids, 1)
    some = [grid_body(ids, stack, 0), ids["two"], ids["spin"], ids["bullet"]]
    assert all(q in bodies for q in some[1:])
    have, want = type_targets(a, ids, bodies)  # (read before anything is queued: nothing but the calls below touches a world)
    want[bodies == ids["far"]] = b2hip.STATIC
    for w in (a, b):  # single calls queued before the batches: they lie underneath them
        w.set_bullet(some[0], True)
        w.set_type(some[1], b2hip.KINEMATIC)
        w.set_body_damping(some[2], 0.25, 0.5, 0.75)
        w.set_fixed_rotation(some[2], True)
        w.set_velocity(ids["two"], (0.5, 0.0), 0.25)
        w.set_sleeping_allowed(some[3], False)
    flags = np.arange(len(bodies)) % 2 == 0
    a.set_types(bodies, want)
    a.set_bullets(bodies, flags)
    a.set_body_dampings(bodies, linear=0.125)
    a.set_fixed_rotations(bodies, ~flags)
    a.set_sleeping_alloweds(bodies, flags)
    a.reset_mass_datas(bodies)
    for q, t in zip(bodies.tolist(), want.tolist()):
        b.set_type(q, t)
    for q, f in zip(bodies.tolist(), flags.tolist()):
        b.set_bullet(q, f)
    damp = ids["damping"].copy()
    damp[some[2]] = (0.25, 0.5, 0.75)
    for q in bodies.tolist():
        b.set_body_damping(q, 0.125, float(damp[q, 1]), float(damp[q, 2]))
    for q, f in zip(bodies.tolist(), flags.tolist()):
        b.set_fixed_rotation(q, not f)
    for q, f in zip(bodies.tolist(), flags.tolist()):
        b.set_sleeping_allowed(q, f)
    for q in bodies.tolist():
        b.set_mass_data(q)
    for w in (a, b):  # single calls after the batches on the same bodies
        for q in bodies[:9].tolist():
            w.set_type(q, b2hip.DYNAMIC)
            w.set_bullet(q, True)
            w.set_fixed_rotation(q, False)
            w.set_mass_data(q, 1.5, 0.75, (0.1, -0.1))
            w.set_awake(q, True)
    same(a, b, "single calls and batches mixed", ids)
    step_and_compare(a, b, "mixed", ids, 3)
    a.close()
    b.close()


# ---- 7. refusals apply nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_calls_name_the_offender_and_apply_nothing():
    a, b, ids = twins()
    n = a.body_count
    victim = ids["grid"][7]
    for w in (a, b):
        w.destroy_body(victim)
    con_before = a.contacts()  # (first: the read applies the single call's queued operation, which wakes the victim's neighbours)
    before, mass_before, damp_before = a.body_states(), mass_datas(a), damping_rows(a)
    good = np.asarray(ids["grid"][20:30], np.int32)
    calls = (lambda q: a.set_types(q, b2hip.STATIC), lambda q: a.set_bullets(q, True), lambda q: a.set_fixed_rotations(q, True),
             lambda q: a.set_sleeping_alloweds(q, False), lambda q: a.set_body_dampings(q, linear=0.5),
             lambda q: a.set_mass_datas(q, 2.0, 1.0, (0.1, 0.1)), lambda q: a.reset_mass_datas(q))

    def unchanged():
        assert a.body_states().tobytes() == before.tobytes() and a.contacts().tobytes() == con_before.tobytes()
        assert mass_datas(a).tobytes() == mass_before.tobytes() and damping_rows(a).tobytes() == damp_before.tobytes()

    def refused(bodies, words):
        bodies = np.asarray(bodies, np.int32)
        for call in calls:
            with pytest.raises(b2hip.B2HipError) as e:
                call(bodies)
            for word in words:
                assert word in str(e.value), (word, str(e.value))
        unchanged()

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
    # a bad type, a bad mask: looked at before the ids
    types = np.full(len(good), b2hip.STATIC, np.uint8)
    types[4] = 3
    bad[3] = n
    assert a.L.b2hip_set_types(a.p, len(bad), bad.ctypes.data_as(C.c_void_p), types.ctypes.data_as(C.c_void_p)) == ERR_INVALID
    msg = a.L.b2hip_last_error().decode()
    assert "entry 4" in msg and "type 3" in msg, msg
    rec = np.zeros(len(good), b2hip.BODY_DAMPING_DTYPE)
    for mask in (0, 8, 15, -1):
        assert a.L.b2hip_set_body_dampings(a.p, len(bad), bad.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), mask) == ERR_INVALID
        assert "mask" in a.L.b2hip_last_error().decode()
    unchanged()
    # inside a step
    _check(a.L.b2hip_step_begin(a.p, C.c_float(1.0 / 60.0), 8, 3))
    for call in calls:
        with pytest.raises(b2hip.B2HipError) as e:
            call(good)
        assert "inside a step" in str(e.value)
    for fn in ("b2hip_collide", "b2hip_solve", "b2hip_sync_fixtures", "b2hip_find_new_contacts", "b2hip_solve_toi", "b2hip_step_end"):
        _check(getattr(a.L, fn)(a.p))
    b.step()
    same(a, b, "a step after the refused calls", ids)
    # n == 0 succeeds
    none = np.zeros(0, np.int32)
    for call in calls:
        call(none)
    a.step()
    b.step()
    same(a, b, "after the empty calls", ids)
    a.close()
    b.close()
