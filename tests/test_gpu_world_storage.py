"""GPU: who owns a world's memory (box2d-mt_amd/csrc/b2hip_host_world.h: DevArray, PinnedBuf, the tables WORLD_ARRAYS_DW /
WORLD_ARRAYS_HOST), through the test hook b2hip_test_storage.

1. Nothing outlives a world: the count of blocks the two owner types hold in this process is back where it was once a world is
   destroyed - a world that has stepped, grown its on-demand arrays (a call of every batched family) and lost a body, twice in
   a row, and a world with nothing in it.
2. The kernels' argument block follows every growth: at no stop does DW hold a pointer that is not its array's current one.
3. A world created after others were destroyed is the same world: the pyramid built whole, and built in two stages with steps
   in between (its arrays grow under a world that has run), give the same body states and contacts, bit for bit, the second
   time round. Two runs of the same code: what is right is the parity suite's business."""
import ctypes as C
import gc

import numpy as np
import pytest

import b2hip

pytestmark = pytest.mark.gpu

BASE = 10                       # the pyramid's base: 55 boxes
BOXES = BASE * (BASE + 1) // 2
RADIX_TILE = 2048               # box2d-mt_amd/csrc/b2d_scan.h

FILTER_BATCH_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
PRE_SOLVE_BATCH_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p)


def _lib():
    L = b2hip.lib()
    L.b2hip_test_storage.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    L.b2hip_test_radix_sort.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.b2hip_default_should_collide.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.b2hip_set_contact_filter_batch.argtypes = [C.c_void_p, FILTER_BATCH_FN, C.c_void_p]
    L.b2hip_set_pre_solve_batch.argtypes = [C.c_void_p, PRE_SOLVE_BATCH_FN, C.c_void_p]
    L.b2hip_enable_post_solve.argtypes = [C.c_void_p, C.c_int]
    return L


def storage(w=None):
    """(live blocks in this process, stale pointers in w's argument block)"""
    out = (C.c_longlong * 2)()
    assert _lib().b2hip_test_storage(w.p if w is not None else None, out) == 0, b2hip.lib().b2hip_last_error()
    return out[0], out[1]


def live_blocks():
    gc.collect()  # (a world an earlier test dropped without close() goes now, not in the middle of a count)
    return storage()[0]


def install_callbacks(w):
    """contact events, PreSolve (every contact stays enabled), PostSolve, a contact filter (the built-in rule): the listener
    arrays become contact-sized. Returns what must stay alive as long as the world."""
    L = _lib()

    def should_collide(user, count, pairs, verdict):
        for k in range(count):
            verdict[k] = L.b2hip_default_should_collide(w.p, pairs[2 * k], pairs[2 * k + 1])

    def pre_solve(user, count, records):
        pass

    keep = [FILTER_BATCH_FN(should_collide), PRE_SOLVE_BATCH_FN(pre_solve)]
    w.enable_contact_events(True)
    assert L.b2hip_set_contact_filter_batch(w.p, keep[0], None) == 0
    assert L.b2hip_set_pre_solve_batch(w.p, keep[1], None) == 0
    assert L.b2hip_enable_post_solve(w.p, 1) == 0
    return keep


def pyramid_positions():
    """row after row from the bottom, the boxes of a row 1/8 apart and a row 1/100 above the one below: in contact at once"""
    return [(1.125 * (k - 0.5 * (BASE - 1 - row)), 0.51 + 1.01 * row) for row in range(BASE) for k in range(BASE - row)]


def add_boxes(w, positions):
    out = []
    for p in positions:
        body = w.create_body(b2hip.DYNAMIC, position=p)
        out.append((body, w.create_fixture(body, b2hip.box_shape(0.5, 0.5), density=5.0)))
    return out


def make_world(boxes=BOXES, callbacks=True):
    """a ground, the first `boxes` boxes of the pyramid, a revolute joint between two extra bodies; continuous physics"""
    w = b2hip.World(gravity=(0.0, -10.0), continuous=True)
    w.keep = install_callbacks(w) if callbacks else []
    ground = w.create_body(b2hip.STATIC)
    w.create_fixture(ground, b2hip.edge_shape((-40.0, 0.0), (40.0, 0.0)))
    arm_a = w.create_body(b2hip.DYNAMIC, position=(-20.0, 4.0))
    arm_b = w.create_body(b2hip.DYNAMIC, position=(-19.0, 4.0))
    w.create_fixture(arm_a, b2hip.box_shape(0.5, 0.125), density=1.0)
    w.create_fixture(arm_b, b2hip.box_shape(0.5, 0.125), density=1.0)
    w.joint = w.create_revolute_joint(arm_a, arm_b, anchor_a=(0.5, 0.0), anchor_b=(-0.5, 0.0))
    w.arm = arm_a
    w.boxes = add_boxes(w, pyramid_positions()[:boxes])
    return w


# ---- 1. nothing outlives a world --------------------------------------------------------------------------------------------
def test_nothing_outlives_a_world():
    base = live_blocks()
    for round_ in range(2):
        w = make_world()
        for _ in range(3):
            w.step()
        ids = np.array([b for b, _ in w.boxes[:8]], np.int32)
        w.ray_cast_closest([(-30.0, 0.75), (0.0, 30.0)], [(30.0, 0.75), (0.0, 0.1)])
        w.body_contacts(ids)
        w.set_velocities(ids[:2], velocity=[(0.0, 0.0), (0.0, 0.0)])
        w.joint_states([w.joint])
        w.fixture_set_sensors([f for _, f in w.boxes[-5:-1]], True)
        w.destroy_bodies([w.boxes[-1][0]])
        w.step()
        assert w.body_count == BOXES + 3 and w.contact_count > BOXES
        assert storage(w)[0] > base, "round %d: a live world holds nothing" % round_
        w.close()
        assert live_blocks() == base, "round %d: blocks outlive the world" % round_


def test_nothing_outlives_an_empty_world():
    base = live_blocks()
    w = b2hip.World()
    assert storage(w)[0] > base
    w.close()
    assert live_blocks() == base


# ---- 2. the kernels' argument block follows every growth --------------------------------------------------------------------
def stale(w, where):
    assert storage(w)[1] == 0, "%s: %d pointers of the argument block are not their arrays'" % (where, storage(w)[1])


def test_the_argument_block_follows_every_growth():
    w = make_world()
    stale(w, "after creation")
    w.step()
    stale(w, "after the first step")
    # 57 bodies -> 127 (past 64: the per-body arrays double), 58 fixtures -> 128 (past 64 and, for the 2 * np + 64 ones, 256)
    add_boxes(w, [(-30.0 + 1.25 * (k % 35), 20.0 + 1.25 * (k // 35)) for k in range(70)])
    w.step()
    stale(w, "after 70 more bodies")
    # a sort over more tiles than the pair buffers have: the hook grows the radix and scan scratch itself
    n = 40 * RADIX_TILE + 5
    keys = np.random.default_rng(7).integers(0, 1 << 40, n, dtype=np.uint64)
    vals = np.zeros((n, 2), np.int32)
    shifts, widths = np.array([0, 11, 22, 33], np.int32), np.array([11, 11, 11, 7], np.int32)
    rc = w.L.b2hip_test_radix_sort(w.p, n, keys.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), 4,
                                   shifts.ctypes.data_as(C.c_void_p), widths.ctypes.data_as(C.c_void_p))
    assert rc == 0, w.L.b2hip_last_error()
    assert (np.diff(keys.astype(np.int64)) >= 0).all()
    stale(w, "after a sort beyond the pair buffers' tiles")
    w.step()
    stale(w, "after the step behind that sort")
    w.close()


def test_the_argument_block_follows_the_listener_arrays():
    w = make_world(callbacks=False)
    w.step()
    stale(w, "no callbacks")
    w.keep = install_callbacks(w)  # (one element each so far: contact-sized from the next step on)
    w.step()
    stale(w, "after installing the callbacks")
    assert w.contact_count > BOXES
    w.close()


# ---- 3. a grown world is the same world ---------------------------------------------------------------------------------------
def run_whole():
    w = make_world()
    for _ in range(30):
        w.step()
    return w


def run_staged():
    w = make_world(boxes=20)
    for _ in range(5):
        w.step()
    w.boxes += add_boxes(w, pyramid_positions()[20:])
    for _ in range(25):
        w.step()
    return w


@pytest.mark.parametrize("run", (run_whole, run_staged), ids=("whole", "staged"))
def test_a_world_after_a_destroyed_one_is_the_same_world(run):
    got = []
    for _ in range(2):
        w = run()
        assert w.body_count == BOXES + 3 and storage(w)[1] == 0
        got.append((w.body_states().tobytes(), w.contacts().tobytes(), w.contact_count))
        w.close()  # (the second world is created after this one is gone)
    assert got[0][2] > BOXES
    assert got[0] == got[1]
