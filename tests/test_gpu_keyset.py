"""GPU: the contact-key hash set the pair update keeps across steps (box2d-mt_amd/csrc/b2d_kernels_collide.h: "contact key hash
set"; B2HIP_KEYSET_KEEP, default on) against a world created under B2HIP_KEYSET_KEEP=0, which clears and builds the set in
every pair update as before.

The kept set may change nothing: at every stop b2hip_debug_hash 0 (bodies), 1 (contacts) and 2 (fat AABBs) of the two worlds
are equal, exactly. And wherever the kept world reports its set valid, b2hip_test_keyset_check is clean: no live contact's key
missing, no dead contact's entry left, recounted fill = tracked fill. The statistics (b2hip_debug_read 23) show that the case
went down the path it is there for: updates that kept the set, rebuilds by the cause in question."""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
from spatial_util import SpatialRanks

pytestmark = pytest.mark.gpu

CCD = bh.F_CONTINUOUS | bh.F_SLEEP | bh.F_WARM
KEPT, INVALID, STALE, MASK, FILL, SHARDED, OFF, TOMBSTONES, INSERTS, NOT_FOUND, FILL_NOW, MASK_NOW = range(12)


def _lib():
    L = b2hip.lib()
    L.b2hip_debug_hash.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.b2hip_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.b2hip_test_keyset_check.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    return L


def _ptr(w):
    """b2hip_world* of a harness world or of a b2hip.World"""
    return w.device_world() if hasattr(w, "device_world") else w.p


def hashes(w):
    L, out = _lib(), []
    for which in (0, 1, 2):
        h = C.c_uint64()
        assert L.b2hip_debug_hash(_ptr(w), which, C.byref(h)) == 0
        out.append(h.value)
    return out


def stats(w):
    out = (C.c_longlong * 12)()
    assert _lib().b2hip_debug_read(_ptr(w), 23, 0, 12, out) == 0
    return list(out)


def check(w):
    out = (C.c_longlong * 6)()
    assert _lib().b2hip_test_keyset_check(_ptr(w), out) == 0, b2hip.lib().b2hip_last_error()
    return list(out)


def stop(kept, plain, what):
    """One stop: the two worlds are equal, the kept set (where it is valid) is right. Returns whether it was valid."""
    assert hashes(kept) == hashes(plain), what
    valid, missing, surplus, fill_off, live, tombs = check(kept)
    if valid:
        assert (missing, surplus, fill_off) == (0, 0, 0), "%s: key set check %s (%d live entries, %d tombstones)" % (
            what, (missing, surplus, fill_off), live, tombs)
    return bool(valid)


def pair(make, monkeypatch):
    """(a world with the set kept, the same world under B2HIP_KEYSET_KEEP=0)"""
    monkeypatch.delenv("B2HIP_KEYSET_KEEP", raising=False)
    kept = make()
    monkeypatch.setenv("B2HIP_KEYSET_KEEP", "0")
    plain = make()
    monkeypatch.delenv("B2HIP_KEYSET_KEEP", raising=False)
    return kept, plain


def plain_stats_are_todays(plain):
    st = stats(plain)
    assert st[KEPT] == 0 and st[OFF] > 0 and sum(st[INVALID:SHARDED + 1]) == 0 and st[TOMBSTONES] == 0 and st[INSERTS] == 0, st


def test_churn_and_growing_masks(amd, monkeypatch):
    """Tumbler 60 x 60 from its start grid: the contact count climbs from 0 through several powers of two (rebuilds by mask),
    and contacts come and go every step in between (inserts, tombstones)."""
    monkeypatch.delenv("B2HIP_KEYSET_MAX_FILL", raising=False)
    a, b = pair(lambda: amd.world(bh.TUMBLER, p0=60), monkeypatch)
    valid = 0
    for k in range(12):
        a.step(10)
        b.step(10)
        valid += stop(a, b, "after %d steps" % (10 * (k + 1)))
    st = stats(a)
    print("tumbler 60, 120 steps:", st)
    assert valid > 0
    assert st[KEPT] > 0 and st[MASK] > 0 and st[TOMBSTONES] > 0 and st[INSERTS] > 0, st
    assert st[NOT_FOUND] == 0 and st[OFF] == 0 and st[SHARDED] == 0, st
    plain_stats_are_todays(b)
    a.close()
    b.close()


def test_fill_driven_rebuild(amd, monkeypatch):
    """The same scene under B2HIP_KEYSET_MAX_FILL=25: live keys are less than a quarter of the slots after a rebuild (the mask
    is chosen so), tombstones take the set over the limit, it is rebuilt and kept again. (30 is not reached on this scene:
    120 steps end at 78 072 of 262 144 slots, 29.8 %. 25 is the lowest limit a rebuild always gets under.)"""
    monkeypatch.setenv("B2HIP_KEYSET_MAX_FILL", "25")
    a, b = pair(lambda: amd.world(bh.TUMBLER, p0=60), monkeypatch)
    monkeypatch.delenv("B2HIP_KEYSET_MAX_FILL", raising=False)
    kept_at_first_fill = None
    for k in range(12):
        a.step(10)
        b.step(10)
        stop(a, b, "after %d steps" % (10 * (k + 1)))
        st = stats(a)
        if st[FILL] > 0 and kept_at_first_fill is None:
            kept_at_first_fill = st[KEPT]
    st = stats(a)
    print("tumbler 60, 120 steps, fill limit 25 %:", st, check(a))
    assert st[FILL] >= 1, st
    assert kept_at_first_fill is not None and st[KEPT] > kept_at_first_fill > 0, (kept_at_first_fill, st)
    assert st[NOT_FOUND] == 0, st
    a.close()
    b.close()


@pytest.mark.parametrize("count,seed,flags", [(48, 5, CCD), (36, 2, bh.DEFAULT_FLAGS)])
def test_scripted_edits_between_steps(amd, monkeypatch, count, seed, flags):
    """The life-cycle scene as tests/test_lifecycle.py steps it: bodies and fixtures destroyed in a heap, new ones created
    (proxy ids reused), filter data changed, bodies switched off and on, types changed."""
    a, b = pair(lambda: amd.world(bh.LIFECYCLE, count, 0, seed=seed, flags=flags), monkeypatch)
    valid = 0
    for s in range(240):
        a.step(1)
        b.step(1)
        valid += stop(a, b, "step %d" % s)
    st = stats(a)
    print("life cycle %d:" % count, st)
    assert valid > 0 and st[KEPT] > 0 and st[TOMBSTONES] > 0 and st[INSERTS] > 0 and st[NOT_FOUND] == 0, st
    a.close()
    b.close()


def test_hand_made_edits_reuse_dead_slots(monkeypatch):
    """A few hundred boxes in a tray: every fifth step some are destroyed and new ones are created in the same places (their
    contacts' keys die and new keys are inserted, into tombstones where the probe paths cross), and touching fixtures are
    re-filtered (the pairs whose filter now refuses them lose their contacts in the next Collide)."""
    def make():
        w = b2hip.World(gravity=(0.0, -10.0))
        g = w.create_body(b2hip.STATIC)
        w.create_fixture(g, b2hip.box_shape(30.0, 0.5))
        w.create_fixture(g, b2hip.edge_shape((-12.0, 0.0), (-12.0, 30.0)))
        w.create_fixture(g, b2hip.edge_shape((12.0, 0.0), (12.0, 30.0)))
        w.boxes = {}
        for i in range(300):
            w.boxes[i] = spawn(w, i)
        return w

    def spawn(w, i, group=0):
        body = w.create_body(b2hip.DYNAMIC, position=(-11.0 + 1.1 * (i % 20), 1.0 + 1.05 * (i // 20)))
        fx = w.create_fixture(body, b2hip.box_shape(0.5, 0.5), density=1.0, friction=0.3, group=group)
        return body, fx

    a, b = pair(make, monkeypatch)
    valid = 0
    for s in range(60):
        if s % 5 == 4:
            for w in (a, b):
                for i in range(s % 7, 300, 23):
                    w.destroy_body(w.boxes[i][0])
                    # (group -1: the new boxes do not collide with one another - where two of them touch, no contact)
                    w.boxes[i] = spawn(w, i, group=-1 if s % 10 == 9 else 0)
                for i in range(3, 300, 17):
                    w.fixture_refilter(w.boxes[i][1])
        a.step()
        b.step()
        valid += stop(a, b, "step %d" % s)
    st = stats(a)
    print("hand-made edits:", st)
    assert valid > 0 and st[KEPT] > 0 and st[TOMBSTONES] > 0 and st[INSERTS] > 0 and st[NOT_FOUND] == 0, st
    a.close()
    b.close()


@pytest.mark.parametrize("name,scene,p0,p1", [("bullets", bh.BULLETS, 60, 6), ("field 2 000 / 50 bullets", bh.FIELD, 2000, 50)])
def test_continuous_physics_marks_the_set_stale(amd, monkeypatch, name, scene, p0, p1):
    """TOI sub-steps create contacts (and a phase that is taken back drops them) without the pair update's kernels: the set
    is marked stale and the next pair update rebuilds it (the TOI phase does not maintain the set)."""
    a, b = pair(lambda: amd.world(scene, p0, p1, flags=CCD), monkeypatch)
    valid = 0
    for k in range(12):
        a.step(5)
        b.step(5)
        valid += stop(a, b, "%s: after %d steps" % (name, 5 * (k + 1)))
    st = stats(a)
    print(name, st, "valid stops", valid)
    assert st[STALE] >= 1 and st[NOT_FOUND] == 0, st
    assert valid >= 1 and st[KEPT] >= 1, "the set was never kept between TOI events: the self-check never ran (%d, %s)" % (valid, st)
    a.close()
    b.close()


def test_a_loaded_snapshot_builds_its_set(amd, monkeypatch):
    """Tumbler 40 x 40 saved at step 50, the set kept and partly tombstoned: the set is not part of the snapshot, the loaded
    world's first pair update rebuilds it ("invalid"), and 20 further steps are the original's."""
    a, b = pair(lambda: amd.world(bh.TUMBLER, p0=40), monkeypatch)
    a.step(50)
    b.step(50)
    assert stop(a, b, "step 50"), "the set is not kept at step 50"
    st = stats(a)
    assert st[KEPT] > 0 and st[TOMBSTONES] > 0 and check(a)[5] > 0, st
    c = b2hip.World.from_snapshot(b2hip.World.borrow(a.device_world()).save_snapshot())
    assert stats(c)[:MASK_NOW] == [0] * MASK_NOW and check(c)[0] == 0
    for s in range(20):
        a.step(1)
        b.step(1)
        c.step(1.0 / 60.0, a.vel_iters, a.pos_iters)
        assert hashes(c) == hashes(a), "the loaded world parts from the original at step %d after the snapshot" % s
        stop(a, b, "step %d after the snapshot" % s)
        stop(c, b, "loaded world, step %d after the snapshot" % s)
        if s == 0:
            st = stats(c)
            assert st[INVALID] == 1 and sum(st[STALE:OFF + 1]) == 0, st
    st = stats(c)
    assert st[INVALID] == 1 and st[KEPT] > 0, st
    a.close()
    b.close()
    c.close()


def test_growing_buffers_leave_a_clean_set(monkeypatch):
    """The dense start of tests/test_gpu_edge_cases.py::test_dense_start_grows_the_pair_buffer: the first pair update overflows
    the pair buffer, the arrays (the hash table with them) are re-allocated and the update runs again. Continuous physics off
    (as tests/test_gpu_spatial.py runs this arena): no TOI phase marks the set stale, so the one stale rebuild is the
    re-allocation's, and the set is kept - and checked - from then on."""
    monkeypatch.setenv("B2HIP_FORCE_LARGE", "2")
    amd = bh.Harness(bh.AMD_LIB)
    kw = dict(p0=1406, p1=456, f0=35.0, f1=2.0, seed=2623, flags=bh.F_SLEEP | bh.F_WARM)
    a, b = pair(lambda: amd.world(bh.FIELD, **kw), monkeypatch)
    valid = 0
    for s in range(5):
        a.step(1)
        b.step(1)
        assert a.contact_count > 15000
        valid += stop(a, b, "step %d" % s)
    st = stats(a)
    print("dense start:", st, "valid stops", valid)
    assert st[STALE] >= 1, "ht_keys was not re-allocated under a built set: %s" % st
    assert valid >= 1 and st[KEPT] >= 1 and st[NOT_FOUND] == 0, (valid, st)
    a.close()
    b.close()


def test_a_sharded_world_builds_its_set_every_update(amd, monkeypatch):
    """Two ranks in one process, spatial ownership: CF_FOREIGN of a contact changes with the ownership of its bodies, so a
    sharded world never keeps the set - with the switch on or off the ranks hold the same worlds."""
    monkeypatch.setenv("B2HIP_SHARD_FULL_ROWS", "1")
    L = b2hip.lib()

    def make():
        ws = [amd.world(bh.FIELD, 3000, 300, seed=3, flags=CCD) for _ in range(2)]
        return ws, SpatialRanks(L, [(w, w.device_world()) for w in ws])

    (wa, ra), (wb, rb) = pair(make, monkeypatch)
    for k in range(4):
        for _ in range(5):
            ra.step()
            rb.step()
        for r in range(2):
            assert hashes(wa[r]) == hashes(wb[r]), "rank %d after %d steps" % (r, 5 * (k + 1))
            assert check(wa[r])[0] == 0
    for r in range(2):
        st = stats(wa[r])
        assert st[KEPT] == 0 and st[SHARDED] > 0 and st[TOMBSTONES] == 0 and st[INSERTS] == 0, st
        assert stats(wb[r])[KEPT] == 0
    for w in wa + wb:
        w.close()
