"""GPU: the narrow phase that stores the compacted contact array itself (box2d-mt_amd/csrc/b2d_kernels_collide.h:
k_collide<0, false, true>; B2HIP_COLLIDE_COMPACT, default on) against a world created under B2HIP_COLLIDE_COMPACT=0, which runs
the split narrow phase, the scan of the keep flags and k_compact_contacts as before.

The fused form may change nothing: at every stop b2hip_debug_hash 0 (bodies), 1 (contacts) and 2 (fat AABBs) of the two worlds
are equal, exactly, and wherever the key set is valid b2hip_test_keyset_check is clean (the fused form writes the tombstones
of the contacts it drops). b2hip_debug_read 24 counts the narrow phases that took the fused form: it shows that a case went
down the path it is there for. B2HIP_COLLIDE_SPLIT=1 throughout, so that worlds this small take the split form at all."""
import ctypes as C

import pytest

import b2harness as bh
import b2hip
from test_gpu_keyset import _lib, _ptr, check, hashes

pytestmark = pytest.mark.gpu

CCD = bh.F_CONTINUOUS | bh.F_SLEEP | bh.F_WARM
PLAIN = bh.F_SLEEP | bh.F_WARM


def fused(w):
    """narrow phases of this world that stored the compacted array themselves"""
    out = C.c_longlong()
    assert _lib().b2hip_debug_read(_ptr(w), 24, 0, 1, C.byref(out)) == 0
    return out.value


def stop(a, b, what):
    assert hashes(a) == hashes(b), what
    valid, missing, surplus, fill_off, live, tombs = check(a)
    if valid:
        assert (missing, surplus, fill_off) == (0, 0, 0), "%s: key set check %s (%d live entries, %d tombstones)" % (
            what, (missing, surplus, fill_off), live, tombs)
    return bool(valid)


def pair(make, monkeypatch, chunk=None):
    """(a world that may take the fused form, the same world under B2HIP_COLLIDE_COMPACT=0)"""
    monkeypatch.setenv("B2HIP_COLLIDE_SPLIT", "1")
    monkeypatch.delenv("B2HIP_COLLIDE_COMPACT", raising=False)
    if chunk:
        monkeypatch.setenv("B2HIP_TEST_COLLIDE_CHUNK", str(chunk))
    a = make()
    monkeypatch.delenv("B2HIP_TEST_COLLIDE_CHUNK", raising=False)
    monkeypatch.setenv("B2HIP_COLLIDE_COMPACT", "0")
    b = make()
    monkeypatch.delenv("B2HIP_COLLIDE_COMPACT", raising=False)
    monkeypatch.delenv("B2HIP_COLLIDE_SPLIT", raising=False)
    return a, b


@pytest.mark.parametrize("chunk", [None, 32, 2])
def test_tumbler_churn(amd, monkeypatch, chunk):
    """Tumbler 40 x 40 (1 600 boxes, continuous physics off), 150 steps: contacts die and are born every step, the count is no
    multiple of the chunk and the survivors' places cross chunk boundaries. With 256 contacts per workgroup the look-back
    reads the counts of two groups of 64 chunks; with 32 (B2HIP_TEST_COLLIDE_CHUNK) there are a thousand chunks in sixteen
    groups, so a chunk's place is the sum of its own group's counts and of many groups' sums; with 2 a chunk looks back
    over more words than the workgroup has lanes (63 counts and 250 sums: a second round)."""
    a, b = pair(lambda: amd.world(bh.TUMBLER, p0=40, flags=PLAIN), monkeypatch, chunk)
    valid, most = 0, 0
    for k in range(15):
        a.step(10)
        b.step(10)
        valid += stop(a, b, "after %d steps" % (10 * (k + 1)))
        most = max(most, a.contact_count)
    print("tumbler 40, chunk %s: fused %d of 150, most contacts %d, key set valid at %d stops" % (chunk, fused(a), most, valid))
    # (every narrow phase but the first, which comes before the world's first read-back)
    assert fused(a) == 149 and fused(b) == 0
    assert most > 64 * (chunk or 256), "the look-back never went past one group of chunks"
    assert chunk != 2 or most > 2 * (256 - 63) * 64, "the look-back never took a second round"
    assert valid > 0
    a.close()
    b.close()


def tray(n):
    """n boxes in rows of 20 on a static floor between two walls, a little apart: they drop a few centimetres and rest"""
    w = b2hip.World(gravity=(0.0, -10.0))
    g = w.create_body(b2hip.STATIC)
    # (thick shapes: a contact between a box and a static fixture that is not thick would be a TOI candidate, see
    # test_toi_candidates_keep_the_old_path)
    w.create_fixture(g, b2hip.box_shape(30.0, 0.5), thick=True)
    w.create_fixture(g, b2hip.edge_shape((-12.0, 0.0), (-12.0, 30.0)), thick=True)
    w.create_fixture(g, b2hip.edge_shape((12.0, 0.0), (12.0, 30.0)), thick=True)
    w.boxes = []
    for i in range(n):
        body = w.create_body(b2hip.DYNAMIC, position=(-11.0 + 1.1 * (i % 20), 1.05 + 1.05 * (i // 20)))
        w.create_fixture(body, b2hip.box_shape(0.5, 0.5), density=1.0, friction=0.3)
        w.boxes.append(body)
    return w


def test_resting_world_switches_buffers_then_an_edit_compacts(monkeypatch):
    """400 resting boxes: most steps destroy nothing and the fused form still leaves the survivors - all of them - in the other
    half. Then bodies are destroyed between steps: applyEditOps runs k_compact_contacts on whichever half is live, and the
    fused form goes on behind it."""
    a, b = pair(lambda: tray(400), monkeypatch, 8)
    quiet = 0
    for s in range(30):
        a.step()
        b.step()
        stop(a, b, "step %d" % s)
        quiet += 1 if a.counters()["destroyed_contacts"] == 0 and s > 0 else 0
    before = fused(a)
    assert before == 29 and quiet > 0, (before, quiet)
    for s in range(3):
        for w in (a, b):
            for i in range(7 + s, 400, 41):
                w.destroy_body(w.boxes[i])
        for k in range(4):
            a.step()
            b.step()
            stop(a, b, "round %d, step %d after the bodies were destroyed" % (s, k))
    assert a.contact_count == b.contact_count and a.contact_count > 8 * 64
    assert fused(a) == before + 12 and fused(b) == 0
    a.close()
    b.close()


def test_whole_chunks_die(monkeypatch):
    """Settled boxes are moved apart with SetTransform: first every second row (the contacts of whole runs of the array die
    in one narrow phase, chunks of 8 among them), then all of them (every chunk is empty)."""
    a, b = pair(lambda: tray(400), monkeypatch, 8)
    L = _lib()
    a.step(20)
    b.step(20)
    stop(a, b, "settled")
    n0 = a.contact_count
    assert n0 > 8 * 64
    for rnd, rows in enumerate((range(1, 20, 2), range(0, 20))):
        at = fused(a)
        for w in (a, b):
            for r in rows:
                for c in range(20):
                    assert L.b2hip_set_transform(_ptr(w), w.boxes[20 * r + c], C.c_float(100.0 + 3.0 * c), C.c_float(100.0 + 3.0 * r + 70.0 * rnd), C.c_float(0.0)) == 0
        a.step()
        b.step()
        stop(a, b, "round %d: the step that destroys" % rnd)
        assert fused(a) == at + 1, "the step that destroyed the contacts did not take the fused form"
        for k in range(3):
            a.step()
            b.step()
            stop(a, b, "round %d, step %d after" % (rnd, k))
    print("contacts: %d settled, %d at the end" % (n0, a.contact_count))
    assert a.contact_count < n0 // 4
    a.close()
    b.close()


def test_toi_candidates_keep_the_old_path(amd, monkeypatch):
    """A pyramid of 30 rows with continuous physics. The boxes start a little above the static ground: for a few steps no TOI
    candidate is alive and the fused form runs. From the pair update that creates the bottom row's contacts with the ground -
    candidates, and they never leave - the deaths of candidates would be replayed by the contacts' old indices: every narrow
    phase after it takes the old path."""
    a, b = pair(lambda: amd.world(bh.PYRAMID, 30, 1, flags=CCD), monkeypatch)
    took = []
    for s in range(60):
        at = fused(a)
        a.step(1)
        b.step(1)
        took.append(fused(a) - at)
        stop(a, b, "step %d" % s)
    print("pyramid 30, continuous: fused form in steps", [s for s in range(60) if took[s]])
    first_old = took.index(0, 1)  # (step 0 comes before the world's first read-back)
    assert took[0] == 0 and sum(took[first_old:]) == 0 and 60 - first_old >= 40, took
    assert fused(b) == 0
    a.close()
    b.close()


def test_snapshot_round_trip(amd, monkeypatch):
    """Saved behind a fused narrow phase (whichever half is live then), loaded, stepped on: the loaded world, the original and
    the world that never fused stay equal. The loaded world's first narrow phase comes before its first read-back."""
    a, b = pair(lambda: amd.world(bh.TUMBLER, p0=40, flags=PLAIN), monkeypatch)
    a.step(50)
    b.step(50)
    stop(a, b, "step 50")
    assert fused(a) == 49
    monkeypatch.setenv("B2HIP_COLLIDE_SPLIT", "1")
    c = b2hip.World.from_snapshot(b2hip.World.borrow(a.device_world()).save_snapshot())
    monkeypatch.delenv("B2HIP_COLLIDE_SPLIT", raising=False)
    for s in range(20):
        a.step(1)
        b.step(1)
        c.step(1.0 / 60.0, a.vel_iters, a.pos_iters)
        assert hashes(c) == hashes(a), "the loaded world parts from the original at step %d after the snapshot" % s
        stop(a, b, "step %d after the snapshot" % s)
    assert fused(c) == 19 and fused(a) == 69 and fused(b) == 0
    a.close()
    b.close()
    c.close()
