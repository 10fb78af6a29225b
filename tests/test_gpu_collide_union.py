"""GPU: the narrow phase that unites the contacts it stores (box2d-mt_amd/csrc/b2d_kernels_collide.h: k_collide<0, false, true,
true>; B2HIP_COLLIDE_UNION, default on) against a world created under B2HIP_COLLIDE_UNION=0, whose narrow phase stores the
compacted array as before and whose island build runs k_island_union over the contacts.

The tail of the narrow phase counts the degrees, hands out the places in the adjacency segments, walks the union-find trees
and voids the colours k_color_check's first loop would void. None of it may change a bit: at every stop b2hip_debug_hash 0 to 3
(bodies, contacts, fat AABBs, islands) of the two worlds are equal, exactly. b2hip_debug_read 31 counts the island builds that
ran no union pass over the contacts: in the first world it equals the count of fused narrow phases (b2hip_debug_read 24), in
the second it is 0. B2HIP_COLLIDE_SPLIT=1 throughout, so that worlds this small take the form at all."""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
import plan_ref as pr
from test_gpu_collide_compact import fused, tray
from test_gpu_keyset import _lib, _ptr
from test_gpu_large_plan import capture, counters
from test_gpu_large_plan import _lib as plan_lib

pytestmark = pytest.mark.gpu

PLAIN = bh.F_SLEEP | bh.F_WARM
PLAN_NAMES = ("degree", "row_set", "root", "colour_clash", "body_colour_mask")


def skipped(w):
    """island builds of this world that ran no union pass over the contacts"""
    out = C.c_longlong()
    assert _lib().b2hip_debug_read(_ptr(w), 31, 0, 1, C.byref(out)) == 0
    return out.value


def hashes4(w):
    L, out = _lib(), []
    for which in (0, 1, 2, 3):
        h = C.c_uint64()
        assert L.b2hip_debug_hash(_ptr(w), which, C.byref(h)) == 0
        out.append(h.value)
    return out


def labels(w):
    L = plan_lib()
    ptr = C.c_void_p(_ptr(w))
    nb = L.b2hip_body_count(ptr)
    out = np.zeros(nb, np.int32)
    assert L.b2hip_get_island_labels(ptr, nb, out.ctypes.data_as(C.c_void_p)) == nb
    return out


def stop(a, b, what):
    assert hashes4(a) == hashes4(b), what


def pair(make, monkeypatch, chunk=None, env=None):
    """(a world whose narrow phase may unite its contacts, the same world under B2HIP_COLLIDE_UNION=0)"""
    env = dict(env or {}, B2HIP_COLLIDE_SPLIT="1")
    if chunk:
        env["B2HIP_TEST_COLLIDE_CHUNK"] = str(chunk)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("B2HIP_COLLIDE_UNION", raising=False)
    a = make()
    monkeypatch.setenv("B2HIP_COLLIDE_UNION", "0")
    b = make()
    monkeypatch.delenv("B2HIP_COLLIDE_UNION", raising=False)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return a, b


def counted(a, b, least):
    """the first world's island builds skipped the union pass behind every fused narrow phase, the second's never did"""
    assert fused(a) >= least and skipped(a) == fused(a), (fused(a), skipped(a))
    assert fused(b) == fused(a) and skipped(b) == 0, (fused(b), skipped(b))


@pytest.mark.parametrize("chunk", [256, 32, 2])
def test_tumbler_churn(amd, monkeypatch, chunk):
    """Tumbler 40 x 40 (1 600 boxes, continuous physics off), 150 steps: one large island with a hub (the container) and a
    joint, loose boxes, contacts born and dying every step. With 2 contacts per workgroup most workgroups hold no solid
    contact at all and a body's contacts lie in many workgroups."""
    a, b = pair(lambda: amd.world(bh.TUMBLER, p0=40, flags=PLAIN), monkeypatch, chunk)
    for k in range(15):
        a.step(10)
        b.step(10)
        stop(a, b, "after %d steps" % (10 * (k + 1)))
    # (every narrow phase but the first, which comes before the world's first read-back)
    counted(a, b, 149)
    a.close()
    b.close()


def thick_ground(w, half):
    """a static floor whose contacts are no TOI candidates (a candidate alive keeps the narrow phase on its old path:
    tests/test_gpu_collide_compact.py, test_toi_candidates_keep_the_old_path)"""
    g = w.create_body(b2hip.STATIC)
    w.create_fixture(g, b2hip.box_shape(half, 0.5), thick=True)
    return g


def piles(count, height):
    """`count` piles of `height` boxes on a thick floor, 2 m apart. Pile p leaves a gap under its box p % (height + 1): the
    boxes above it are in flight for the first steps (islands of one body, no contact) and land one after the other."""
    w = b2hip.World(gravity=(0.0, -10.0))
    thick_ground(w, count + 10.0)
    for p in range(count):
        y = 0.5
        for k in range(height):
            y += 0.01 if k != p % (height + 1) else 0.3 * (1 + p % 7)
            body = w.create_body(b2hip.DYNAMIC, position=(-count + 2.0 * p + 0.05 * (k % 3), y + 0.2))
            w.create_fixture(body, b2hip.box_shape(0.4, 0.2), density=1.0 + 0.25 * (k % 4), friction=0.4)
            y += 0.4
    return w


def linked(count):
    """`count` boxes resting 2 m apart on a thick floor: no contact joins two of them. Distance joints tie them in chains of
    1, 2, 3, ... boxes, a weld joint ties the first of every other chain to a box that sits on it."""
    w = b2hip.World(gravity=(0.0, -10.0))
    thick_ground(w, count + 10.0)
    boxes = []
    for i in range(count):
        body = w.create_body(b2hip.DYNAMIC, position=(-count + 2.0 * i, 1.0))
        w.create_fixture(body, b2hip.box_shape(0.5, 0.5), density=1.0, friction=0.5)
        boxes.append(body)
    w.chains, w.ties, first, length = [], [], 0, 1
    while first + length <= count:
        for i in range(first, first + length - 1):
            w.create_distance_joint(boxes[i], boxes[i + 1], length=2.0)
            w.ties.append((boxes[i], boxes[i + 1]))
        if (length & 1) == 0:
            top = w.create_body(b2hip.DYNAMIC, position=(-count + 2.0 * first, 1.75))
            w.create_fixture(top, b2hip.box_shape(0.25, 0.25), density=1.0, friction=0.5)
            w.create_weld_joint(boxes[first], top, anchor_a=(0.0, 0.75), anchor_b=(0.0, 0.0), collide_connected=True)
        w.chains.append(boxes[first:first + length])
        first += length
        length += 1
    return w


def test_many_components(amd, monkeypatch):
    """Islands of every size. bh.PILES - 2 000 piles of 5, a shape record per body, a plain static floor - stays equal to
    its twin, whichever narrow phase its records and the floor's TOI candidates leave it. 800 piles of 5 on a thick floor
    take the new form in every step: singletons in flight (ROOT_FREE), piles that grow as boxes land, all of them in the
    reference-order tier."""
    a, b = pair(lambda: amd.world(bh.PILES, p0=2000, p1=5, seed=7, flags=PLAIN), monkeypatch)
    for k in range(6):
        a.step(10)
        b.step(10)
        stop(a, b, "bh.PILES after %d steps" % (10 * (k + 1)))
        assert np.array_equal(labels(a), labels(b)), "bh.PILES: island labels after %d steps" % (10 * (k + 1))
    counted(a, b, 0)
    a.close()
    b.close()
    a, b = pair(lambda: piles(800, 5), monkeypatch)
    sizes = set()
    for k in range(12):
        for s in range(5):
            a.step()
            b.step()
        stop(a, b, "800 piles after %d steps" % (5 * (k + 1)))
        la = a.island_labels()
        assert np.array_equal(la, b.island_labels()), "800 piles: island labels after %d steps" % (5 * (k + 1))
        sizes |= set(np.bincount(la[la >= 0]).tolist())
        assert a.counters()["large_islands"] == 0
    counted(a, b, 59)
    assert {1, 2, 3, 4, 5} <= sizes, "island sizes seen: %s" % sorted(sizes)
    a.close()
    b.close()


def test_joints_connect_what_no_contact_connects(amd, monkeypatch):
    """The machines buried under 600 boxes (tests/test_gpu_large_plan.py) stay equal to their twin. Then a world in which
    only joints join bodies and every narrow phase takes the new form: chains of 1 to 30 boxes that touch nothing but the
    floor - their islands come out of the launch that walks the joints only."""
    a, b = pair(lambda: amd.world(bh.MACHINES, p0=600, p1=6, seed=3, flags=PLAIN), monkeypatch)
    for k in range(16):
        a.step(10)
        b.step(10)
        stop(a, b, "machines after %d steps" % (10 * (k + 1)))
        assert np.array_equal(labels(a), labels(b)), "machines: island labels after %d steps" % (10 * (k + 1))
    counted(a, b, 0)
    a.close()
    b.close()
    a, b = pair(lambda: linked(465), monkeypatch, 32)
    for k in range(8):  # (24 steps: the chains rest from the first step and fall asleep after 30)
        for s in range(3):
            a.step()
            b.step()
        stop(a, b, "chains after %d steps" % (3 * (k + 1)))
        la = a.island_labels()
        assert np.array_equal(la, b.island_labels()), "chains: island labels after %d steps" % (3 * (k + 1))
        contacts = a.contacts()
        solid = (contacts["flags"] & 3) == 3
        tied = set(zip(contacts["body_a"][solid].tolist(), contacts["body_b"][solid].tolist()))
        assert not any((x, y) in tied or (y, x) in tied for x, y in a.ties), "two boxes of a chain touch"
        for chain in a.chains:
            assert la[chain[0]] >= 0 and len(set(la[chain].tolist())) == 1, "a chain of %d boxes in islands %s" % (len(chain), sorted(set(la[chain].tolist())))
        assert len(set(la[c[0]] for c in a.chains)) == len(a.chains), "two chains share an island"
    counted(a, b, 23)
    a.close()
    b.close()


def test_bodies_destroyed_between_steps(monkeypatch):
    """400 resting boxes, then bodies destroyed between steps: applyEditOps compacts the contact array, the step behind it
    unites what is left, and the counter goes on counting."""
    a, b = pair(lambda: tray(400), monkeypatch, 8)
    for s in range(30):
        a.step()
        b.step()
        stop(a, b, "step %d" % s)
    before = skipped(a)
    assert before == 29 and fused(a) == 29, (before, fused(a))
    for s in range(3):
        for w in (a, b):
            for i in range(7 + s, 400, 41):
                w.destroy_body(w.boxes[i])
        for k in range(4):
            a.step()
            b.step()
            stop(a, b, "round %d, step %d after the bodies were destroyed" % (s, k))
    assert skipped(a) == before + 12
    counted(a, b, before + 12)
    a.close()
    b.close()


def test_plan_invariants(amd, monkeypatch):
    """Tumbler 60, a launch per colour: the device's plan of the large-island solve behind every one of 40 steps - degrees, rows,
    roots, colours, the colour masks of the bodies - against tests/plan_ref.py, in the world whose narrow phase counted the
    degrees, walked the trees and voided the colours."""
    monkeypatch.setenv("B2HIP_COLLIDE_SPLIT", "1")
    monkeypatch.setenv("B2HIP_SOLVER_LAUNCHES", "1")
    monkeypatch.delenv("B2HIP_COLLIDE_UNION", raising=False)
    w = amd.world(bh.TUMBLER, p0=60, flags=PLAIN)
    monkeypatch.delenv("B2HIP_COLLIDE_SPLIT", raising=False)
    monkeypatch.delenv("B2HIP_SOLVER_LAUNCHES", raising=False)
    L = plan_lib()
    ptr = C.c_void_p(w.device_world())
    checked = 0
    for s in range(40):
        w.step(1)
        got = capture(L, ptr)
        if got is None:
            continue
        plan, world = got
        found = [v for v in pr.check_plan(plan, world) if v.name in PLAN_NAMES]
        assert not found, "step %d:\n%s" % (s, pr.format_violations(found))
        checked += 1
    assert checked >= 20, "only %d of 40 steps had a large island" % checked  # (the boxes pile up against the wall first)
    assert skipped(w) == 39 and fused(w) == 39, (skipped(w), fused(w))
    w.close()


def test_run_to_run(amd, monkeypatch):
    """Two worlds under the default: the unions interleave differently, the places in the adjacency segments differ, the
    state after 100 steps does not."""
    monkeypatch.setenv("B2HIP_COLLIDE_SPLIT", "1")
    monkeypatch.delenv("B2HIP_COLLIDE_UNION", raising=False)
    a = amd.world(bh.TUMBLER, p0=40, flags=PLAIN)
    b = amd.world(bh.TUMBLER, p0=40, flags=PLAIN)
    monkeypatch.delenv("B2HIP_COLLIDE_SPLIT", raising=False)
    a.step(100)
    b.step(100)
    stop(a, b, "after 100 steps")
    assert skipped(a) == 99 and skipped(b) == 99, (skipped(a), skipped(b))
    a.close()
    b.close()
