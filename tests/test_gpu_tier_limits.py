"""The reference-order solver tier ON its lines: k_island_classify -> k_island_assign -> k_island_dfs -> k_solve_small<256 | 1024, JOINTS>.

Every bit-exact guarantee of the project rests on that tier, and the tier is four constants (b2d_world.h: weight 128 / 512, 64
joints, 256 / 1 024 lanes) with three pieces of rule arithmetic on top (tier rule, chunk rule, LDS sizing by LANES; restated in
tests/tier_worlds.py). The scenes of the other GPU tests have whatever island sizes they happen to have; here the worlds of
tests/tier_worlds.py - planks with bridges, one plank, pendulum chains; tests/test_tier_worlds_cpu.py holds them to their
sizes on the oracle - stand an island on each line, one short of it and one over it, and take one across it during a run.

Every world is built twice with the same calls (tier_worlds.Lockstep), on libb2hip.so and on the oracle's ABI shim. After every
step, BEFORE anything is compared, the device's counters (small_islands, large_islands, free_islands, small_island_bodies,
small_island_contacts, solver_chunks, islands) are held to what the documented rules make of (1) the census the case pins for
that step and (2) the census read from the oracle's island labels and touching contacts: a case cannot pass in another tier
than it names (TierAssertion; the two tests at the end show that it bites). Then bits:

    small side, and everything under B2HIP_FORCE_LARGE=2   bitwise against the plain oracle: body states and the whole contact
                                                          records (ids, flags, manifolds, warm-start impulses), every step
    one over a line, default mode                          the oracle replays the device's plan (tests/solve_order_ref.py,
                                                          joints by id): body words and contact count every step, hook
                                                          errors [0, 0], contact records at the end; in (b) the integers
                                                          (body flags, contact set, touching bits, point counts, islands)
                                                          also against an unhooked oracle (PLAIN_INTEGERS)

No step is left out, there is no tolerance. The cases, per line:
    (a) w = 127, 128 at the default tier and 511, 512 with B2HIP_SMALL_MAX_W=512, each as one plank (bodies = contacts, a chain of
        w dependency levels), bridged planks (contacts > bodies) and a plank with welded riders (bodies > contacts; the JOINTS
        kernel): resting, falling asleep, woken by a push on one box. large_islands == 0 throughout.
    (b) w = 129 and 513 (widened): large_islands == 1, small_islands == 0; replayed, and in exact-order mode.
    (c) chains of 63 and 64 joints small; 65 joints one large island without a contact row; a planks island of w = 128 with 64
        distance joints (the 256-lane JOINTS kernel full on both lines) and with 65.
    (d) chunk packing: ~40 islands of weights 1 .. 128 by seed, 12 of 1 .. 512 widened (1 024 lanes), 600 single boxes (chunks of
        255 islands: nI against LANES), a largest island of 129 widened (chunkW = 895).
    (e) 126 -> 127 -> 128 -> 129 -> 130 by boxes landing on the last plank, split into small islands by destroying two ties, one
        again by renewing them, two more boxes, split again: tiers change twice in each direction; ties are bridging boxes
        (plain colours) or distance joints (the jointed large side).
"""
import ctypes as C

import numpy as np
import pytest

import b2harness as bh
import b2hip
import plan_ref as pr
import solve_order_ref as so
import tier_worlds as tw
from test_gpu_edge_cases import same
from test_gpu_large_plan import set_env
from test_gpu_solve_replay import capture

pytestmark = pytest.mark.gpu

COUNTED = ("islands", "free_islands", "small_islands", "large_islands", "small_island_bodies", "small_island_contacts")


# What of a contact record does not depend on the order of the sweep. The manifold type and the feature ids do: a bridging box
# rests on 0.15 of a plank, and which of the two faces is the reference face flips with the last bits of the positions - the
# oracle in a greedy colour order against the oracle in reference order differs in exactly these two fields (eight steps of the
# w = 129 case), so they are compared against the replay only.
PLAIN_INTEGERS = ("fixture_a", "fixture_b", "body_a", "body_b", "flags", "point_count")


class TierAssertion(AssertionError):
    """The device's counters are not what the tier rule and the chunk rule make of the step's islands."""


@pytest.fixture(scope="module")
def libs(built_libs):
    if not bh.have_amd():
        pytest.fail("libb2hip.so missing (no CPU fallback)")
    return b2hip.lib(), b2hip.load(bh.ORACLE_LIB, optional_ok=True)


def misses(ctr, want):
    out = ["%s %d, the rules say %d" % (k, ctr[k], want[k]) for k in COUNTED if ctr[k] != want[k]]
    lo, hi = want["solver_chunks"]
    if not lo <= ctr["solver_chunks"] <= hi:
        out.append("solver_chunks %d, the rules say %d .. %d (windows of %s)" % (ctr["solver_chunks"], lo, hi, want.get("chunk_width")))
    return out


def hold(ctr, censuses, case, step, source):
    """The counters fit one of the censuses, or TierAssertion."""
    found = [misses(ctr, tw.expected_counters(c, case.small_max_w, case.force_large)) for c in censuses]
    if all(found):
        raise TierAssertion("%s, step %d: the counters do not fit the islands %s: %s" % (case, step, source, "; or ".join(", ".join(f) for f in found)))


def sorted_words(c):
    """A contact list as raw words, sorted by its fixture ids (an empty list too)."""
    order = np.lexsort((c["fixture_b"], c["fixture_a"]))
    return np.ascontiguousarray(c[order]).view(np.uint32).reshape(len(c), c.dtype.itemsize // 4)


def states_words(w, dead):
    s = w.body_states().view(np.uint32).reshape(-1, 10)
    if dead:
        keep = np.ones(len(s), bool)
        keep[dead] = False  # (destroyed bodies: their ids stay, what their rows hold is not defined)
        s = s[keep]
    return s


def run_case(libs, monkeypatch, case, replay=False, env=None, plain_integers=False):
    """The case on the device and the oracle in lockstep; returns (counters per step, solvers of the large-island plans seen)."""
    set_env(monkeypatch, case.env if env is None else env)
    L, O = libs
    dev = b2hip.World(library=L, allow_sleep=case.sleep)
    set_env(monkeypatch, {})
    orc = b2hip.World(library=O, allow_sleep=case.sleep)
    plain = b2hip.World(library=O, allow_sleep=case.sleep) if plain_integers else None
    worlds = tw.Lockstep(*[w for w in (dev, orc, plain) if w is not None])
    log, solvers = [], set()
    try:
        state = case.build(worlds)
        for step in range(case.steps):
            what = "%s, step %d" % (case, step)
            if case.script:
                case.script(step, worlds, state)
            dev.step()
            if replay:
                got = capture(L, dev.p)
                if got is None:  # no large island: an empty table
                    entries, large = np.zeros(0, so.ORDER_DTYPE), np.zeros(dev.body_count, np.uint8)
                else:
                    entries, large = so.solve_order(*got)
                    solvers.add(got[0].numbers["solver"])
                entries, large = np.ascontiguousarray(entries, so.ORDER_DTYPE), np.ascontiguousarray(large, np.uint8)
                O.b2o_shim_set_solve_order(orc.p, len(entries), entries.ctypes.data_as(C.c_void_p), len(large), large.ctypes.data_as(C.c_void_p), 1)
                if plain is not None:
                    plain.step()
            orc.step()
            # ---- where it went, before any comparison
            ctr = dev.counters()
            census = tw.census(orc, state.joint_bodies.values())
            allowed = case.pins(step, state)
            if allowed is not None:
                hold(ctr, allowed, case, step, "the case names")
                assert census in allowed, "%s: the oracle's islands are %s, the case allows %s" % (what, census[:6], [a[:6] for a in allowed])
            hold(ctr, (census,), case, step, "of the oracle")
            log.append(ctr)
            # ---- bits
            if not replay:
                same(dev, orc, what, skip=tuple(state.dead))
                assert np.array_equal(dev.contacts().view(np.uint32), orc.contacts().view(np.uint32)), "%s: contact records differ" % what
                continue
            errors = np.zeros(2, np.int32)
            O.b2o_shim_get_solve_order_errors(orc.p, errors.ctypes.data_as(C.c_void_p))
            assert errors.tolist() == [0, 0], "%s: the hook could not follow the plan: %s" % (what, errors.tolist())
            d, o = states_words(dev, state.dead), states_words(orc, state.dead)
            bad = np.flatnonzero((d != o).any(axis=1))
            assert len(bad) == 0, "%s: %d bodies differ from the replay of the device's plan; the first (row %d): device %s, replay %s" % (
                what, len(bad), bad[0], d[bad[0]].view(np.float32)[:8].tolist(), o[bad[0]].view(np.float32)[:8].tolist())
            assert dev.contact_count == orc.contact_count, "%s: %d contacts on the device, %d in the replay" % (what, dev.contact_count, orc.contact_count)
            # integers against the unhooked oracle, while the case pins ONE census for the step (the three worlds then solve the
            # same islands; once a pile may fall asleep again the step it does so depends on the floats, which are the order's)
            if plain is None or allowed is None or len(allowed) != 1:
                continue
            p = states_words(plain, state.dead)
            assert np.array_equal(d[:, 8] & 0x7f, p[:, 8] & 0x7f), "%s: body flags differ from the plain oracle's" % what
            dc, pc = dev.contacts(), plain.contacts()
            assert len(dc) == len(pc), "%s: %d contacts, the plain oracle has %d" % (what, len(dc), len(pc))
            for f in PLAIN_INTEGERS:
                assert np.array_equal(dc[f], pc[f]), "%s: contact %s differs from the plain oracle's" % (what, f)
            assert tw.census(plain, state.joint_bodies.values()) == census, "%s: the plain oracle's islands differ" % what
        if replay:
            d, o = sorted_words(dev.contacts()), sorted_words(orc.contacts())
            assert d.shape == o.shape and np.array_equal(d, o), "%s: the contact records differ from the replay's at the end" % case
    finally:
        for w in worlds.worlds:
            w.close()
        set_env(monkeypatch, {})
    print("%s: large islands in %d of %d steps, most chunks %d, solvers %s" % (
        case, sum(c["large_islands"] > 0 for c in log), len(log), max(c["solver_chunks"] for c in log), sorted(solvers)))
    return log, solvers


def solved(log):
    return [c for c in log if c["islands"] > 0]


# ---- (a) on the line, small side ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tw.SMALL_SIDE, ids=repr)
def test_on_the_line_small_side(libs, monkeypatch, case):
    log, _ = run_case(libs, monkeypatch, case)
    assert all(c["large_islands"] == 0 for c in log)
    awake = solved(log)
    assert all(c["small_islands"] == 1 and c["solver_chunks"] == 1 for c in awake)
    # asleep in between, and back after the push
    assert 2 * tw.ASLEEP_AT <= len(awake) < len(log) and log[tw.WAKE_AT - 1]["islands"] == 0 and log[tw.WAKE_AT]["small_islands"] == 1


# ---- (b) one over the line ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tw.OVER, ids=repr)
def test_one_over_the_line_replayed(libs, monkeypatch, case):
    log, solvers = run_case(libs, monkeypatch, case, replay=True, plain_integers=True)
    awake = solved(log)
    assert all(c["large_islands"] == 1 and c["small_islands"] == 0 and c["solver_chunks"] == 0 for c in awake)
    assert 2 * tw.ASLEEP_AT <= len(awake) < len(log) and log[tw.WAKE_AT]["large_islands"] == 1
    assert solvers and pr.SOLVER_EXACT not in solvers, solvers


@pytest.mark.parametrize("case", [c.exact() for c in tw.OVER], ids=repr)
def test_one_over_the_line_in_exact_order(libs, monkeypatch, case):
    log, _ = run_case(libs, monkeypatch, case)
    assert all(c["large_islands"] == 1 for c in solved(log)) and len(solved(log)) >= 2 * tw.ASLEEP_AT


# ---- (c) the joint line ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tw.CHAINS_SMALL + [tw.RODS_64], ids=repr)
def test_joint_line_small_side(libs, monkeypatch, case):
    log, _ = run_case(libs, monkeypatch, case)
    assert all(c["large_islands"] == 0 for c in log)
    assert all(c["small_islands"] == 1 and c["solver_chunks"] == 1 for c in solved(log)) and len(solved(log)) >= 2 * tw.ASLEEP_AT


@pytest.mark.parametrize("case", [tw.CHAIN_65, tw.RODS_65], ids=repr)
def test_one_joint_over_replayed(libs, monkeypatch, case):
    log, solvers = run_case(libs, monkeypatch, case, replay=True)
    awake = solved(log)
    assert all(c["large_islands"] == 1 and c["small_islands"] == 0 for c in awake) and len(awake) >= 2 * tw.ASLEEP_AT
    if case is tw.CHAIN_65:
        assert all(c["large_island_contacts"] == 0 and c["large_island_bodies"] == 65 for c in log)  # not one contact row
    assert solvers and pr.SOLVER_EXACT not in solvers, solvers


@pytest.mark.parametrize("case", [tw.CHAIN_65.exact(), tw.RODS_65.exact()], ids=repr)
def test_one_joint_over_in_exact_order(libs, monkeypatch, case):
    log, _ = run_case(libs, monkeypatch, case)
    assert all(c["large_islands"] == 1 for c in solved(log)) and len(solved(log)) >= 2 * tw.ASLEEP_AT


# ---- (d) chunk packing -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tw.CHUNKS, ids=repr)
def test_chunk_packing(libs, monkeypatch, case):
    log, _ = run_case(libs, monkeypatch, case)
    assert all(c["large_islands"] == 0 for c in log) and len(solved(log)) == tw.ASLEEP_AT
    first = log[0]
    if "600" in case.name:
        # windows of 255 islands of weight 1: three chunks, the first two with 255 islands on 256 lanes
        assert first["small_islands"] == 600 and first["solver_chunks"] in (2, 3)
    else:  # (2 159 rows in windows of 895 where the largest island is 129)
        assert first["solver_chunks"] > 1, first


# ---- (e) across the line during a run ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tw.CROSSINGS, ids=repr)
def test_across_the_line_both_ways(libs, monkeypatch, case):
    log, solvers = run_case(libs, monkeypatch, case, replay=True)
    without, with_large, up, down = tw.tier_changes([c["large_islands"] for c in log])
    print("%s: %d steps without a large island, %d with one, %d changes small -> large, %d large -> small" % (case, without, with_large, up, down))
    assert without > 40 and with_large > 40 and up >= 2 and down >= 2, (without, with_large, up, down)
    assert max(c["free_islands"] for c in log) == 2  # (boxes in the air)
    if "joints" in case.name:
        assert pr.SOLVER_SWEEP in solvers, "the jointed large island never took k_blocks_sweep: %s" % sorted(solvers)


# ---- the tier assertions bite ------------------------------------------------------------------------------------------------

def test_an_island_on_the_line_in_a_tier_one_narrower_is_noticed(libs, monkeypatch):
    case = tw.line_case(128, "one plank")
    with pytest.raises(TierAssertion, match="large_islands 1, the rules say 0"):
        run_case(libs, monkeypatch, case, env={"B2HIP_SMALL_MAX_W": "127"})


def test_a_65th_joint_is_noticed(libs, monkeypatch):
    as_64 = tw.Case("65 joints held to the 64-joint case", tw.CHAIN_65.build, 3, lambda step, state: ([(64, 0, 64)],))
    with pytest.raises(TierAssertion, match="large_islands 1, the rules say 0"):
        run_case(libs, monkeypatch, as_64)
