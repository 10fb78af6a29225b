"""Which way the host ran b2World::SolveTOI, and which rungs of its fall-back ladder it took (docs/TOI.md, "host flow";
box2d-mt_amd/csrc/b2hip_host_toi.h), read from the statistics of b2hip_debug_read 25 - ten counters since the world was
created: the phase run as chains queued without the first pass's census [0] / after it [1], as components queued without
the census [2] / after it [3], by the serial loop straight from the census [4]; then the rungs: redo behind a late pair
sort [5], chains once more with the hash grid [6], serial fall-back [7], re-run after a contact-array overflow [8],
PreSolve re-run [9].

The grid retry. The candidate the rung was first measured on, a settled pyramid, does NOT reach it at a test's size: PYRAMID
with 10, 20, 30, 40, 60, 80 and 99 rows (56 to 4 951 boxes), continuous physics on, 400 steps each - the counter stays 0 in
all of them (the chains run in ~370 of the 400 steps, never with a proxy leaving its fat AABB while the grid hint is out).
A rain of 1 500 bodies reaches it twice in 100 steps - bodies that come to rest one after the other, with pauses of more than
16 steps between two moved proxies - so that is the scene of the test.
"""
import ctypes as C

import pytest

import b2harness as bh
import b2hip
from spatial_util import SpatialRanks

pytestmark = pytest.mark.gpu

CCD = bh.F_CONTINUOUS | bh.F_SLEEP | bh.F_WARM
CHAINS_QUEUED, CHAINS_CENSUS, COMPONENTS_QUEUED, COMPONENTS_CENSUS, SERIAL_DIRECT = 0, 1, 2, 3, 4
REDO_LATE_PAIRS, GRID_RETRY, SERIAL_FALLBACK, OVERFLOW_RERUN, PRESOLVE_RERUN = 5, 6, 7, 8, 9


def toi_stats(w):
    L = b2hip.lib()
    L.b2hip_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out = (C.c_longlong * 10)()
    assert L.b2hip_debug_read(C.c_void_p(w.device_world()), 25, 0, 10, out) == 0
    return list(out)


def fallbacks_reported(w):
    ctr = b2hip.Counters()
    assert b2hip.lib().b2hip_get_counters(C.c_void_p(w.device_world()), C.byref(ctr)) == 0
    return ctr.toi_serial_fallbacks


def run(amd, monkeypatch, scene, p0, p1, seed, steps, env=None, hashes=False):
    """-> (the statistics after every step, per-step (state hash, contact count) if asked for, toi_serial_fallbacks at the end)"""
    for k in ("B2HIP_TOI_NO_SPEC_DOMAINS", "B2HIP_TOI_SERIAL", "B2HIP_DEBUG_ASSUME_FRESH_GRID", "B2HIP_FORCE_LARGE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)  # (read once, when the world is made)
    w = amd.world(scene, p0, p1, 0.0, 0.0, seed=seed, flags=CCD)
    series, states = [], []
    for _ in range(steps):
        w.step(1)
        series.append(toi_stats(w))
        if hashes:
            states.append((bh.fnv1a64(w.bodies()), w.contact_count))
    reported = fallbacks_reported(w)
    w.close()
    return series, states, reported


def first_step(series, k):
    return next((i for i, s in enumerate(series) if s[k] > 0), None)


FIELD = (bh.FIELD, 2500, 300, 11, 25)  # the world of test_ccd_components_run_side_by_side_and_stay_bit_exact


def test_components_run_after_the_census_first_and_without_it_from_then_on(amd, monkeypatch):
    series, _, _ = run(amd, monkeypatch, *FIELD)
    last = series[-1]
    print("FIELD 2500/300:", last)
    assert last[COMPONENTS_CENSUS] > 0 and last[COMPONENTS_QUEUED] > 0
    census, queued = first_step(series, COMPONENTS_CENSUS), first_step(series, COMPONENTS_QUEUED)
    assert census < queued, "the census form must come first: it leaves the hints the queued form is sized from"
    # from some step on: every step behind the first queued one is a queued one (bullets are in flight in all 25 steps)
    assert [s[COMPONENTS_QUEUED] for s in series[queued:]] == list(range(1, len(series) - queued + 1))
    assert last[SERIAL_DIRECT] == 0


def test_components_always_look_at_the_census_when_told_to(amd, monkeypatch):
    series, _, _ = run(amd, monkeypatch, *FIELD, env={"B2HIP_TOI_NO_SPEC_DOMAINS": "1"})
    print("FIELD 2500/300, census first:", series[-1])
    assert series[-1][COMPONENTS_QUEUED] == 0
    assert series[-1][COMPONENTS_CENSUS] > 0


def test_serial_only_moves_the_serial_counter_alone(amd, monkeypatch):
    series, _, _ = run(amd, monkeypatch, *FIELD, env={"B2HIP_TOI_SERIAL": "1"})
    print("FIELD 2500/300, serial only:", series[-1])
    assert series[-1][SERIAL_DIRECT] > 0
    assert [v for k, v in enumerate(series[-1]) if k != SERIAL_DIRECT] == [0] * 9


def test_every_wrong_guess_of_the_queued_components_is_a_serial_fall_back(amd, monkeypatch):
    """B2HIP_DEBUG_ASSUME_FRESH_GRID=1 makes every step of the queued component path a wrong guess. Step by step: the
    fall-back counter moves exactly when the queued-components counter does, from the first such step on - so the fall-backs
    from there on equal the queued component steps. (The world's very first step falls back once more, with the switch and
    without it: its chains, queued before anything is known of the world, meet the bullets. Measured: 24 fall-backs for 23
    queued component steps with the switch, 1 without.)"""
    series, _, reported = run(amd, monkeypatch, *FIELD, env={"B2HIP_DEBUG_ASSUME_FRESH_GRID": "1"})
    plain, _, _ = run(amd, monkeypatch, *FIELD)
    print("FIELD 2500/300, every guess wrong:", series[-1], "plain:", plain[-1])
    queued = first_step(series, COMPONENTS_QUEUED)
    assert queued is not None and series[-1][COMPONENTS_QUEUED] > 0
    before = series[queued - 1][SERIAL_FALLBACK] if queued > 0 else 0
    for s in series[queued:]:
        assert s[SERIAL_FALLBACK] - before == s[COMPONENTS_QUEUED]
    assert before == plain[queued - 1][SERIAL_FALLBACK], "the fall-backs before the first queued step are not the switch's"
    assert plain[-1][SERIAL_FALLBACK] == before, "the plain world's queued components fell back"
    assert reported == series[-1][SERIAL_FALLBACK]


@pytest.fixture(scope="module")
def rain(amd):
    """RAIN 1500 seed 7, 100 steps, and the same world through the serial loop only (computed once, shared, left unchanged)"""
    mp = pytest.MonkeyPatch()
    try:
        par = run(amd, mp, bh.RAIN, 1500, 0, 7, 100, hashes=True)
        ser = run(amd, mp, bh.RAIN, 1500, 0, 7, 100, env={"B2HIP_TOI_SERIAL": "1"}, hashes=True)
    finally:
        mp.undo()
    return par, ser


def test_chains_run_and_both_counters_report_the_same_fall_backs(rain):
    (series, _, reported), _ = rain
    print("RAIN 1500:", series[-1])
    assert series[-1][CHAINS_QUEUED] > 0 and series[-1][CHAINS_CENSUS] > 0
    assert reported == series[-1][SERIAL_FALLBACK]


def test_grid_retry_is_taken_and_gives_the_serial_loops_states(rain):
    (series, states, _), (serial_series, serial_states, _) = rain
    print("RAIN 1500: grid retries", series[-1][GRID_RETRY], "first at step", first_step(series, GRID_RETRY))
    assert series[-1][GRID_RETRY] > 0, "no chain moved a proxy out of its fat AABB while the grid hint was out: the test is vacuous"
    assert serial_series[-1][GRID_RETRY] == 0 and serial_series[-1][SERIAL_DIRECT] > 0
    first = next((i for i, (x, y) in enumerate(zip(states, serial_states)) if x != y), None)
    assert first is None, "the chains (with their grid retry) and the serial loop diverge at step %s" % first


def test_a_sharded_ranks_ladder_counts_too(amd, monkeypatch):
    """Two ranks in one process (tests/spatial_util.py) on the dense bullets of test_gpu_spatial.py: the ranks settle their
    phases through the same ladder (spAfterToi), so their rungs are counted like the unsharded world's."""
    for k in ("B2HIP_TOI_NO_SPEC_DOMAINS", "B2HIP_TOI_SERIAL", "B2HIP_DEBUG_ASSUME_FRESH_GRID", "B2HIP_FORCE_LARGE", "B2HIP_SHARD_FULL_ROWS"):
        monkeypatch.delenv(k, raising=False)
    kw = dict(p0=60, p1=6, f0=0.0, f1=0.0, seed=3, flags=CCD)
    ref = amd.world(bh.BULLETS, **kw)
    ws = [amd.world(bh.BULLETS, **kw) for _ in range(2)]
    sr = SpatialRanks(b2hip.lib(), [(w, w.device_world()) for w in ws])
    for _ in range(120):
        ref.step(1)
        sr.step()
    one, ranks = toi_stats(ref), [toi_stats(w) for w in ws]
    for w in ws:
        assert w.contact_count == ref.contact_count
        w.close()
    ref.close()
    taken = sum(r[SERIAL_FALLBACK] + r[GRID_RETRY] for r in ranks)
    print("BULLETS 60/6: unsharded", one, "ranks", ranks, "- serial fall-backs + grid retries over the ranks:", taken)
    assert all(r[CHAINS_QUEUED] == 0 and r[COMPONENTS_QUEUED] == 0 for r in ranks), "a sharded rank always looks at its census"
    if one[SERIAL_FALLBACK] + one[GRID_RETRY] > 0:
        assert taken > 0
