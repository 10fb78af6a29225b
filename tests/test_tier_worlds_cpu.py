"""The worlds of tests/tier_worlds.py ARE what they say, on the oracle alone: no GPU.

tests/test_gpu_tier_limits.py stands islands on the lines of the reference-order tier (weight 128 / 512, 64 joints) and asserts
from the device's counters which tier each took. That is worth something only if the island really has the weight its builder
names, on every step of the window the GPU test runs - one contact that flickers, one box that slides off, and the case would
hold the device to another island than it thinks. Here every case of tier_worlds.ALL_CASES runs its whole window on the
oracle (libb2oracle_harness.so through the C ABI shim), and after every step the census of the islands that step solved -
island labels and touching contacts read from the oracle - must be one the case allows (tier_worlds.Case.pins).

The rules themselves (tier, free bodies, chunk width, number of chunks) are restated in tier_worlds.expected_counters from
their documentation; a few hand-made censuses pin that restatement down.
"""
import numpy as np
import pytest

import b2harness as bh
import b2hip
import tier_worlds as tw


@pytest.fixture(scope="module")
def oracle_lib(built_libs):
    return b2hip.load(bh.ORACLE_LIB, optional_ok=True)


def run_on_oracle(lib, case):
    """[(census, most solid contacts on one moving body)] per step."""
    w = b2hip.World(library=lib, allow_sleep=case.sleep)
    try:
        state = case.build(w)
        out = []
        for step in range(case.steps):
            if case.script:
                case.script(step, w, state)
            w.step()
            got = tw.census(w, state.joint_bodies.values())
            allowed = case.pins(step, state)
            assert allowed is None or got in allowed, "%s, step %d: the islands are %s, the case allows %s" % (case, step, got[:6], [a[:6] for a in allowed])
            c = w.contacts()
            solid = c[(c["flags"] & 3) == 3]
            moving = (w.body_states()["flags"] & 3) != 0
            ends = np.concatenate([solid["body_a"], solid["body_b"]])
            degree = np.bincount(ends[moving[ends]], minlength=1)
            out.append((got, int(degree.max())))
        return out, state
    finally:
        w.close()


@pytest.mark.parametrize("case", tw.ALL_CASES, ids=[c.name for c in tw.ALL_CASES])
def test_every_step_has_the_islands_the_case_names(oracle_lib, case):
    log, state = run_on_oracle(oracle_lib, case)
    pinned = sum(case.pins(step, state) is not None for step in range(case.steps))
    assert pinned >= case.steps // 20, "%s pins %d of its %d steps" % (case, pinned, case.steps)
    assert any(census for census, _ in log), "%s: no step solved an island" % case


def large_per_step(case, log):
    return [tw.expected_counters(census, case.small_max_w)["large_islands"] for census, _ in log]


@pytest.mark.parametrize("case", tw.SMALL_SIDE + [tw.RODS_64] + tw.CHAINS_SMALL + tw.CHUNKS, ids=repr)
def test_small_side_cases_stay_in_the_tier(oracle_lib, case):
    log, _ = run_on_oracle(oracle_lib, case)
    assert max(large_per_step(case, log)) == 0
    if case in tw.SMALL_SIDE:
        # asleep, woken, and the whole island is back
        solved = [bool(census) for census, _ in log]
        assert not any(solved[tw.ASLEEP_AT:tw.WAKE_AT]) and all(solved[:tw.ASLEEP_AT]) and all(solved[tw.WAKE_AT:tw.WAKE_AT + tw.ASLEEP_AT])


@pytest.mark.parametrize("case", tw.OVER + [tw.RODS_65, tw.CHAIN_65] + tw.CROSSINGS, ids=repr)
def test_large_side_cases_have_one_large_island_and_no_hub(oracle_lib, case):
    log, _ = run_on_oracle(oracle_lib, case)
    large = large_per_step(case, log)
    assert max(large) == 1 and sum(large) > 20, large
    # a body with more than HUB_DEGREE rows would bring the hub group in: these cases are about plain colours
    assert max(degree for _, degree in log) <= tw.PLANK_MAX_CONTACTS < tw.HUB_DEGREE


@pytest.mark.parametrize("case", tw.CROSSINGS, ids=repr)
def test_the_crossing_cases_cross_both_ways_twice(oracle_lib, case):
    log, _ = run_on_oracle(oracle_lib, case)
    without, with_large, up, down = tw.tier_changes(large_per_step(case, log))
    assert without > 40 and with_large > 40 and up >= 2 and down >= 2, (without, with_large, up, down)
    weights = sorted({max(i[0], i[1]) for census, _ in log for i in census[:1]})
    assert {126, 127, 128, 129, 130}.issubset(weights), weights


def test_the_line_cases_name_their_weights(oracle_lib):
    for case in tw.SMALL_SIDE + tw.OVER + [tw.RODS_64, tw.RODS_65]:
        want = int(case.name.split(",")[0].split("=")[1].split()[0])
        w = b2hip.World(library=oracle_lib)
        isl = case.build(w).islands[0]
        w.close()
        assert isl.w == want and want in (127, 128, 129, 511, 512, 513), (case, isl.expected)
        if "riders" in case.name:
            assert isl.bodies == want > isl.contacts and isl.joints == 3
        elif "one plank" in case.name:
            assert isl.bodies == isl.contacts == want
        else:
            assert isl.contacts == want > isl.bodies
    assert tw.bridged_counts(128) == [23] * 5 and sum(tw.bridged_counts(513)) + 3 * len(tw.bridged_counts(513)) - 2 == 513
    assert max(tw.bridged_counts(512)) + 3 <= tw.PLANK_MAX_CONTACTS and tw.bridged_counts(126, 6)[-1] + 2 + 6 <= tw.PLANK_MAX_CONTACTS


def test_the_rules_on_hand_made_censuses():
    ec = tw.expected_counters
    # the weight line: max(bodies, contacts), either way round
    assert ec([(128, 100, 0)])["large_islands"] == 0 and ec([(100, 128, 0)])["large_islands"] == 0
    assert ec([(129, 100, 0)])["large_islands"] == 1 and ec([(100, 129, 0)])["small_islands"] == 0
    assert ec([(100, 129, 0)], 512)["small_islands"] == 1 and ec([(513, 2, 0)], 512)["large_islands"] == 1
    # the joint line does not move with the weight line
    assert ec([(5, 0, 64)])["small_islands"] == 1 and ec([(5, 0, 65)])["large_islands"] == 1 and ec([(5, 0, 65)], 512)["large_islands"] == 1
    # a free body is neither
    e = ec([(1, 0, 0), (1, 1, 0), (1, 0, 1)])
    assert (e["free_islands"], e["small_islands"], e["large_islands"], e["islands"]) == (1, 2, 0, 3)
    # chunks: 600 boxes of weight 1 in windows of 255; a largest island of 128 halves 256 lanes, of 129 takes 1 024 lanes
    e = ec([(1, 1, 0)] * 600)
    assert (e["chunk_width"], e["chunk_lanes"], e["solver_chunks"]) == (255, 256, (2, 3))
    assert tw.chunk_width(128) == (128, 256) and tw.chunk_width(129) == (895, 1024) and tw.chunk_width(512) == (512, 1024) and tw.chunk_width(600) == (512, 1024)
    assert ec([(128, 128, 0)])["solver_chunks"] == (1, 1) and ec([(128, 128, 0), (1, 1, 0)])["solver_chunks"] == (1, 2)
    # exact-order mode: nothing is free, everything goes through the large-island solver
    e = ec([(1, 0, 0), (5, 5, 0)], force_large=2)
    assert (e["free_islands"], e["small_islands"], e["large_islands"]) == (0, 2, 2)
