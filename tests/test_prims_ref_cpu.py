"""CPU checks of tests/prims_ref.py: every reference against a naive per-element loop, colorSlot against a table written out
by hand, and the CASE TABLES of tests/test_gpu_scan.py and tests/test_gpu_wave.py - the conditions that keep those tests from
being vacuous, computed here from the inputs alone so that they hold before anyone has a GPU."""
import os
import re

import numpy as np
import pytest

import prims_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_H = os.path.join(ROOT, "box2d-mt_amd", "csrc", "b2d_scan.h")


# ---- references against naive loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem_ints", [1, 4])
@pytest.mark.parametrize("pattern", pr.SCAN_PATTERNS)
def test_exclusive_scan_against_loop(pattern, elem_ints):
    a = pr.scan_input(pattern, 300, elem_ints, seed=3)
    got = pr.exclusive_scan(a)
    run = [0] * elem_ints
    for i in range(301):
        assert list(np.atleast_1d(got[i])) == run
        if i < 300:
            run = [x + int(y) for x, y in zip(run, np.atleast_1d(a[i]))]
    assert got.dtype == np.int32 and got.shape[0] == 301


def test_exclusive_scan_refuses_overflow():
    with pytest.raises(AssertionError):
        pr.exclusive_scan(np.full(3, 2**30, np.int32))


def test_scan_input_components_differ():
    for pattern in ("flags", "mixed", "ones", "tile_id"):
        a = pr.scan_input(pattern, 5000, 4, seed=1)
        tot = a.astype(np.int64).sum(axis=0)
        assert len(set(tot.tolist())) == 4, pattern  # a swap of two components changes the result


def test_tile_aggregates_against_loop():
    a = pr.scan_input("mixed", 2500, 1, seed=2)
    want = [int(a[t:t + 1024].astype(np.int64).sum()) for t in range(0, 2500, 1024)]
    assert pr.tile_aggregates(a).tolist() == want


@pytest.mark.parametrize("how,kind", [("add", "sum"), ("min", "i32"), ("max", "u32"), ("min", "u32"), ("max", "i32")])
def test_ref_aggregate_against_loop(how, kind):
    rng = np.random.default_rng(4)
    key = rng.integers(0, 7, (3, 150))
    valid = rng.random((3, 150)) < 0.6
    val = pr.wave_values(kind, (3, 150), seed=1)
    base0 = pr.initial_base(kind if kind != "sum" else "count", 7)
    got = pr.ref_aggregate(how, base0, key, val, valid)
    want = [int(x) for x in base0]
    for r in range(3):
        for i in range(150):
            if valid[r, i]:
                k, v = int(key[r, i]), int(val[r, i])
                want[k] = want[k] + v if how == "add" else (min(want[k], v) if how == "min" else max(want[k], v))
    assert got.dtype == base0.dtype and [int(x) for x in got] == want


def test_ref_aggregate_signedness():
    # 0x80000000 is the largest of these as uint32 and the smallest as int32
    bits = np.array([1, 0x80000000, 0x7fffffff], np.uint32)
    zero = np.zeros(3, np.int64)
    assert pr.ref_aggregate("max", np.zeros(1, np.uint32), zero, bits, np.ones(3))[0] == 0x80000000
    assert pr.ref_aggregate("max", np.zeros(1, np.int32), zero, bits.view(np.int32), np.ones(3))[0] == 0x7fffffff
    assert pr.ref_aggregate("min", np.full(1, 5, np.int32), zero, bits.view(np.int32), np.ones(3))[0] == pr.INT_MIN


def test_ref_max_if_above_against_loop():
    for kind, base in (("nonpos", 0), ("nonpos", 7), ("pos", 0), ("pos", 2 * 10**6)):
        val = pr.wave_values(kind, (2, 200), seed=5)
        valid = np.random.default_rng(6).random((2, 200)) < 0.5
        want = base
        for v, ok in zip(val.ravel(), valid.ravel()):
            if ok and v > 0 and v > want:
                want = int(v)
        assert int(pr.ref_max_if_above(np.array([base], np.int32), val, valid)[0]) == want


def test_color_slot_table():
    assert [int(pr.color_slot(c)) for c in (0, 1, 64, 65, 66)] == [0, 32, 2048, 2080, 2081]
    assert pr.color_slot(np.arange(70)).tolist() == [c * 32 if c < 65 else 2080 + c - 65 for c in range(70)]


def _sequential_alloc(helper, base0, word, key, valid, block):
    """A naive allocator that keeps every promise of the header: threads in order, one at a time."""
    counter = [int(x) for x in base0]
    slots = np.zeros(key.shape, np.int32)
    for r in range(key.shape[0]):
        for i in range(key.shape[1]):
            if valid[r, i]:
                slots[r, i] = counter[int(word[r, i])]
                counter[int(word[r, i])] += 1
    return np.array(counter, np.int32), slots


@pytest.mark.parametrize("helper", sorted(pr.ORDER_GROUPS))
def test_check_alloc_accepts_a_correct_allocation_and_refuses_wrong_ones(helper):
    block = 128
    key, valid = pr.wave_pattern("holes", 300, 2, nkeys=5, seed=9)
    word = np.zeros_like(key) if helper == "blockAlloc" else key
    base0 = pr.initial_base("count", 5, seed=1)
    base1, slots = _sequential_alloc(helper, base0, word, key, valid, block)
    pr.check_alloc(helper, base0, base1, word, key, valid, slots, block)
    ok = np.argwhere(valid != 0)
    # (a) a counter that is off by one
    with pytest.raises(AssertionError, match=r"\(a\)"):
        pr.check_alloc(helper, base0, base1 + (np.arange(5) == int(word[tuple(ok[0])])), word, key, valid, slots, block)
    # (b) a slot handed out twice
    bad = slots.copy()
    a = tuple(ok[0])
    b = tuple(next(q for q in ok[1:] if word[tuple(q)] == word[a]))
    bad[b] = bad[a]
    with pytest.raises(AssertionError, match=r"\(b\)"):
        pr.check_alloc(helper, base0, base1, word, key, valid, bad, block)
    # an invalid lane with a slot
    bad = slots.copy()
    bad[tuple(np.argwhere(valid == 0)[0])] = 3
    with pytest.raises(AssertionError, match="invalid lane"):
        pr.check_alloc(helper, base0, base1, word, key, valid, bad, block)
    # (c) two lanes of one group swapped: a permutation of the right slots in the wrong order
    if pr.ORDER_GROUPS[helper] is not None:
        bad = None
        for r in range(2):
            for i in range(299):
                if valid[r, i] and valid[r, i + 1] and word[r, i] == word[r, i + 1] and (i + 1) % 64:
                    bad = slots.copy()
                    bad[r, i], bad[r, i + 1] = slots[r, i + 1], slots[r, i]
                    break
            if bad is not None:
                break
        with pytest.raises(AssertionError, match=r"\(c\)"):
            pr.check_alloc(helper, base0, base1, word, key, valid, bad, block)
    # fetch = false: counters only, every slot 0
    pr.check_alloc(helper, base0, base1, word, key, valid, np.zeros_like(slots), block, fetch=False)
    with pytest.raises(AssertionError):
        pr.check_alloc(helper, base0, base1, word, key, valid, slots, block, fetch=False)


def test_check_alloc_order_is_per_group_only():
    """What the header does not promise is not asked for: two waves of waveKeyedAlloc may take their slots in either order, and
    a key's second run in waveRunAlloc may come before its first."""
    key = np.zeros((1, 128), np.int32)
    valid = np.ones((1, 128), np.int32)
    slots = np.concatenate([np.arange(64, 128), np.arange(0, 64)])[None].astype(np.int32)
    pr.check_alloc("waveKeyedAlloc", np.zeros(1, np.int32), np.array([128], np.int32), key, key, valid, slots, 128)
    with pytest.raises(AssertionError, match=r"\(c\)"):
        pr.check_alloc("blockAlloc", np.zeros(1, np.int32), np.array([128], np.int32), key, key, valid, slots, 128)
    key = np.array([[1, 1, 2, 1, 1]], np.int32)
    slots = np.array([[2, 3, 0, 0, 1]], np.int32)
    pr.check_alloc("waveRunAlloc", np.zeros(3, np.int32), np.array([0, 4, 1], np.int32), key, key, np.ones((1, 5), np.int32), slots, 64)
    with pytest.raises(AssertionError, match=r"\(c\)"):
        pr.check_alloc("waveKeyedAlloc", np.zeros(3, np.int32), np.array([0, 4, 1], np.int32), key, key, np.ones((1, 5), np.int32), slots, 64)


# ---- the case tables --------------------------------------------------------------------------------------------------------
def test_scan_constants_match_the_header():
    text = open(SCAN_H).read()
    for name, want in (("SCAN_THREADS", 256), ("SCAN_ITEMS", 4), ("SCAN_ITEMS_WIDE", 16), ("SCAN_CHAIN_MAX_TILES", 256)):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
        assert m and int(m.group(1)) == want == getattr(pr, name), name
    assert re.search(r"sf\.epoch >= 0x3fffffffu", text) and pr.EPOCH_LAST == 0x3fffffff


def test_scan_table_forms():
    for cap_n, n, form in pr.SCAN_TABLE:
        assert 0 <= n <= cap_n <= 1400000
        assert pr.scan_form(cap_n) == form, (cap_n, n)
        assert pr.epoch_step(cap_n) == (0 if form == pr.THREE else 1)
    assert len(set(pr.SCAN_TABLE)) == len(pr.SCAN_TABLE) == 30
    for form in (pr.CHAIN4, pr.CHAIN16, pr.THREE):
        rows = [(c, n) for c, n, f in pr.SCAN_TABLE if f == form]
        counts = {n for _, n in rows}
        tile = pr.FORM_TILE[form]
        assert 0 in counts, form
        assert any(0 < n < 64 for n in counts), form               # small: less than a wave
        assert tile in counts and ({tile - 1, tile + 1} & counts), form  # one tile, and one beside it
        assert any(n == c and c > tile for c, n in rows), form      # full capacity, more than one tile
    # the boundaries between the forms, from both sides
    caps = {c for c, _, _ in pr.SCAN_TABLE}
    assert {262144, 262145, 1048576, 1048577} <= caps
    # tile 64 has exactly one look-back window, tile 65 needs a second; 257 tile sums cross the carry's first round
    tiles4 = {-(-n // 1024) for c, n, f in pr.SCAN_TABLE if f == pr.CHAIN4}
    assert {64, 65, 66} <= tiles4
    assert any(f == pr.CHAIN16 and -(-n // 4096) == 66 for _, n, f in pr.SCAN_TABLE)
    tiles3 = {-(-n // 1024) for c, n, f in pr.SCAN_TABLE if f == pr.THREE}
    assert {256, 257} <= tiles3 and max(tiles3) > 5 * 256


def test_no_scan_input_leaves_int32():
    biggest = max(n for _, n, _ in pr.SCAN_TABLE)
    for pattern in pr.SCAN_PATTERNS:
        out = pr.exclusive_scan(pr.scan_input(pattern, biggest, 4, seed=0))  # (asserts inside)
        assert out.shape == (biggest + 1, 4)
        if pattern not in ("zeros",):
            assert np.abs(out[-1]).min() > 0
    for elem_ints, tiles, pattern, seed in pr.REUSE_SEQUENCE:
        pr.exclusive_scan(pr.scan_input(pattern, tiles * 1024, elem_ints, seed))
    # mixed: |total| <= 1000 n stays under 1.4e9 whatever the draw
    assert 1000 * biggest <= 1.4e9 < pr.INT_MAX


def test_tile_id_aggregates_are_distinct():
    a = pr.scan_input("tile_id", 1400000, 4)
    for c in range(4):
        agg = pr.tile_aggregates(a[:, c])
        assert len(set(agg.tolist())) == len(agg) == 1368 and agg.min() > 0


def test_reuse_sequence_shape():
    (e0, t0, p0, _), (e1, t1, _, _), (e2, t2, _, _), (e3, t3, _, s3) = pr.REUSE_SEQUENCE
    assert (e0, t0, p0) == (1, 200, "tile_id") and (e1, t1) == (1, 3) and (e2, t2) == (4, 200) and (e3, t3) == (1, 200)
    assert len({s for _, _, _, s in pr.REUSE_SEQUENCE}) == 4
    # the words a 200-tile scan leaves must not read as published to the next: its aggregates differ tile by tile
    first = pr.tile_aggregates(pr.scan_input(p0, 200 * 1024, 1, 0))
    last = pr.tile_aggregates(pr.scan_input("mixed", 200 * 1024, 1, s3))
    assert (first != last).all()


def test_post_wrap_scan_differs_from_every_scan_before_it():
    """The scan that runs at epoch 1 again (W) meets the status words of the first scan (X, epoch 1) if the flag array was not
    zeroed, and in `work` the aggregates and prefixes of the scans since: every tile aggregate and every tile prefix of W differs
    from that of X, and of every other scan before W, so an accepted stale word shows."""
    assert pr.STATE_N == 200 * 1024 and len(pr.WRAP_BEFORE) == 3 and len(pr.WRAP_AFTER) == 3
    w = pr.scan_input(*pr.WRAP_AFTER[-1][:1], pr.STATE_N, 1, pr.WRAP_AFTER[-1][1])
    agg_w = pr.tile_aggregates(w)
    pre_w = np.cumsum(agg_w)
    assert len(agg_w) == 200
    for pattern, seed in pr.WRAP_BEFORE + pr.WRAP_AFTER[:-1]:
        other = pr.tile_aggregates(pr.scan_input(pattern, pr.STATE_N, 1, seed))
        assert (agg_w != other).all(), (pattern, seed)
        assert (pre_w != np.cumsum(other)).all(), (pattern, seed)
    # the second wrap test: the scans between X and W leave most of X's words alone
    assert 0 < pr.WRAP_SMALL_TILES < 64 and pr.scan_form(pr.WRAP_SMALL_TILES * 1024) == pr.scan_form(pr.STATE_N) == pr.CHAIN4


def test_launch_counts():
    for block in pr.BLOCKS:
        for grid in pr.GRIDS:
            full, one, sixty_three = pr.launch_counts(block, grid)
            assert full == block * grid and one % 64 == 1 and sixty_three % 64 == 63
            assert block * (grid - 1) < one < sixty_three < full  # the last workgroup is there and partial
    assert set(pr.BLOCKS) == {64, 192, 256, 1024} and set(pr.GRIDS) == {1, 7}


@pytest.mark.parametrize("name", pr.WAVE_PATTERNS)
def test_wave_pattern_claims(name):
    assert set(pr.PATTERN_CLAIMS) == set(pr.WAVE_PATTERNS)
    for nkeys in (pr.NKEYS, 65):
        for block in pr.BLOCKS:
            for grid in pr.GRIDS:
                n = block * grid
                key, valid = pr.wave_pattern(name, n, 2, nkeys=nkeys, block=block)
                assert key.shape == valid.shape == (2, n) and key.min() >= 0 and key.max() < nkeys
                assert pr.PATTERN_CLAIMS[name](*pr.as_waves(key, valid)), (name, nkeys, block, grid)
                # the cut counts keep the launch's other waves as they are
                for m in pr.launch_counts(block, grid)[1:]:
                    k2, v2 = pr.wave_pattern(name, m, 2, nkeys=nkeys, block=block)
                    assert np.array_equal(k2, key[:, :m]) and np.array_equal(v2, valid[:, :m])
    # a claim is not true of everything: a wave of one key has none of the other properties
    k, v = pr.as_waves(*pr.wave_pattern("all_same", 64, 1))
    for other in pr.WAVE_PATTERNS:
        assert pr.PATTERN_CLAIMS[other](k, v) == (other == "all_same"), other


def test_wave_patterns_reach_the_edges():
    # blockKeyedAlloc65's keys include 64, valid
    k, v = pr.wave_pattern("all_distinct", 128, 2, nkeys=65, block=128)
    assert 64 in k[v != 0] and 0 in k[v != 0]
    # the remainder path of B2D_WAVE_ATOMIC: a third key is left after two rounds, in some wave of every launch shape
    k, v = pr.as_waves(*pr.wave_pattern("three_keys", 64, 2))
    assert all(len(set(row)) == 3 for row in k)
    # lanes_0_63: both forms - one key in both lanes, and two keys
    k, v = pr.as_waves(*pr.wave_pattern("lanes_0_63", 128, 1))
    assert k[0, 0] == k[0, 63] and k[1, 0] != k[1, 63]
    # holes: about half the lanes, never all or none over a launch
    k, v = pr.wave_pattern("holes", 1024, 2)
    assert 0.4 < (v != 0).mean() < 0.6


@pytest.mark.parametrize("name", pr.BLOCK_PATTERNS)
def test_block_pattern_claims(name):
    for block in pr.BLOCKS:
        for grid in pr.GRIDS:
            key, valid = pr.wave_pattern(name, block * grid, 4, block=block)
            assert key.min() >= 0 and key.max() < pr.NKEYS
            assert pr.block_claim(name, key, valid, block), (name, block, grid)
    if name not in ("wg_one_key", "hot_one"):
        key, valid = pr.wave_pattern("wg_one_key", 256 * 7, 4, block=256)
        assert not pr.block_claim(name, key, valid, 256), name


def test_values_and_initial_contents():
    u = pr.wave_values("u32", (3, 4096))
    assert u.dtype == np.uint32 and set(pr.U32_SPECIAL.tolist()) <= set(u.ravel().tolist())
    assert ((u >= 0x80000000).mean() > 0.3) and ((u < 0x80000000).mean() > 0.3)  # both sides of 2^31
    i = pr.wave_values("i32", (3, 4096))
    assert i.dtype == np.int32 and {pr.INT_MIN, pr.INT_MAX, -1} <= set(i.ravel().tolist()) and (i < 0).mean() > 0.3
    s = pr.wave_values("sum", (4, 7168))
    assert np.abs(s.astype(np.int64)).sum() + 1000 < pr.INT_MAX  # a sum of all of them on top of any initial count stays in int32
    assert pr.wave_values("pos", 1000).min() >= 1 and pr.wave_values("nonpos", 1000).max() <= 0 and 0 in pr.wave_values("nonpos", 1000)
    # below, at and above what is offered: the extremes can never be beaten, the middle one is among the special values
    assert pr.initial_base("u32", 6).tolist() == [0, 0x80000000, 0xffffffff] * 2
    assert pr.initial_base("i32", 6).tolist() == [pr.INT_MIN, 0, pr.INT_MAX] * 2
    assert 0x80000000 in pr.U32_SPECIAL and 0 in pr.I32_SPECIAL
    c = pr.initial_base("count", 96)
    assert c.min() >= 0 and c.max() > 0


def test_max_if_above_cases():
    for block in pr.BLOCKS:
        for grid in pr.GRIDS:
            for n in pr.launch_counts(block, grid):
                assert pr.max_if_above_values("all_nonpositive", n, 2, block).max() <= 0
                mixed = pr.max_if_above_values("mixed", n, 2, block)
                assert mixed.max() < pr.MAX_IF_ABOVE_TOP and (n < 8 or (mixed.max() > 0 and mixed.min() <= 0))
                top = pr.max_if_above_values("max_in_last_wave", n, 2, block)
                r, i = np.unravel_index(np.argmax(top), top.shape)
                live = min(block, n - (i // block) * block)  # threads of that workgroup that own an element
                assert top[r, i] == pr.MAX_IF_ABOVE_TOP and r == 1 and (i % block) // 64 == (live - 1) // 64
                assert (top == pr.MAX_IF_ABOVE_TOP).sum() == 1


def test_spread_keys():
    k = pr.spread_keys(np.arange(pr.NKEYS), 1025)
    assert len(set(k.tolist())) == pr.NKEYS and k.min() >= 0 and k.max() == 1024 == k[0]  # bit 10: all 11 key bits matter
    assert (k >= 512).any() and (k < 32).any()
    assert pr.spread_keys(np.arange(6), 2).tolist() == [0, 1, 0, 1, 0, 1]
    # the patterns keep what their names claim under the map
    for name in pr.WAVE_PATTERNS:
        key, valid = pr.wave_pattern(name, 256, 2)
        assert pr.PATTERN_CLAIMS[name](*pr.as_waves(pr.spread_keys(key, 1025), valid)), name
