"""Host references (numpy only) and case tables for the integer primitives of box2d-mt_amd/csrc/b2d_scan.h (the device-wide
exclusive scan) and box2d-mt_amd/csrc/b2d_wave.h (the wave64 / workgroup aggregation helpers), as tests/probe/prims_probe.hip
runs them. tests/test_gpu_scan.py and tests/test_gpu_wave.py compare the device with what is here; tests/test_prims_ref_cpu.py
checks what is here against naive loops and checks that the case tables hold what their names claim.

Every comparison is exact. The allocators are not deterministic across waves, so their reference is three properties
(check_alloc): (a) the final counters, (b) the slots of a key are exactly c0 .. c0 + m - 1, (c) the order the header promises."""
import numpy as np

INT_MIN, INT_MAX = -2**31, 2**31 - 1
FILL_WORD = 0x5A5A5A5A  # what the probe's output array holds where the scan did not write

# ---- the scan -----------------------------------------------------------------------------------------------------------------
# the #defines of b2d_scan.h that decide the form of a scan (tests/test_prims_ref_cpu.py reads them from the header)
SCAN_THREADS = 256
SCAN_ITEMS = 4
SCAN_ITEMS_WIDE = 16
SCAN_CHAIN_MAX_TILES = 256
SCAN_TILE = SCAN_THREADS * SCAN_ITEMS
SCAN_TILE_WIDE = SCAN_THREADS * SCAN_ITEMS_WIDE
EPOCH_LAST = 0x3fffffff  # a scan that finds this epoch zeroes the flag words and starts again at 1

CHAIN4, CHAIN16, THREE = "chain4", "chain16", "three"
FORM_TILE = {CHAIN4: SCAN_TILE, CHAIN16: SCAN_TILE_WIDE, THREE: SCAN_TILE}


def scan_form(cap_n):
    """The form deviceExclusiveScan takes on a stream that is not being captured: by capacity alone."""
    blocks = max(1, -(-cap_n // SCAN_TILE))
    blocks_wide = -(-cap_n // SCAN_TILE_WIDE)
    if blocks_wide > SCAN_CHAIN_MAX_TILES:
        return THREE
    return CHAIN4 if blocks <= SCAN_CHAIN_MAX_TILES else CHAIN16


def epoch_step(cap_n):
    """What one scan adds to ScanFlags::epoch: the single-pass forms count their launches, the three kernels do not."""
    return 1 if cap_n <= 1048576 else 0


K = 1024
# (capN, n, the form the pair must take): the smallest capacities and counts at which each mechanism can go wrong
SCAN_TABLE = (
    [(1, 0, CHAIN4), (1, 1, CHAIN4), (1024, 1023, CHAIN4), (1024, 1024, CHAIN4), (1025, 1025, CHAIN4)]
    # the look-back reads 64 predecessors per round: tile 64 has exactly one window, tile 65 needs a second
    + [(66 * K, n, CHAIN4) for n in (64 * K, 64 * K + 1, 65 * K, 65 * K + 1)]
    # the last capacity of the form, with a live count far below it
    + [(262144, n, CHAIN4) for n in (0, 5, 129 * K + 3, 262143, 262144)]
    + [(262145, n, CHAIN16) for n in (0, 5, 4096, 4097, 262145)]
    + [(1048576, n, CHAIN16) for n in (65 * 4096 + 1, 1048575, 1048576)]
    # at 257 tile sums the carry of k_scan_blocksums crosses its first round; 1 400 000 is six rounds of it
    + [(1048577, n, THREE) for n in (0, 5, 1024, 1025, 256 * K, 256 * K + 1, 1048577)]
    + [(1400000, 1400000, THREE)]
)
SCAN_PATTERNS = ("flags", "ones", "zeros", "mixed", "tile_id")


def scan_input(pattern, n, elem_ints=1, seed=0):
    """int32 [n] (elem_ints 1) or [n, 4] (int4). The four components of an int4 come from four seeds (or four multiples), so a
    swap of components shows."""
    cols = []
    for c in range(elem_ints):
        rng = np.random.default_rng(1000 * seed + 17 * c + 1)
        if pattern == "flags":  # what keepFlag holds
            a = (rng.random(n) < 0.1).astype(np.int32)
        elif pattern == "ones":
            a = np.full(n, 1 + c, np.int32)
        elif pattern == "zeros":
            a = np.zeros(n, np.int32)
        elif pattern == "mixed":  # 1.4 M elements stay under 1.4e9
            a = rng.integers(-1000, 1001, n).astype(np.int32)
        elif pattern == "tile_id":  # every tile aggregate distinct: a mis-indexed look-back cannot cancel
            a = np.zeros(n, np.int32)
            a[::SCAN_TILE] = (np.arange(len(a[::SCAN_TILE])) + 1) * (c + 1)
        else:
            raise ValueError(pattern)
        cols.append(a)
    return cols[0] if elem_ints == 1 else np.ascontiguousarray(np.stack(cols, axis=1))


def exclusive_scan(a):
    """out[i] = sum of a[0 .. i), out[n] = the total: [n + 1] or [n + 1, 4], int32. Summed in int64; must fit int32."""
    a = np.asarray(a)
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:], np.int64)
    np.cumsum(a.astype(np.int64), axis=0, out=out[1:])
    assert out.min(initial=0) >= INT_MIN and out.max(initial=0) <= INT_MAX, "the running sum leaves int32"
    return out.astype(np.int32)


def tile_aggregates(a, tile=SCAN_TILE):
    """Sum of every tile of `tile` elements (the last one may be short), int64."""
    a = np.asarray(a).astype(np.int64)
    return np.add.reduceat(a, np.arange(0, len(a), tile), axis=0) if len(a) else a[:0]


# the scans of the "state across calls" tests: 200 tiles each, (pattern, seed)
STATE_N = 200 * SCAN_TILE
WRAP_BEFORE = (("tile_id", 0), ("mixed", 11), ("flags", 12))   # X first: epochs 1, 2, 3
WRAP_AFTER = (("mixed", 13), ("flags", 14), ("mixed", 15))     # Y, Z, W: 0x3ffffffe, 0x3fffffff, then 1 again
# ... and the same with scans of WRAP_SMALL_TILES tiles between the first and the last: 200-tile scans overwrite every status
# word with their own epoch, so only here do words of epoch 1 outlive the wrap - in the tiles the small scans never touch
WRAP_SMALL_TILES = 3
REUSE_SEQUENCE = ((1, 200, "tile_id", 0), (1, 3, "mixed", 21), (4, 200, "mixed", 22), (1, 200, "mixed", 23))  # (elem_ints, tiles, pattern, seed)

# ---- the helpers of b2d_wave.h ----------------------------------------------------------------------------------------------
OPS = {"waveAtomicAddInt": 0, "waveAtomicMinInt": 1, "waveAtomicMaxU32": 2, "waveAtomicMaxU32Guarded": 3, "waveAtomicMinU32": 4,
       "blockMaxU32": 5, "blockAtomicMaxIfAbove": 6, "blockHot": 7, "blockAlloc": 8, "waveKeyedAlloc": 9, "waveRunAlloc": 10,
       "waveKeyedAllocOnce": 11, "blockKeyedAlloc65": 12}
BLOCKS = (64, 192, 256, 1024)
GRIDS = (1, 7)
NKEYS = 96  # counters of the general cases

COLOR_SLOT_STRIDE, COLOR_SLOT_PADDED = 32, 65


def color_slot(c):
    """colorSlot of b2d_wave.h: the first 65 colours a 128-byte line apart, the rest densely behind them."""
    c = np.asarray(c)
    return np.where(c < COLOR_SLOT_PADDED, c * COLOR_SLOT_STRIDE, COLOR_SLOT_PADDED * COLOR_SLOT_STRIDE + (c - COLOR_SLOT_PADDED))


def launch_counts(block, grid):
    """The element counts every helper runs with: all threads, n % 64 == 1, n % 64 == 63."""
    return (block * grid, block * grid - 63, block * grid - 1)


RUN_LENGTHS = (1, 2, 3, 5, 8, 13, 32)
WAVE_PATTERNS = ("all_same", "two_interleaved", "three_keys", "all_distinct", "runs", "runs_repeat", "none_valid", "only_lane0",
                 "only_lane63", "lanes_0_63", "holes")
# patterns that are written per WORKGROUP (they need the block size), for blockMaxU32 and blockHot
BLOCK_PATTERNS = ("wg_one_key", "wg_one_wave_other", "wg_one_wave_mixed", "wg_one_wave_silent", "wg_key_changes", "hot_one",
                  "hot_scattered", "hot_first_wave_silent")


def _runs(lengths, keys):
    return np.repeat(np.asarray(keys, np.int64), lengths)


def wave_pattern(name, n, rounds, nkeys=NKEYS, block=64, seed=0):
    """(key, valid): int32 [rounds, n]. Written wave by wave (64 lanes; `gw` counts the waves of the launch, `r` the rounds) and
    cut at n; invalid lanes hold keys in range too. tests/test_prims_ref_cpu.py checks PATTERN_CLAIMS[name] on the result."""
    nw = -(-n // 64)
    lane = np.arange(64)
    key = np.zeros((rounds, nw, 64), np.int64)
    valid = np.ones((rounds, nw, 64), bool)
    rng = np.random.default_rng(77 + seed)
    wpb = block // 64
    for r in range(rounds):
        for gw in range(nw):
            wg, wv = divmod(gw, wpb)
            a = (gw // 2 + r) % nkeys
            if name == "all_same":
                k = np.full(64, a)
            elif name == "two_interleaved":
                k = np.where(lane % 2 == 0, a, (a + 17) % nkeys)
            elif name == "three_keys":  # the lane-by-lane remainder path of B2D_WAVE_ATOMIC
                k = (a + 29 * (lane % 3)) % nkeys
            elif name == "all_distinct":
                k = (lane + 3 * gw + r) % nkeys
            elif name == "runs":
                # even gw + r: the run of 32 ends at lane 63; odd: a single-lane run sits at lane 63
                lengths = RUN_LENGTHS if (gw + r) % 2 == 0 else RUN_LENGTHS[::-1]
                k = _runs(lengths, [(3 * gw + 11 * j + r) % nkeys for j in range(len(lengths))])
            elif name == "runs_repeat":  # A A B A A: one key in two runs that are not neighbours
                b, c = (a + 31) % nkeys, (a + 47) % nkeys
                k = np.roll(_runs((10, 3, 20, 1, 30), [a, b, a, c, a]), (gw + r) % 5)
            elif name == "none_valid":
                k = np.full(64, a)
                valid[r, gw] = False
            elif name == "only_lane0":
                k = np.full(64, a)
                valid[r, gw] = lane == 0
            elif name == "only_lane63":
                k = np.full(64, a)
                valid[r, gw] = lane == 63
            elif name == "lanes_0_63":  # one key in both (even gw) or two keys
                k = np.where(lane < 32, a, a if gw % 2 == 0 else (a + 5) % nkeys)
                valid[r, gw] = (lane == 0) | (lane == 63)
            elif name == "holes":  # runs over five keys, cut by invalid lanes that hold the run's key
                five = (a + 13 * np.arange(5)) % nkeys
                k = np.repeat(five[rng.integers(0, 5, 64)], rng.integers(1, 6, 64))[:64]
                valid[r, gw] = rng.random(64) < 0.5
            elif name == "wg_one_key":  # the one-atomic path of blockMaxU32Flush
                k = np.full(64, wg % nkeys)
            elif name == "wg_one_wave_other":
                k = np.full(64, (wg + (40 if wv == wpb - 1 and wpb > 1 else 0)) % nkeys)
            elif name == "wg_one_wave_mixed":
                k = (wg + 29 * (lane % 3)) % nkeys if wv == wpb - 1 else np.full(64, wg % nkeys)
            elif name == "wg_one_wave_silent":
                k = np.full(64, wg % nkeys)
                valid[r, gw] = not (wv == wpb - 1 and wpb > 1)
            elif name == "wg_key_changes":  # the `other` path of blockMaxU32Offer
                k = np.full(64, (wg + 7 * r) % nkeys)
            elif name == "hot_one":
                k = np.full(64, 5 % nkeys)
            elif name == "hot_scattered":
                k = np.where(rng.random(64) < 0.75, wg % nkeys, rng.integers(0, nkeys, 64))
            elif name == "hot_first_wave_silent":
                k = np.where(lane % 8 == 0, (a + 9) % nkeys, wg % nkeys)
                valid[r, gw] = not (r == 0 and wv == 0)
            else:
                raise ValueError(name)
            key[r, gw] = k
    key = key.reshape(rounds, nw * 64)[:, :n]
    valid = valid.reshape(rounds, nw * 64)[:, :n]
    return np.ascontiguousarray(key, np.int32), np.ascontiguousarray(valid, np.int32)


def spread_keys(key, nkeys):
    """The keys of a pattern (below NKEYS) spread over [0, nkeys) for waveKeyedAllocOnce: 37 k + nkeys - 1 modulo nkeys, which
    keeps distinct keys distinct where 37 is coprime to nkeys and NKEYS <= nkeys (key 0 becomes the highest key); else k % nkeys."""
    key = np.asarray(key).astype(np.int64)
    return ((key * 37 + nkeys - 1) % nkeys if nkeys >= NKEYS else key % nkeys).astype(np.int32)


def as_waves(key, valid):
    """[rounds, n] -> [rounds * waves, 64] as the device sees them: threads beyond n are invalid lanes."""
    rounds, n = key.shape
    nw = -(-n // 64)
    k = np.zeros((rounds, nw * 64), np.int64)
    v = np.zeros((rounds, nw * 64), bool)
    k[:, :n] = key
    v[:, :n] = valid != 0
    return k.reshape(-1, 64), v.reshape(-1, 64)


def _run_heads(k, v):
    """waveRunAlloc's heads, per wave row: a valid lane whose left neighbour is invalid or holds another key."""
    head = v.copy()
    head[:, 1:] &= ~v[:, :-1] | (k[:, 1:] != k[:, :-1])
    return head


def _some(rows):
    return bool(np.any(rows))


def _claim_runs(k, v):
    full = v.all(axis=1)
    ends_63 = full & (k[:, 63] == k[:, 62])
    single_63 = full & (k[:, 63] != k[:, 62])
    return _some(ends_63) and _some(single_63)


def _claim_runs_repeat(k, v):
    for row, ok in zip(k, v):
        if not ok.all():
            continue
        heads = row[np.flatnonzero(_run_heads(row[None], ok[None])[0])]
        for j in range(len(heads) - 2):
            if heads[j] in heads[j + 2:]:
                return True
    return False


def _claim_holes(k, v):
    for row, ok in zip(k, v):
        for j in range(1, 63):
            if not ok[j] and ok[j - 1] and ok[j + 1] and row[j - 1] == row[j] == row[j + 1]:
                return True
    return False


def _distinct_valid(k, v):
    return np.array([len(set(row[ok])) for row, ok in zip(k, v)])


def _mask_is(v, lanes):
    want = np.zeros(64, bool)
    want[list(lanes)] = True
    return _some((v == want).all(axis=1))


# name -> f(k, v) over as_waves(): some wave really has the property the name claims
PATTERN_CLAIMS = {
    "all_same": lambda k, v: _some(v.all(axis=1) & (k == k[:, :1]).all(axis=1)),
    "two_interleaved": lambda k, v: _some(v.all(axis=1) & (_distinct_valid(k, v) == 2) & (k[:, 0::2] == k[:, :1]).all(axis=1)
                                          & (k[:, 1::2] == k[:, 1:2]).all(axis=1)),
    "three_keys": lambda k, v: _some(_distinct_valid(k, v) >= 3),
    "all_distinct": lambda k, v: _some(v.all(axis=1) & (_distinct_valid(k, v) == 64)),
    "runs": _claim_runs,
    "runs_repeat": _claim_runs_repeat,
    "none_valid": lambda k, v: _some(~v.any(axis=1)),
    "only_lane0": lambda k, v: _mask_is(v, [0]),
    "only_lane63": lambda k, v: _mask_is(v, [63]),
    "lanes_0_63": lambda k, v: _mask_is(v, [0, 63]),
    "holes": _claim_holes,
}


def block_claim(name, key, valid, block):
    """The same for the per-workgroup patterns, at a count that fills every workgroup."""
    rounds, n = key.shape
    assert n % block == 0
    wpb = block // 64
    k = key.reshape(rounds, n // block, wpb, 64).astype(np.int64)
    v = valid.reshape(rounds, n // block, wpb, 64) != 0
    one_key = (k == k[:, :, :1, :1]).all(axis=(2, 3))  # [rounds, workgroups]
    wave_uniform = (k == k[:, :, :, :1]).all(axis=3)   # [rounds, workgroups, waves]
    if name == "wg_one_key":
        return _some(v.all(axis=(0, 2, 3)) & one_key.all(axis=0))
    if name == "wg_one_wave_other":  # every wave uniform, all valid, two keys in the workgroup
        return wpb == 1 or _some(v.all(axis=(2, 3)) & wave_uniform.all(axis=2) & ~one_key)
    if name == "wg_one_wave_mixed":
        return _some(v.all(axis=(2, 3)) & ~wave_uniform[:, :, -1] & (wpb == 1 or wave_uniform[:, :, 0]))
    if name == "wg_one_wave_silent":
        return wpb == 1 or _some(~v[:, :, -1].any(axis=2) & v[:, :, :-1].all(axis=(2, 3)) & one_key)
    if name == "wg_key_changes":
        return rounds > 1 and _some(one_key.all(axis=0) & (k[0, :, 0, 0] != k[1, :, 0, 0]))
    if name == "hot_one":
        return bool((k == k.flat[0]).all() and v.all())
    if name == "hot_scattered":
        return _some(~one_key) and all(np.bincount(k[0, g].ravel()).max() > block // 2 for g in range(n // block))
    if name == "hot_first_wave_silent":
        return bool(not v[0, :, 0].any() and (rounds == 1 or v[1:].all()))
    raise ValueError(name)


U32_SPECIAL = np.array([0, 1, 0x7fffffff, 0x80000000, 0xffffffff], np.uint32)
I32_SPECIAL = np.array([INT_MIN, INT_MAX, -1, 0, 1], np.int32)


def wave_values(kind, shape, seed=0):
    """Values offered: "u32" / "i32" a third of them the special values, the rest any 32 bits; "sum" small enough for 10^5 of them
    to stay in int32; "pos" 1 .. 10^6 and "nonpos" -10^6 .. 0 for blockAtomicMaxIfAbove."""
    rng = np.random.default_rng(500 + seed)
    if kind == "u32":
        rnd = rng.integers(0, 2**32, shape, dtype=np.uint64).astype(np.uint32)
        return np.where(rng.random(shape) < 1 / 3, U32_SPECIAL[rng.integers(0, 5, shape)], rnd)
    if kind == "i32":
        rnd = rng.integers(INT_MIN, INT_MAX + 1, shape).astype(np.int32)
        return np.where(rng.random(shape) < 1 / 3, I32_SPECIAL[rng.integers(0, 5, shape)], rnd)
    if kind == "sum":
        return rng.integers(-1000, 1001, shape).astype(np.int32)
    if kind == "pos":
        return rng.integers(1, 10**6 + 1, shape).astype(np.int32)
    if kind == "nonpos":
        return np.where(rng.random(shape) < 0.25, 0, rng.integers(-10**6, 1, shape)).astype(np.int32)
    raise ValueError(kind)


MAX_IF_ABOVE_CASES = ("all_nonpositive", "mixed", "max_in_last_wave")
MAX_IF_ABOVE_TOP = 2 * 10**6


def max_if_above_values(case, n, rounds, block, seed=0):
    """Values for blockAtomicMaxIfAbove, int32 [rounds, n]: nothing to offer (the word stays as it is); offers and non-offers
    mixed; the same with the maximum in the last live wave of the first workgroup, in the last round."""
    neg = wave_values("nonpos", (rounds, n), seed)
    if case == "all_nonpositive":
        return neg
    val = np.where(np.random.default_rng(40 + seed).random((rounds, n)) < 0.5, wave_values("pos", (rounds, n), seed), neg)
    if case == "max_in_last_wave":
        val[rounds - 1, min(block, n) - 1] = MAX_IF_ABOVE_TOP
    return val.astype(np.int32)


def initial_base(kind, length, seed=0):
    """Initial contents that lie below, at and above what is offered, key by key (the WORTH_BELOW / WORTH_ABOVE guards have to
    leave a better stored value alone); small counts for sums and counters."""
    q = np.arange(length) % 3
    if kind == "u32":
        return np.choose(q, [0, 0x80000000, 0xffffffff]).astype(np.uint32)
    if kind == "i32":
        return np.choose(q, [INT_MIN, 0, INT_MAX]).astype(np.int32)
    return np.random.default_rng(900 + seed).integers(0, 1000, length).astype(np.int32)


def ref_aggregate(how, base0, word, val, valid):
    """The final array: `how` in add / min / max over the valid offers of all rounds, in base0's signedness, from base0.
    `word`: the element of the array an offer aims at."""
    sel = np.asarray(valid).ravel() != 0
    word = np.asarray(word).ravel()[sel]
    val = np.asarray(val).ravel()[sel].astype(base0.dtype)
    if how == "add":
        out = base0.astype(np.int64)
        np.add.at(out, word, val.astype(np.int64))
        assert out.min() >= INT_MIN and out.max() <= INT_MAX, "a sum leaves int32"
        return out.astype(base0.dtype)
    out = base0.copy()
    (np.minimum if how == "min" else np.maximum).at(out, word, val)
    return out


def ref_max_if_above(base0, val, valid):
    """blockAtomicMaxIfAbove on one int word: values <= 0 are no offer."""
    v = np.asarray(val).astype(np.int32).ravel()[np.asarray(valid).ravel() != 0]
    v = v[v > 0]
    out = base0.copy()
    if len(v):
        out[0] = max(int(out[0]), int(v.max()))
    return out


ORDER_GROUPS = {"waveKeyedAlloc": "wave_key", "waveKeyedAllocOnce": "wave_key", "waveRunAlloc": "run", "blockAlloc": "block",
                "blockKeyedAlloc65": None}


def check_alloc(helper, base0, base1, word, key, valid, slots, block, fetch=True):
    """The three properties of an allocator's result; raises AssertionError naming the first that fails.
    word [rounds, n]: the counter a thread's key addresses (key, key * stride, colorSlot(key) or 0)."""
    key = np.asarray(key).astype(np.int64)
    ok = np.asarray(valid) != 0
    word = np.asarray(word).astype(np.int64)
    slots = np.asarray(slots).astype(np.int64)
    rounds, n = key.shape
    # (a) every counter moved by its valid offers
    want = base0.astype(np.int64) + np.bincount(word[ok], minlength=len(base0))
    assert np.array_equal(base1.astype(np.int64), want), "(a) final counters differ at %s" % np.flatnonzero(base1 != want)[:8]
    assert not slots[~ok].any(), "an invalid lane got a slot other than 0"
    if not fetch:
        assert not slots.any(), "fetch = false returned a slot"
        return
    # (b) the slots of a counter, sorted, are c0 .. c0 + m - 1
    w, s = word[ok], slots[ok]
    order = np.lexsort((s, w))
    w, s = w[order], s[order]
    first = np.searchsorted(w, w, side="left")
    assert np.array_equal(s, base0.astype(np.int64)[w] + np.arange(len(w)) - first), "(b) the slots of a counter are not c0 .. c0 + m - 1"
    # (c) the promised order: consecutive slots within a group, in thread order
    how = ORDER_GROUPS[helper]
    if how is None:
        return
    i = np.broadcast_to(np.arange(n), (rounds, n))
    r = np.broadcast_to(np.arange(rounds)[:, None], (rounds, n))
    if how == "run":  # valid neighbours in one wave with one key
        same = ok[:, 1:] & ok[:, :-1] & (key[:, 1:] == key[:, :-1]) & (i[:, 1:] % 64 != 0)
        assert np.array_equal(slots[:, 1:][same], slots[:, :-1][same] + 1), "(c) a run's slots are not consecutive in lane order"
        return
    group = [r[ok], i[ok] // block] if how == "block" else [r[ok], i[ok] // 64, word[ok]]
    order = np.lexsort([i[ok]] + group[::-1])
    g = np.stack(group, axis=1)[order]
    s = slots[ok][order]
    same = (g[1:] == g[:-1]).all(axis=1)
    assert np.array_equal(s[1:][same], s[:-1][same] + 1), "(c) a group's slots are not consecutive in thread order"
