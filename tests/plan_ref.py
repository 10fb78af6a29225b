"""Host reference (numpy only: no GPU, no ctypes) of the PLAN every large-island solver reads, and the checker that holds a
recorded plan to it. The solvers - k_solve_blocks, k_blocks_sweep, the launch-per-colour kernels with k_large_rest /
k_sweep_end / k_rest_hub - trust one plan: the colours of the rows, the per-body masks, the block partition, the row table
and the hub list. A wrong plan that every solver reads alike passes every parity and determinism test; this module
recomputes what the plan must be from the world's contact list alone and names what differs.

    plan  = read_plan(read, n_bodies, counters)       # `read(which, first, count, dtype)`: b2hip_debug_read, wrapped by the caller
    world = World(body_flags, labels, body_a, body_b, solid, joints)
    check_plan(plan, world) -> [Violation(name, where, detail), ...]     # empty: the plan is what it must be

tests/test_plan_ref_cpu.py builds synthetic plans and corrupts them one thing at a time (every violation under its own
name); tests/test_gpu_large_plan.py reads the device's plan behind every step.

WHERE EACH ARRAY HOLDS THE STEP'S PLAN (b2hip_debug_read id in brackets; "solve" = b2hip_solve of that step)

  deg [14]             k_island_union counts it (k_island_init zeroes it); final behind the island build, untouched until the
                       next step's k_island_init. Every non-static body, whatever tier its island is in.
  b_blk1 [17]          home block + 1. Written by k_part_assign (a new partition), k_block_census / k_color_check (an adoption
                       made permanent), zeroed by the host when the partition is dissolved (largeIslandPolicy) and by
                       k_part_keys for bodies outside the large islands. Final behind repartition(), i.e. before layoutRows.
  effective block [26] effBlk evaluated on the host from b_blk1, b_adopt, b_flags and the counters: holds from the island build
                       (k_island_edges / k_block_adopt fill b_adopt, k_island_assign sets BF_LARGE) to the next k_island_init.
  bodyColorMask [13]   k_color_masks stores it (k_island_init / k_color_begin / k_color_recheck_begin zero it); k_color_small
                       and k_color_resolve OR in what they hand out, the compaction of k_color_small takes a bit out. Final
                       behind colorLargeIslands. On a step without large islands lately (largeHintSteps == 0) k_color_masks
                       does not run: all zero.
  colour census [12]   colorCount: k_color_check counts (k_island_init's colorCheckBegin zeroes), k_color_small /
                       k_color_resolve keep it current. Final behind colorLargeIslands. Exact-order mode: k_exact_convert.
  li_ref [18],         k_color_fill (layoutRows) writes rows [0, large_island_contacts); k_hub_build / k_hub_order then
  rowColor [19]        permute the li_ref of the hub group's rows among themselves (their colour is 63 throughout). Valid from
                       layoutRows to the next step's layoutRows; a step without large islands leaves the last plan's rows
                       (the row count of THAT step is gone: do not read).
  blkRowStart [20]     k_block_census, [0, nBlocks]; valid while blockSort == 1 (else it is the census of a partition the
                       rows are not laid out by).
  bodyActive [16],     zeroed by k_island_init (and by k_solver_recover_reset before a safe pass), ORed by k_color_fill;
  bodyRest [21]        bodyRest bit 63 also by k_joints_fill. Valid from layoutRows to the next k_island_init. A step without
                       large islands leaves zeros.
  hubList [15]         k_hub_build, or k_hub_fill + k_hub_order: written only on a step that has hub rows (SolveStep::hasHubs);
                       [0, nHubRows). The TOI phase uses words [0, 16 + 16 * domains) as scratch for its timers
                       (b2d_kernels_toi.h:1365-1368): in a world with continuous physics the list is valid only between
                       b2hip_solve and b2hip_solve_toi.
  plan numbers [27]    the host's record of the last pass (LargePass::recordPlan) and the device's counters as they stand.
                       nHubRows / nHubWide are this step's from layoutRows on; b2hip_get_counters' hub_constraints is
                       refreshed at b2hip_step_end only.

The tests read between b2hip_solve and b2hip_sync_fixtures in worlds with continuous physics (the TOI sub-steps update
TOUCHING flags and overwrite hubList) and behind b2hip_step otherwise: without continuous physics nothing changes a contact's
TOUCHING / ENABLED flag between the island build and the end of the step (contacts are updated and destroyed by Collide; the
pair update only appends contacts, which do not touch yet), so the contact list behind the step is the one the solve saw.
Only steps with large islands are read.

WHERE THE KERNELS SAY OTHERWISE THAN THE ISSUE THAT ASKED FOR THIS MODULE

  * hubList holds ROW indices (places in li_ref), not contact indices: k_hub_fill, `W.hubList[...] = W.hubRowOf[i]`
    (b2d_kernels_solve_large.h); "in ascending contact index" is about li_ref[hubList[k]].x.
  * hubWide == 0: the list is TWO ascending runs, not one - the rows of a hub (rowIsHubs) first, then the other rows that
    are swept in order (orphans, rows without a free colour): k_hub_flag, `f = 1` / `f = 1 << 20`, and k_hub_fill's two
    ranks; k_hub_build: `cls = rowIsHubs(...) ? 0 : 1` above the contact index in the sort key.
  * hubWide == 1: a wide row's other side may be STATIC (the hub resting on the ground): k_hub_flag / k_hub_build test the
    partner's degree and hubFirst only `if (otherNs ...)`; k_hub_order: "the hub against a static body: ready at once".
    "Pairwise different partners" and "the partner's lowest contact index" hold among the non-static partners.
    The rows behind the wide ones are in ascending contact index (class 1 of k_hub_build's key; k_hub_fill's second rank).
  * bodyRest bit 63 is also set, whatever restFirst is, on every non-static body of a live joint of a large island
    (k_joints_fill, b2d_kernels_island.h: `atomicOr(&W.bodyRest[ids[q]], 1ull << HUB_COLOR)`), except behind a recovery
    (k_solver_recover_reset wipes the masks and the joint lists are not filled again).
  * an INTERIOR row may carry an upper-range colour when no lower colour is free on its two bodies (colorClassMask: "it
    may spill into the upper range then"); with at most 30 rows per body that needs B2HIP_TEST_MAX_COLORS. The checker
    accepts it exactly then: every permitted colour below the row's is taken on one of its bodies. A CUT row below 32 is
    never accepted.
  * a row is in the hub group without a hub and without being an orphan only when NO permitted colour of its class was
    free (k_color_small / k_color_resolve: `used == ~0ull`); the checker recomputes that from the other rows on its bodies.
  * `colors` is the highest colour in use + 1 - except on a step with such rows: handing out "colour" 63 leaves the count at
    64 (`atomicMax(&S->c.nColors, color + 1)`, k_color_small's `s_maxColor`), which the host cuts to 63
    (b2hip_host_phases.h, solveLargeIslands: `if (!s.exactLarge && s.nColors > HUB_COLOR) s.nColors = HUB_COLOR`); the empty
    colours between are skipped by their census.
  * "no body is home to two blocks": b_blk1 is one word per body; what is checked is that it lies in [0, blocks] and that
    a body with a home block has that block as its effective block.
  * the persistent colours themselves (ContactArrays::color, li_color) have no read-back; rowColor is li_color in row order
    (k_color_fill), and that is what is checked.
  * contacts between sensors: b2hip_get_contacts reports TOUCHING and ENABLED, not CF_SENSOR. `World.solid` is the caller's;
    the scenes of tests/test_gpu_large_plan.py have no sensors, so touching & enabled is the solid set there.
"""
from collections import namedtuple

import numpy as np

# ---- the #defines of box2d-mt_amd/csrc/b2d_world.h the plan is built on (tests/test_plan_ref_cpu.py reads them from the header)
MAX_COLORS = 64
HUB_COLOR = MAX_COLORS - 1
HUB_DEGREE = 30
CUT_COLOR_BASE = 32
MAX_BLOCKS = 1024
SMALL_ISLAND_MAX_JOINTS = 64
TINY_ISLAND_MAX_W = 128
BF_TYPE_MASK, BT_STATIC, BF_ACTIVE, BF_LARGE = 0x3, 0, 0x40, 0x100
NO_REST = 0x7fffffff
CENSUS_SLOTS = 65  # what b2hip_debug_read 12 serves

SOLVER_LAUNCHES, SOLVER_BLOCKS, SOLVER_SWEEP, SOLVER_EXACT = 0, 1, 2, 3

# b2hip_debug_read 27, in order
PLAN_FIELDS = ("passes", "solver", "safe", "rest_first", "tail_first", "big_end", "use_rest", "fuse_hub", "block_sort", "hub_wide",
               "serial_orphans", "pass_colors", "has_hubs", "has_joints", "hub_build_one", "use_sweep_end", "leftover_apart",
               "hub_rows", "hub_wide_rows", "hub_body", "hub_degree", "blocks", "colors", "max_degree",
               "force_large", "small_max_w", "test_max_colors", "joints")

Violation = namedtuple("Violation", "name where detail")


class World:
    """What the reference recomputes the plan from. body_flags: DW::b_flags (b2hip_debug_read 4; type and BF_ACTIVE are used),
    labels: b2hip_get_island_labels, body_a / body_b / solid: one entry per contact of b2hip_get_contacts (solid = touching,
    enabled, no sensor), joints: [n, 4] bodyA, bodyB, gear bodyC, bodyD (b2hip_debug_read 28; -1 where there is none)."""

    def __init__(self, body_flags, labels, body_a, body_b, solid, joints=None):
        self.body_flags = np.asarray(body_flags, np.uint32)
        self.labels = np.asarray(labels, np.int64)
        self.body_a = np.asarray(body_a, np.int64)
        self.body_b = np.asarray(body_b, np.int64)
        self.solid = np.asarray(solid, bool)
        self.joints = np.zeros((0, 4), np.int64) if joints is None else np.asarray(joints, np.int64).reshape(-1, 4)
        self.n_bodies = len(self.body_flags)
        self.non_static = (self.body_flags & BF_TYPE_MASK) != BT_STATIC
        self.active = (self.body_flags & BF_ACTIVE) != 0


class Plan:
    """A recorded plan: `numbers` (PLAN_FIELDS), `counters` (b2hip_get_counters: large_island_contacts, colors, blocks,
    cut_constraints, block_max_rows) and the arrays named in the module's docstring."""

    ARRAYS = ("li_ref", "row_color", "deg", "body_color_mask", "body_active", "body_rest", "b_blk1", "eff_blk", "blk_row_start",
              "census", "hub_list")

    def __init__(self, numbers, counters, **arrays):
        self.numbers = dict(numbers)
        self.counters = dict(counters)
        for k in self.ARRAYS:
            setattr(self, k, np.array(arrays[k]))

    def copy(self):
        return Plan(self.numbers, self.counters, **{k: getattr(self, k).copy() for k in self.ARRAYS})

    @property
    def n_rows(self):
        return int(self.counters["large_island_contacts"])


def read_plan(read, n_bodies, counters):
    """The plan of the last solve through `read(which, first, count, dtype)` -> numpy array of `count` elements of `dtype`
    (b2hip_debug_read; the int4 rows of id 18 are read as `4 * count` int32 by the caller's wrapper: dtype "i4x4")."""
    numbers = dict(zip(PLAN_FIELDS, (int(v) for v in read(27, 0, len(PLAN_FIELDS), "i4"))))
    n_rows = int(counters["large_island_contacts"])
    nb = min(max(numbers["blocks"], 0), MAX_BLOCKS)
    n_hub = min(max(numbers["hub_rows"], 0), n_rows)
    return Plan(numbers, counters,
                li_ref=read(18, 0, n_rows, "i4x4").reshape(-1, 4), row_color=read(19, 0, n_rows, "i4"),
                deg=read(14, 0, n_bodies, "i4"), body_color_mask=read(13, 0, n_bodies, "u8"), body_active=read(16, 0, n_bodies, "u8"),
                body_rest=read(21, 0, n_bodies, "u8"), b_blk1=read(17, 0, n_bodies, "i4"), eff_blk=read(26, 0, n_bodies, "i4"),
                blk_row_start=read(20, 0, nb + 1, "i4"), census=read(12, 0, CENSUS_SLOTS, "i4"), hub_list=read(15, 0, n_hub, "i4"))


def own_id_block(body, nb):
    """ownIdBlock of box2d-mt_amd/csrc/b2d_math.h restated: the block (+ 1) a body takes by its own id - hash(body) mod nb, the
    remainder by way of a float32 quotient with both corrections. `body`, `nb`: integers or arrays (broadcast)."""
    body = np.asarray(body, np.int64)
    nb = np.asarray(nb, np.int64)
    x = ((body * 2654435761) & 0xffffffff) >> 8
    q = (x.astype(np.float32) / nb.astype(np.float32)).astype(np.int64)
    r = x - q * nb
    r = np.where(r < 0, r + nb, np.where(r >= nb, r - nb, r))
    return (1 + r).astype(np.int32)


def eff_blk_from(b_blk1, b_adopt, body_flags, blocks, own_id_blocks):
    """effBlk of b2d_kernels_island.h from its ingredients: the home block, else the block a neighbour offered (the low 11 bits
    of the offer), else - for a body of a large island, where `own_id_blocks` (plain islands: no joints, no hub) - the block
    by its own id. 0: none."""
    b_blk1 = np.asarray(b_blk1, np.int64)
    offered = np.asarray(b_adopt, np.int64) & 0x7ff
    large = (np.asarray(body_flags, np.int64) & BF_LARGE) != 0
    nb = min(int(blocks), MAX_BLOCKS)
    own = own_id_block(np.arange(len(b_blk1)), nb) if (own_id_blocks and nb > 0) else np.zeros(len(b_blk1), np.int32)
    return np.where(b_blk1 != 0, b_blk1, np.where(offered != 0, offered, np.where(large, own, 0))).astype(np.int32)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def large_contacts(world, numbers):
    """Which contacts of the world are rows of the large-island solve, from the contact list, the labels (which island is
    which) and the size rule (k_island_classify: an island is small when it has at most SMALL_ISLAND_MAX_JOINTS joints and
    max(bodies, contacts, 1) <= smallMaxW; B2HIP_FORCE_LARGE=1: none is small, = 2: every island is a row group; an island of
    one body without contacts and joints is stepped on its own unless = 2). Returns (is_row [contacts], violations)."""
    v = []
    lab = world.labels
    a, b, solid = world.body_a, world.body_b, world.solid
    nsa, nsb = world.non_static[a], world.non_static[b]
    first = np.where(nsa, a, b)
    live = solid & (nsa | nsb)
    both = live & nsa & nsb
    split = both & (lab[a] != lab[b])
    if split.any():
        i = int(np.flatnonzero(split)[0])
        v.append(Violation("island_label_split", "contact %d" % i, "bodies %d and %d touch but carry labels %d and %d" % (a[i], b[i], lab[a[i]], lab[b[i]])))
    roots = lab[first]
    in_island = live & (roots >= 0)
    n = world.n_bodies
    member = lab >= 0
    n_bodies = np.bincount(lab[member], minlength=n)
    n_contacts = np.bincount(roots[in_island], minlength=n)
    n_joints = np.zeros(n, np.int64)
    for ja, jb in world.joints[:, :2]:
        if ja < 0 or jb < 0 or not (world.active[ja] and world.active[jb]):
            continue
        body = ja if world.non_static[ja] else jb
        if world.non_static[body] and lab[body] >= 0:
            n_joints[lab[body]] += 1
    force = numbers["force_large"]
    w = np.maximum(np.maximum(n_bodies, n_contacts), 1)
    free = (n_bodies == 1) & (n_contacts == 0) & (n_joints == 0) & (force != 2)
    small = (n_joints <= SMALL_ISLAND_MAX_JOINTS) & (w <= numbers["small_max_w"]) & (force == 0)
    is_large = (n_bodies > 0) & ~free & (~small | (force == 2))
    is_row = in_island & is_large[np.maximum(roots, 0)]
    return is_row, is_large, v


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def _or_by_body(n, bodies, bits):
    """OR of `bits` (uint64) over the entries of `bodies` -> [n] uint64."""
    out = np.zeros(n, np.uint64)
    if len(bodies):
        np.bitwise_or.at(out, bodies, bits)
    return out


def check_plan(plan, world):
    """Every violation of the invariants the module's docstring lists, each with the first offending row or body."""
    num, ctr = plan.numbers, plan.counters
    v = []
    exact = num["solver"] == SOLVER_EXACT
    n_rows = plan.n_rows
    nb_all = world.n_bodies
    ns = world.non_static
    lab = world.labels

    def bad(name, where, detail):
        v.append(Violation(name, where, detail))

    # ---- degrees: every solid contact of the world on its non-static bodies
    a, b = world.body_a, world.body_b
    live = world.solid
    deg = np.bincount(a[live & ns[a]], minlength=nb_all) + np.bincount(b[live & ns[b]], minlength=nb_all)
    wrong = ns & (plan.deg != deg)
    if wrong.any():
        i = _first(wrong)
        bad("degree", "body %d" % i, "deg %d, the contact list has %d solid contacts on it" % (plan.deg[i], deg[i]))

    # ---- the row set
    is_row, is_large, lv = large_contacts(world, num)
    v.extend(lv)
    want_rows = int(is_row.sum())
    if n_rows != want_rows:
        bad("row_count", "world", "large_island_contacts %d, the contact list has %d contacts in large islands" % (n_rows, want_rows))
    ref = plan.li_ref.astype(np.int64)
    color = plan.row_color.astype(np.int64)
    if len(ref) != n_rows or len(color) != n_rows:
        bad("row_count", "world", "%d rows / %d colours read for %d rows" % (len(ref), len(color), n_rows))
        return v
    enc_a, enc_b = ref[:, 1], ref[:, 2]
    ra = np.where(enc_a >= 0, enc_a, -(enc_a + 1))
    rb = np.where(enc_b >= 0, enc_b, -(enc_b + 1))
    out_of_range = (ra >= nb_all) | (rb >= nb_all)
    if out_of_range.any():
        i = _first(out_of_range)
        bad("row_set", "row %d" % i, "bodies (%d, %d) of a world of %d" % (ra[i], rb[i], nb_all))
        return v
    # the multiset of (bodyA, bodyB): each contact of the large islands once
    key_rows = np.sort(ra * nb_all + rb)
    key_want = np.sort(a[is_row] * nb_all + b[is_row])
    if len(key_rows) != len(key_want) or (key_rows != key_want).any():
        extra = np.setdiff1d(key_rows, key_want)
        missing = np.setdiff1d(key_want, key_rows)
        uniq, cnt = np.unique(key_rows, return_counts=True)
        uw, cw = np.unique(key_want, return_counts=True)
        twice = [int(k) for k, c in zip(uniq, cnt) if c > dict(zip(uw.tolist(), cw.tolist())).get(int(k), 0)][:1]
        k = int(missing[0]) if len(missing) else (int(extra[0]) if len(extra) else (twice[0] if twice else -1))
        bad("row_set", "bodies (%d, %d)" % (k // nb_all, k % nb_all),
            "%d contacts of the large islands are in no row, %d rows are no such contact, %s" % (len(missing), len(extra), "a contact has more rows than the list has contacts of its bodies" if twice else "counts per pair equal"))
    nsa, nsb = ns[ra], ns[rb]
    wrong = ((enc_a >= 0) != nsa) | ((enc_b >= 0) != nsb)
    if wrong.any():
        i = _first(wrong)
        bad("static_encoding", "row %d" % i, "stored (%d, %d): a static body is -(id + 1), any other its id" % (enc_a[i], enc_b[i]))
    none = ~(nsa | nsb)
    if none.any():
        bad("row_set", "row %d" % _first(none), "a row between two static bodies")
        return v
    first = np.where(nsa, ra, rb)
    wrong = ref[:, 3] != lab[first]
    if wrong.any():
        i = _first(wrong)
        bad("root", "row %d" % i, "root column %d, the label of body %d is %d" % (ref[i, 3], first[i], lab[first[i]]))

    # ---- proper colouring: no non-static body in two rows of one colour (levels in exact-order mode)
    group = (color != HUB_COLOR) | exact
    if (color < 0).any():
        bad("colour_range", "row %d" % _first(color < 0), "colour %d" % color[_first(color < 0)])
        return v
    if not exact and (color >= MAX_COLORS).any():
        bad("colour_range", "row %d" % _first(color >= MAX_COLORS), "colour %d" % color[_first(color >= MAX_COLORS)])
        return v
    ncol = int(color.max()) + 1 if n_rows else 0
    rows = np.arange(n_rows)
    ends = np.concatenate([np.stack([ra, color, rows], 1)[group & nsa], np.stack([rb, color, rows], 1)[group & nsb]])
    if len(ends):
        k = ends[:, 0] * (ncol + 1) + ends[:, 1]
        order = np.argsort(k, kind="stable")
        same = np.flatnonzero(k[order][1:] == k[order][:-1])
        if len(same):
            e0, e1 = ends[order[same[0]]], ends[order[same[0] + 1]]
            bad("colour_clash", "body %d" % e0[0], "rows %d and %d both carry colour %d" % (e0[2], e1[2], e0[1]))

    # ---- layout by colour: order, census, colour count (both modes)
    block_sort = num["block_sort"] != 0
    if not block_sort:
        down = np.flatnonzero(color[1:] < color[:-1])
        if len(down):
            i = int(down[0])
            bad("row_order", "row %d" % (i + 1), "colour %d behind colour %d" % (color[i + 1], color[i]))
        hist = np.bincount(color, minlength=CENSUS_SLOTS)[:CENSUS_SLOTS]
        top = CENSUS_SLOTS if not exact else min(CENSUS_SLOTS, MAX_COLORS)
        wrong = plan.census[:top] != hist[:top]
        if wrong.any():
            c = _first(wrong)
            bad("census", "colour %d" % c, "the census says %d rows, rowColor has %d" % (plan.census[c], hist[c]))
        used = color[group]
        want = int(used.max()) + 1 if len(used) else 0
        # (a row that found no colour free took "colour" 63: the count stands at 64 and the host cuts it to 63, the colours
        # between are skipped by their census - solveLargeIslands, `if (!s.exactLarge && s.nColors > HUB_COLOR)`)
        spilled = not exact and int(ctr["colors"]) == HUB_COLOR and n_rows > 0 and bool((
            (color == HUB_COLOR) & ~(nsa & (plan.deg[ra] > HUB_DEGREE)) & ~(nsb & (plan.deg[rb] > HUB_DEGREE))
            & ~((num["serial_orphans"] != 0) & ((nsa & (plan.eff_blk[ra] == 0)) | (nsb & (plan.eff_blk[rb] == 0))))).any())
        if int(ctr["colors"]) != want and not spilled:
            bad("colour_count", "world", "colors %d, the highest colour in use is %d" % (ctr["colors"], want - 1))
    if exact:
        return v

    # ---- who is swept in order behind the colours, and why
    eff = plan.eff_blk.astype(np.int64)
    blocks = min(max(num["blocks"], 0), MAX_BLOCKS)
    hub_a, hub_b = nsa & (plan.deg[ra] > HUB_DEGREE), nsb & (plan.deg[rb] > HUB_DEGREE)
    by_hub = hub_a | hub_b
    orphan = (num["serial_orphans"] != 0) & ((nsa & (eff[ra] == 0)) | (nsb & (eff[rb] == 0)))
    by_rule = by_hub | orphan
    is63 = color == HUB_COLOR
    cut = nsa & nsb & (eff[ra] != eff[rb]) & (blocks > 0)
    # the colours on every body, by row (for "no permitted colour was free")
    bit = np.where(is63, np.uint64(0), np.uint64(1) << color.astype(np.uint64)).astype(np.uint64)
    on_body = _or_by_body(nb_all, np.concatenate([ra[nsa], rb[nsb]]), np.concatenate([bit[nsa], bit[nsb]]))
    taken = np.where(nsa, on_body[ra], np.uint64(0)) | np.where(nsb, on_body[rb], np.uint64(0))
    tmc = num["test_max_colors"]
    keep = (1 << tmc) - 1 if 0 < tmc < CUT_COLOR_BASE else (1 << CUT_COLOR_BASE) - 1
    lower_ok, upper_ok = np.uint64(keep), np.uint64((keep << CUT_COLOR_BASE) & ((1 << HUB_COLOR) - 1))
    permitted = np.where(cut, upper_ok, lower_ok | upper_ok)
    wrong = by_rule & ~is63
    if wrong.any():
        i = _first(wrong)
        bad("hub_colour", "row %d" % i, "colour %d on a row that is swept in order (%s)" % (color[i], "a hub's" if by_hub[i] else "an orphan"))
    wrong = is63 & ~by_rule & ((permitted & ~taken) != 0)
    if wrong.any():
        i = _first(wrong)
        bad("hub_colour", "row %d" % i, "colour 63 without a hub (degrees %d, %d), without being an orphan, and with a permitted colour free (taken 0x%x)" % (plan.deg[ra[i]], plan.deg[rb[i]], int(taken[i])))

    # ---- classes
    coloured = ~is63 & ~by_rule
    if blocks > 0:
        wrong = coloured & cut & (color < CUT_COLOR_BASE)
        if wrong.any():
            i = _first(wrong)
            bad("cut_row_interior_colour", "row %d" % i, "colour %d, its bodies %d and %d live in blocks %d and %d" % (color[i], ra[i], rb[i], eff[ra[i]], eff[rb[i]]))
        # (an interior row above 32 only where every permitted colour below its own is taken on its bodies - itself aside)
        below = ((np.uint64(1) << color.astype(np.uint64)) - np.uint64(1)) & (lower_ok | upper_ok)
        wrong = coloured & ~cut & (color >= CUT_COLOR_BASE) & ((below & ~taken) != 0)
        if wrong.any():
            i = _first(wrong)
            bad("interior_row_cut_colour", "row %d" % i, "colour %d, its bodies %d and %d share block %d (or one is static) and a lower colour is free" % (color[i], ra[i], rb[i], eff[first[i]]))
    else:
        wrong = coloured & (color >= CUT_COLOR_BASE)
        if wrong.any():
            i = _first(wrong)
            bad("upper_colour_without_partition", "row %d" % i, "colour %d in a world without blocks" % color[i])

    # ---- per-body masks
    ends_body = np.concatenate([ra[nsa], rb[nsb]])
    ends_color = np.concatenate([color[nsa], color[nsb]])
    ends_bit = np.uint64(1) << ends_color.astype(np.uint64)
    upper = (ends_color >= CUT_COLOR_BASE) & (ends_color != HUB_COLOR)
    want_active = _or_by_body(nb_all, ends_body[upper], ends_bit[upper])
    wrong = plan.body_active != want_active
    if wrong.any():
        i = _first(wrong)
        bad("body_active", "body %d" % i, "bodyActive 0x%x, its rows' colours in 32..62 give 0x%x" % (int(plan.body_active[i]), int(want_active[i])))
    rest_first = num["rest_first"] if num["rest_first"] < MAX_COLORS else MAX_COLORS
    rest_on = rest_first < MAX_COLORS
    rest = (ends_color >= rest_first) & (ends_color != HUB_COLOR)
    want_rest = _or_by_body(nb_all, ends_body[rest], ends_bit[rest])
    if rest_on:
        hubs = ends_color == HUB_COLOR
        want_rest |= _or_by_body(nb_all, ends_body[hubs], ends_bit[hubs])
    if not num["safe"]:
        for j in world.joints:
            if j[0] < 0 or j[1] < 0 or not (world.active[j[0]] and world.active[j[1]]):
                continue
            body = j[0] if ns[j[0]] else j[1]
            if ns[body] and lab[body] >= 0 and is_large[lab[body]]:
                for q in j:
                    if q >= 0 and ns[q]:
                        want_rest[q] |= np.uint64(1) << np.uint64(HUB_COLOR)
    wrong = plan.body_rest != want_rest
    if wrong.any():
        i = _first(wrong)
        bad("body_rest", "body %d" % i, "bodyRest 0x%x; with restFirst %s its rows and joints give 0x%x" % (int(plan.body_rest[i]), rest_first if rest_on else "none", int(want_rest[i])))
    col_ends = ends_color != HUB_COLOR
    want_mask = _or_by_body(nb_all, ends_body[col_ends], ends_bit[col_ends])
    hub_body = ns & (plan.deg > HUB_DEGREE)
    wrong = ~hub_body & ((want_mask & ~plan.body_color_mask) != 0)
    if wrong.any():
        i = _first(wrong)
        bad("body_colour_mask", "body %d" % i, "bodyColorMask 0x%x lacks colours of its rows (0x%x)" % (int(plan.body_color_mask[i]), int(want_mask[i])))
    wrong = hub_body & (plan.body_color_mask != 0)
    if wrong.any():
        i = _first(wrong)
        bad("hub_body_colour_mask", "body %d" % i, "bodyColorMask 0x%x on a body of degree %d" % (int(plan.body_color_mask[i]), plan.deg[i]))

    # ---- layout by block
    if block_sort:
        start = plan.blk_row_start.astype(np.int64)
        ok = len(start) == blocks + 1 and blocks > 0
        if not ok:
            bad("block_starts", "world", "%d starts read for %d blocks" % (len(start), blocks))
        elif (np.diff(start) < 0).any() or start[0] != 0:
            k = _first(np.concatenate([[start[0] != 0], np.diff(start) < 0]))
            bad("block_starts", "block %d" % k, "blkRowStart %s" % start[max(0, k - 1):k + 2].tolist())
            ok = False
        if ok:
            owner = eff[first]
            in_blocks = ~is63
            wrong = in_blocks & ((owner < 1) | (owner > blocks))
            if wrong.any():
                i = _first(wrong)
                bad("block_segment", "row %d" % i, "its first non-static body %d has effective block %d of %d" % (first[i], owner[i], blocks))
            else:
                o = np.clip(owner, 1, blocks)
                wrong = in_blocks & ((rows < start[o - 1]) | (rows >= start[o]))
                if wrong.any():
                    i = _first(wrong)
                    bad("block_segment", "row %d" % i, "body %d is home to block %d, whose rows are [%d, %d)" % (first[i], owner[i], start[owner[i] - 1], start[owner[i]]))
            wrong = is63 & (rows < start[blocks])
            if wrong.any():
                i = _first(wrong)
                bad("hub_segment", "row %d" % i, "a row of the hub group in front of %d, where the blocks' rows end" % start[blocks])
            n_cut = int((cut & ~by_rule).sum())
            if int(ctr["cut_constraints"]) != n_cut:
                bad("cut_count", "world", "cut_constraints %d, recounted %d" % (ctr["cut_constraints"], n_cut))
            seg = int(np.diff(start).max())
            if int(ctr["block_max_rows"]) != seg:
                bad("block_max_rows", "world", "block_max_rows %d, the longest segment has %d" % (ctr["block_max_rows"], seg))
        home = plan.b_blk1.astype(np.int64)
        wrong = (home < 0) | (home > blocks)
        if wrong.any():
            i = _first(wrong)
            bad("home_block", "body %d" % i, "b_blk1 %d with %d blocks" % (home[i], blocks))
        wrong = (home != 0) & (home != eff)
        if wrong.any():
            i = _first(wrong)
            bad("home_block", "body %d" % i, "home block %d but effective block %d: a body is home to one block" % (home[i], eff[i]))

    # ---- the hub list
    n_hub = int(is63.sum())
    if n_hub == 0:
        return v
    if num["hub_rows"] != n_hub:
        bad("hub_count", "world", "nHubRows %d, %d rows carry colour 63" % (num["hub_rows"], n_hub))
        return v
    hl = plan.hub_list.astype(np.int64)
    if len(hl) != n_hub or (np.sort(hl) != np.flatnonzero(is63)).any():
        where = "world"
        if len(hl) == n_hub:
            s = np.sort(hl)
            rep = np.flatnonzero(s[1:] == s[:-1])
            where = "row %d" % (s[rep[0]] if len(rep) else hl[_first(~np.isin(hl, np.flatnonzero(is63)))])
        bad("hub_list", where, "hubList[0, %d) is no permutation of the rows with colour 63" % n_hub)
        return v
    ci = ref[hl, 0]
    if not num["hub_wide"]:
        hubs_first = by_hub[hl]
        n_first = int(hubs_first.sum())
        if not hubs_first[:n_first].all():
            bad("hub_list_order", "entry %d" % _first(~hubs_first), "a row without a hub in front of a hub's row")
        else:
            for lo, hi in ((0, n_first), (n_first, n_hub)):
                down = np.flatnonzero(np.diff(ci[lo:hi]) <= 0)
                if len(down):
                    bad("hub_list_order", "entry %d" % (lo + down[0] + 1), "contact %d behind contact %d" % (ci[lo + down[0] + 1], ci[lo + down[0]]))
                    break
        return v
    n_wide = num["hub_wide_rows"]
    hub = num["hub_body"]
    if n_wide < 0 or n_wide > n_hub or (n_wide > 0 and hub < 0):
        bad("wide_count", "world", "nHubWide %d of %d hub rows, primary hub %d" % (n_wide, n_hub, hub))
        return v
    if hub >= 0:
        top = int(plan.deg[ns].max()) if ns.any() else 0
        cand = np.flatnonzero(ns & (plan.deg == top))
        if top <= HUB_DEGREE or num["hub_degree"] != top or hub != int(cand.max()):
            bad("primary_hub", "body %d" % hub, "hubMeta names degree %d; the busiest body is %d with %d" % (num["hub_degree"], int(cand.max()) if len(cand) else -1, top))
    wa, wb = ra[hl], rb[hl]
    wnsa, wnsb = nsa[hl], nsb[hl]
    p_a, p_b = wnsa & (wa == hub), wnsb & (wb == hub)
    one_side = p_a != p_b
    partner = np.where(p_a, wb, wa)
    partner_ns = np.where(p_a, wnsb, wnsa)
    is_wide = np.arange(n_hub) < n_wide
    wrong = is_wide & ~one_side
    if wrong.any():
        k = _first(wrong)
        bad("wide_side", "entry %d (row %d)" % (k, hl[k]), "bodies (%d, %d): the primary hub %d is not on exactly one side" % (wa[k], wb[k], hub))
        return v
    wrong = is_wide & partner_ns & (plan.deg[partner] > HUB_DEGREE)
    if wrong.any():
        k = _first(wrong)
        bad("wide_partner_hub", "entry %d (row %d)" % (k, hl[k]), "partner %d has degree %d" % (partner[k], plan.deg[partner[k]]))
    moving = is_wide & partner_ns
    pw = partner[moving]
    uniq, cnt = np.unique(pw, return_counts=True)
    twice = uniq[cnt > 1]
    if len(twice):
        k = _first(moving & (partner == twice[0]))
        bad("wide_partner_twice", "entry %d (row %d)" % (k, hl[k]), "partner %d has %d rows among the first %d" % (twice[0], cnt[cnt > 1][0], n_wide))
    # each wide row is its partner's row of lowest contact index with the hub (partners with one wide row)
    with_hub = one_side & partner_ns
    lowest = {}
    for k in np.flatnonzero(with_hub):
        lowest[int(partner[k])] = min(lowest.get(int(partner[k]), 1 << 62), int(ci[k]))
    for k in np.flatnonzero(moving & ~np.isin(partner, twice)):
        if int(ci[k]) != lowest[int(partner[k])]:
            bad("wide_not_first", "entry %d (row %d)" % (k, hl[k]), "contact %d; partner %d meets the hub first in contact %d" % (ci[k], partner[k], lowest[int(partner[k])]))
            break
    # ... and every row the fixed point can take is among them
    # (a row of the hub with a static body; a moving partner that is no hub and has none of its rows among the wide ones)
    can = one_side & ~(partner_ns & (plan.deg[partner] > HUB_DEGREE))
    wrong = ~is_wide & can & (~partner_ns | ~np.isin(partner, pw))
    if wrong.any():
        k = _first(wrong)
        bad("wide_count", "entry %d (row %d)" % (k, hl[k]), "a row of the primary hub with %s behind the first %d" % ("partner %d, which has no row among them," % partner[k] if partner_ns[k] else "a static body", n_wide))
    down = np.flatnonzero(np.diff(ci[n_wide:]) <= 0)
    if len(down):
        bad("hub_list_order", "entry %d" % (n_wide + down[0] + 1), "contact %d behind contact %d among the rows behind the wide ones" % (ci[n_wide + down[0] + 1], ci[n_wide + down[0]]))
    return v


def format_violations(violations, limit=12):
    return "\n".join("  %s at %s: %s" % (x.name, x.where, x.detail) for x in violations[:limit]) or "  (none)"
