"""The checker of tests/plan_ref.py under test, without a GPU. A synthetic world - a lattice pile of 34 x 8 boxes on a static
ground, a bar of degree > 30 on top of it (the hub: it also leans on a static wall and touches one box twice), one box that no
block has adopted, a small island and a sleeping pair beside the pile - is coloured greedily in numpy, split into blocks by
column, and laid out both ways: rows by block (what k_blocks_sweep reads) and rows by colour, with and without a partition,
with and without rest colours, hub list in either form. The checker returns nothing on these plans.

The corruption table is the mutation evidence of the checker: one thing is broken at a time - at the stage of the plan where
the device would break it, everything downstream rebuilt from the broken state - and the checker must name exactly that
violation, nothing else."""
import os
import re

import numpy as np
import pytest

import plan_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS, LAYERS = 34, 8
GROUND, WALL = 0, 1
FIRST_BOX = 2
BAR = FIRST_BOX + COLS * LAYERS
ORPHAN = FIRST_BOX + COLS * (LAYERS - 1)  # top layer, first column: home to no block in the partitioned plans
TWICE = FIRST_BOX + COLS * (LAYERS - 1) + 5  # the top box the bar touches through two contacts
SMALL0, SMALL1, ASLEEP0, ASLEEP1 = BAR + 1, BAR + 2, BAR + 3, BAR + 4
N_BODIES = BAR + 5
DYNAMIC_AWAKE = 2 | 4 | pr.BF_ACTIVE


def box(layer, col):
    return FIRST_BOX + layer * COLS + col


def synthetic_world():
    """Contacts in a shuffled order (a contact's index says nothing about where it is), a few of them not touching."""
    pairs = []
    for layer in range(LAYERS):
        for col in range(COLS):
            pairs.append((GROUND, box(0, col)) if layer == 0 else (box(layer - 1, col), box(layer, col)))
            if col + 1 < COLS:
                pairs.append((box(layer, col), box(layer, col + 1)))
    pairs += [(BAR, box(LAYERS - 1, col)) for col in range(COLS)]
    pairs += [(BAR, TWICE), (WALL, BAR)]
    pairs += [(GROUND, SMALL0), (SMALL0, SMALL1), (ASLEEP0, ASLEEP1), (GROUND, ASLEEP0)]
    n_solid = len(pairs)
    pairs += [(box(1, c), box(3, c)) for c in range(0, COLS, 3)]  # fat AABBs that overlap, shapes that do not
    rng = np.random.RandomState(11)
    order = rng.permutation(len(pairs))
    a = np.array([pairs[k][0] for k in order])
    b = np.array([pairs[k][1] for k in order])
    solid = order < n_solid
    flags = np.full(N_BODIES, DYNAMIC_AWAKE, np.uint32)
    flags[[GROUND, WALL]] = pr.BT_STATIC | pr.BF_ACTIVE
    flags[[ASLEEP0, ASLEEP1]] = 2 | pr.BF_ACTIVE
    labels = np.full(N_BODIES, FIRST_BOX, np.int32)
    labels[[GROUND, WALL, ASLEEP0, ASLEEP1]] = -1
    labels[[SMALL0, SMALL1]] = SMALL0
    return pr.World(flags, labels, a, b, solid)


def lowest_free(used, lo, hi, per_range=pr.CUT_COLOR_BASE):
    """The lowest colour of [lo, hi) that is not in `used` - of the first `per_range` colours of each range (B2HIP_TEST_MAX_COLORS)."""
    for c in range(lo, hi):
        if not (used >> c) & 1 and c % pr.CUT_COLOR_BASE < per_range:
            return c
    return pr.HUB_COLOR


def build(layout, partition=True, hub_wide=1, rest_first=pr.NO_REST, break_rows=None, test_max_colors=0):
    """The plan of the synthetic world. `break_rows(rows, world, eff)`: called with the coloured row table (dict of arrays a, b,
    ci, root, color) before the masks, the layout and the hub list are made from it."""
    w = synthetic_world()
    ns = w.non_static
    deg = np.bincount(w.body_a[w.solid & ns[w.body_a]], minlength=N_BODIES) + np.bincount(w.body_b[w.solid & ns[w.body_b]], minlength=N_BODIES)
    blocks = 6 if partition else 0
    eff = np.zeros(N_BODIES, np.int32)
    if partition:
        for layer in range(LAYERS):
            for col in range(COLS):
                eff[box(layer, col)] = 1 + col * blocks // COLS
        eff[BAR] = 3
        eff[ORPHAN] = 0
    serial_orphans = 1 if partition else 0
    # rows: the solid contacts of the one large island
    is_row = w.solid & (w.labels[np.where(ns[w.body_a], w.body_a, w.body_b)] == FIRST_BOX)
    ci = np.flatnonzero(is_row)
    ra, rb = w.body_a[ci], w.body_b[ci]
    nsa, nsb = ns[ra], ns[rb]
    by_rule = (nsa & (deg[ra] > pr.HUB_DEGREE)) | (nsb & (deg[rb] > pr.HUB_DEGREE))
    if serial_orphans:
        by_rule |= (nsa & (eff[ra] == 0)) | (nsb & (eff[rb] == 0))
    cut = nsa & nsb & (eff[ra] != eff[rb]) & partition
    color = np.full(len(ci), pr.HUB_COLOR)
    used = [0] * N_BODIES
    for k in range(len(ci)):
        if by_rule[k]:
            continue
        u = (used[ra[k]] if nsa[k] else 0) | (used[rb[k]] if nsb[k] else 0)
        per_range = test_max_colors if test_max_colors else pr.CUT_COLOR_BASE
        c = lowest_free(u, pr.CUT_COLOR_BASE if cut[k] else 0, pr.HUB_COLOR, per_range)
        if c == pr.HUB_COLOR:  # (no permitted colour free: swept in order with the hub rows, reserves nothing)
            continue
        color[k] = c
        for body, moving in ((ra[k], nsa[k]), (rb[k], nsb[k])):
            if moving:
                used[body] |= 1 << c
    rows = dict(a=ra.copy(), b=rb.copy(), ci=ci.copy(), root=np.full(len(ci), FIRST_BOX), color=color)
    if break_rows is not None:
        break_rows(rows, w, eff)
    ra, rb, ci, color = rows["a"], rows["b"], rows["ci"], rows["color"]
    nsa, nsb = ns[ra], ns[rb]
    first = np.where(nsa, ra, rb)
    is63 = color == pr.HUB_COLOR
    # masks
    mask, active, rest = (np.zeros(N_BODIES, np.uint64) for _ in range(3))
    rf = min(rest_first, pr.MAX_COLORS)
    for k in range(len(ci)):
        for body, moving in ((ra[k], nsa[k]), (rb[k], nsb[k])):
            if not moving:
                continue
            bit = np.uint64(1) << np.uint64(color[k])
            if not is63[k]:
                if deg[body] <= pr.HUB_DEGREE:
                    mask[body] |= bit
                if color[k] >= pr.CUT_COLOR_BASE:
                    active[body] |= bit
                if color[k] >= rf:
                    rest[body] |= bit
            elif rf < pr.MAX_COLORS:
                rest[body] |= bit
    # layout (the places inside a group are whatever the atomics gave: shuffled)
    rng = np.random.RandomState(5)
    shuffle = rng.permutation(len(ci))
    blk_row_start = np.zeros(blocks + 1, np.int32)
    if layout == "block":
        group = np.where(is63, blocks, eff[first] - 1)
        assert (group >= 0).all()
        blk_row_start[1:] = np.cumsum(np.bincount(group[~is63], minlength=blocks))[:blocks]
    else:
        group = color
    place = shuffle[np.argsort(group[shuffle], kind="stable")]
    li_ref = np.stack([ci, np.where(nsa, ra, -(ra + 1)), np.where(nsb, rb, -(rb + 1)), rows["root"]], 1)[place].astype(np.int32)
    row_color = color[place].astype(np.int32)
    # hub list: row indices; wide rows first (the primary hub with a static body, or with a moving partner's first contact)
    hub_rows = np.flatnonzero(row_color == pr.HUB_COLOR)
    la, lb, lci = ra[place][hub_rows], rb[place][hub_rows], ci[place][hub_rows]
    has_hub = (ns[la] & (deg[la] > pr.HUB_DEGREE)) | (ns[lb] & (deg[lb] > pr.HUB_DEGREE))
    if hub_wide:
        partner = np.where(la == BAR, lb, la)
        one_side = (la == BAR) != (lb == BAR)
        lowest = {}
        for k in np.flatnonzero(one_side & ns[partner]):
            lowest[partner[k]] = min(lowest.get(partner[k], 1 << 60), lci[k])
        wide = np.array([one_side[k] and (not ns[partner[k]] or lci[k] == lowest[partner[k]]) for k in range(len(hub_rows))], bool)
        top = np.array([int(mask[p]).bit_length() if ns[p] else 0 for p in partner])
        order = np.lexsort((lci, np.where(wide, top, 0), ~wide))
        n_wide = int(wide.sum())
    else:
        order = np.lexsort((lci, ~has_hub))
        n_wide = 0
    hub_list = hub_rows[order].astype(np.int32)
    coloured = color[~is63]
    by_rule_now = (nsa & (deg[ra] > pr.HUB_DEGREE)) | (nsb & (deg[rb] > pr.HUB_DEGREE))
    if serial_orphans:
        by_rule_now |= (nsa & (eff[ra] == 0)) | (nsb & (eff[rb] == 0))
    # (a row that found no colour leaves the count at 64, which the host cuts to 63)
    n_colors = pr.HUB_COLOR if (is63 & ~by_rule_now).any() else int(coloured.max()) + 1
    numbers = dict.fromkeys(pr.PLAN_FIELDS, 0)
    numbers.update(passes=1, solver=pr.SOLVER_SWEEP if layout == "block" else pr.SOLVER_LAUNCHES, rest_first=rest_first,
                   use_rest=int(rf < pr.MAX_COLORS), block_sort=int(layout == "block"), hub_wide=hub_wide, serial_orphans=serial_orphans,
                   has_hubs=1, hub_rows=len(hub_rows), hub_wide_rows=n_wide, hub_body=BAR, hub_degree=int(deg[BAR]), blocks=blocks,
                   colors=n_colors, max_degree=int(deg.max()), small_max_w=pr.TINY_ISLAND_MAX_W, test_max_colors=test_max_colors)
    counters = dict(large_island_contacts=len(ci), colors=n_colors, blocks=blocks,
                    cut_constraints=int((nsa & nsb & (eff[ra] != eff[rb]) & partition & ~by_rule_now).sum()),
                    block_max_rows=int(np.diff(blk_row_start).max()) if layout == "block" else 0)
    plan = pr.Plan(numbers, counters, li_ref=li_ref, row_color=row_color, deg=deg.astype(np.int32), body_color_mask=mask, body_active=active,
                   body_rest=rest, b_blk1=eff.copy(), eff_blk=eff, blk_row_start=blk_row_start,
                   census=np.bincount(color, minlength=pr.CENSUS_SLOTS)[:pr.CENSUS_SLOTS].astype(np.int32), hub_list=hub_list)
    return plan, w


VARIANTS = {"rows by block": dict(layout="block"),
            "rows by colour, partition kept, rest colours": dict(layout="colour", rest_first=2),
            "rows by colour, no partition, hub rows in contact order": dict(layout="colour", partition=False, hub_wide=0),
            "rows by colour, no partition, rest colours": dict(layout="colour", partition=False, rest_first=3),
            # B2HIP_TEST_MAX_COLORS=2: rows without a free colour in the hub group, interior rows in the upper range
            "rows by colour, two colours per range": dict(layout="colour", test_max_colors=2)}


def names(plan, world):
    return sorted({x.name for x in pr.check_plan(plan, world)})


def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, "box2d-mt_amd", "csrc", "b2d_world.h")).read()
    for name in ("MAX_COLORS", "HUB_DEGREE", "CUT_COLOR_BASE", "MAX_BLOCKS", "SMALL_ISLAND_MAX_JOINTS", "TINY_ISLAND_MAX_W"):
        m = re.search(r"^#define %s (\d+)" % name, text, re.M)
        assert m and int(m.group(1)) == getattr(pr, name), name
    assert re.search(r"^#define HUB_COLOR \(MAX_COLORS - 1\)", text, re.M) and pr.HUB_COLOR == 63
    for name, value in (("BF_TYPE_MASK", pr.BF_TYPE_MASK), ("BF_ACTIVE", pr.BF_ACTIVE), ("BF_LARGE", pr.BF_LARGE)):
        m = re.search(r"^#define %s 0x([0-9a-f]+)u" % name, text, re.M)
        assert m and int(m.group(1), 16) == value, name
    # the fields of b2hip_debug_read 27 as its comment counts them
    api = open(os.path.join(ROOT, "box2d-mt_amd", "csrc", "b2hip_api_callbacks.h")).read()
    assert "const int N = %d;" % len(pr.PLAN_FIELDS) in api


def test_own_id_block_is_the_integer_remainder():
    from test_gpu_device_math import _own_id_block_expected
    ids = np.concatenate([np.arange(0, 2000000, 1009), [0xc1f9f3 * 0 + 622]]).astype(np.int32)
    every = np.arange(2000000, dtype=np.int64)
    top = every[(((every * 2654435761) & 0xffffffff) >> 8) >= 0xfff000].astype(np.int32)  # where the float quotient rounds up
    for part in (ids, top[:3000]):
        want = _own_id_block_expected(part, 1024)
        got = pr.own_id_block(part[:, None], np.arange(1, 1025)[None, :])
        assert (got == want).all()
    # effBlk from its ingredients: home block, else the offer's low 11 bits, else the own-id block of a large island's body
    flags = np.array([pr.BF_LARGE, pr.BF_LARGE, pr.BF_LARGE, 0], np.uint32)
    e = pr.eff_blk_from([4, 0, 0, 0], [0, (123 << 11) | 7, 0, 0], flags, 11, True)
    assert e.tolist() == [4, 7, int(pr.own_id_block(2, 11)), 0]
    assert pr.eff_blk_from([4, 0, 0, 0], [0, 0, 0, 0], flags, 11, False).tolist() == [4, 0, 0, 0]


@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS))
def test_clean_plans_pass(variant):
    plan, world = build(**VARIANTS[variant])
    found = pr.check_plan(plan, world)
    assert not found, pr.format_violations(found)
    # the plans are what their names say
    color = plan.row_color
    assert plan.n_rows > 500 and plan.deg[BAR] > pr.HUB_DEGREE and (color == pr.HUB_COLOR).sum() >= plan.deg[BAR]
    if plan.numbers["test_max_colors"]:
        assert (color == pr.HUB_COLOR).sum() > plan.deg[BAR] + 20 and plan.counters["colors"] == pr.HUB_COLOR
        assert set(np.unique(color)) == {0, 1, 32, 33, 63}
    if VARIANTS[variant].get("partition", True):
        assert ((color >= pr.CUT_COLOR_BASE) & (color != pr.HUB_COLOR)).sum() > 20 and plan.counters["cut_constraints"] > 20
    else:
        assert not ((color >= pr.CUT_COLOR_BASE) & (color != pr.HUB_COLOR)).any()
    if plan.numbers["hub_wide"]:
        assert plan.numbers["hub_wide_rows"] == COLS + 1 and plan.numbers["hub_rows"] > plan.numbers["hub_wide_rows"]
    if plan.numbers["use_rest"]:
        assert (plan.body_rest != 0).sum() > 100 and (plan.body_rest >> np.uint64(63)).sum() >= COLS


def test_the_reference_counts_islands_itself():
    """Which islands are large follows from the contact list, the labels and the size rule - and B2HIP_FORCE_LARGE."""
    plan, world = build("colour", partition=False, hub_wide=0)
    is_row, is_large, v = pr.large_contacts(world, plan.numbers)
    assert not v and is_row.sum() == plan.n_rows and is_large[FIRST_BOX] and not is_large[SMALL0]
    forced = dict(plan.numbers, force_large=1)
    is_row1, is_large1, _ = pr.large_contacts(world, forced)
    assert is_large1[SMALL0] and is_row1.sum() == plan.n_rows + 2  # (the small island's two contacts; the sleeping pair stays out)
    assert "row_count" in names(pr.Plan(forced, plan.counters, **{k: getattr(plan, k) for k in pr.Plan.ARRAYS}), world)
    # 65 joints make the small island a large one
    world.joints = np.array([[SMALL0, SMALL1, -1, -1]] * 65)
    assert pr.large_contacts(world, plan.numbers)[1][SMALL0]
    world.joints = np.array([[SMALL0, SMALL1, -1, -1]] * 64)
    assert not pr.large_contacts(world, plan.numbers)[1][SMALL0]


# ---- the corruption table ---------------------------------------------------------------------------------------------------------
def on_body(rows, world, body, skip=-1):
    m = 0
    for k in np.flatnonzero(((rows["a"] == body) | (rows["b"] == body))):
        if k != skip and rows["color"][k] != pr.HUB_COLOR and world.non_static[body]:
            m |= 1 << int(rows["color"][k])
    return m


def plain_rows(rows, world, eff, want_cut):
    """Rows that are neither a hub's nor an orphan's, of the class asked for."""
    ns = world.non_static
    out = []
    for k in range(len(rows["a"])):
        a, b = rows["a"][k], rows["b"][k]
        if rows["color"][k] == pr.HUB_COLOR or BAR in (a, b) or ORPHAN in (a, b):
            continue
        cut = ns[a] and ns[b] and eff[a] != eff[b]
        if cut == want_cut:
            out.append(k)
    return out


def duplicate_colour_on_one_body(rows, world, eff):
    for r1 in plain_rows(rows, world, eff, False):
        for r2 in plain_rows(rows, world, eff, False):
            shared = {rows["a"][r1], rows["b"][r1]} & {rows["a"][r2], rows["b"][r2]}
            if r1 != r2 and any(world.non_static[x] for x in shared):
                rows["color"][r2] = rows["color"][r1]
                return
    raise AssertionError("no two interior rows share a body")


def drop_one_row_duplicate_another(rows, world, eff):
    """Row i becomes a second row of contact j (the count stays): with i's colour, which j's bodies do not hold yet, and of j's class."""
    cand = plain_rows(rows, world, eff, False)
    for i in cand:
        for j in cand:
            c = int(rows["color"][i])
            if i != j and not ((on_body(rows, world, rows["a"][j]) | on_body(rows, world, rows["b"][j])) >> c) & 1:
                for f in ("a", "b", "ci", "root"):
                    rows[f][i] = rows[f][j]
                return
    raise AssertionError("no pair of rows fits")


def recolour(want_cut, lo, hi):
    def go(rows, world, eff):
        for k in plain_rows(rows, world, eff, want_cut):
            used = on_body(rows, world, rows["a"][k], k) | on_body(rows, world, rows["b"][k], k)
            c = lowest_free(used, lo, hi)
            if c != pr.HUB_COLOR:
                rows["color"][k] = c
                return
        raise AssertionError("no row fits")
    return go


def colours_of(rows, body):
    return {int(c) for c in rows["color"][(rows["a"] == body) | (rows["b"] == body)]}


def coloured_row_into_the_hub_group(rows, world, eff):
    """Two colours per range: a row whose bodies hold no row without a colour gives its colour up - so one IS free for it."""
    for k in plain_rows(rows, world, eff, False):
        moving = [x for x in (rows["a"][k], rows["b"][k]) if world.non_static[x]]
        if all(pr.HUB_COLOR not in colours_of(rows, x) for x in moving):
            rows["color"][k] = pr.HUB_COLOR
            return
    raise AssertionError("no row fits")


def interior_row_up_although_a_lower_colour_is_free(rows, world, eff):
    for k in plain_rows(rows, world, eff, False):
        moving = [x for x in (rows["a"][k], rows["b"][k]) if world.non_static[x]]
        if rows["color"][k] == 0 and all(not ({32, pr.HUB_COLOR} & colours_of(rows, x)) for x in moving):
            rows["color"][k] = 32
            return
    raise AssertionError("no row fits")


def hub_row_gets_colour_12(rows, world, eff):
    for k in range(len(rows["a"])):
        a, b = rows["a"][k], rows["b"][k]
        if a == BAR and world.non_static[b] and b != ORPHAN and not (on_body(rows, world, b) >> 12) & 1:
            rows["color"][k] = 12
            return
    raise AssertionError("no hub row fits")


def clear_rest_bit_on_b_side(plan, world):
    for p in range(plan.n_rows):
        c, b = plan.row_color[p], plan.li_ref[p, 2]
        if plan.li_ref[p, 1] >= 0 and b >= 0 and c != pr.HUB_COLOR and c >= plan.numbers["rest_first"]:
            plan.body_rest[b] &= ~(np.uint64(1) << np.uint64(c))
            return
    raise AssertionError("no rest row with two moving bodies")


def one_active_bit_too_many(plan, world):
    plan.body_active[box(2, 7)] |= np.uint64(1) << np.uint64(40)


def repeat_a_hub_list_entry(plan, world):
    plan.hub_list[-1] = plan.hub_list[-2]


def rows_of_the_twice_touched_box(plan):
    """(entry of the first contact, entry of the second) of the bar with the box it touches twice, in hubList."""
    at = [k for k, row in enumerate(plan.hub_list) if set(plan.li_ref[row, 1:3]) == {BAR, TWICE}]
    assert len(at) == 2 and at[0] < plan.numbers["hub_wide_rows"] <= at[1]
    return at


def second_row_of_a_partner_made_wide(plan, world):
    first, second = rows_of_the_twice_touched_box(plan)
    n_wide = plan.numbers["hub_wide_rows"]
    hl = plan.hub_list.tolist()
    row = hl.pop(second)
    hl.insert(n_wide, row)
    plan.hub_list[:] = hl
    plan.numbers["hub_wide_rows"] = n_wide + 1


def later_row_of_a_partner_in_place_of_its_first(plan, world):
    first, second = rows_of_the_twice_touched_box(plan)
    n_wide = plan.numbers["hub_wide_rows"]
    hl = plan.hub_list.tolist()
    hl[first], hl[second] = hl[second], hl[first]
    # (the rows behind the wide ones stay in ascending contact index)
    tail = sorted(hl[n_wide:], key=lambda row: plan.li_ref[row, 0])
    plan.hub_list[:] = hl[:n_wide] + tail


def swap_two_rows_across_a_colour_boundary(plan, world):
    c = plan.row_color
    p = next(p for p in range(plan.n_rows - 1) if c[p] < c[p + 1] and c[p + 1] != pr.HUB_COLOR)
    plan.li_ref[[p, p + 1]] = plan.li_ref[[p + 1, p]]
    plan.row_color[[p, p + 1]] = plan.row_color[[p + 1, p]]


def static_body_stored_with_its_id(plan, world):
    p = next(p for p in range(plan.n_rows) if plan.li_ref[p, 1] < 0)
    plan.li_ref[p, 1] = -(plan.li_ref[p, 1] + 1)


def wrong_root(plan, world):
    plan.li_ref[plan.n_rows // 2, 3] = SMALL0


def swap_two_rows_across_a_block_boundary(plan, world):
    p = int(plan.blk_row_start[2])
    plan.li_ref[[p - 1, p]] = plan.li_ref[[p, p - 1]]
    plan.row_color[[p - 1, p]] = plan.row_color[[p, p - 1]]


def hub_row_in_a_block_segment(plan, world):
    # (the last block's segment reaches one row into the hub group's; the census that goes with it says the same)
    plan.blk_row_start[-1] += 1
    plan.counters["block_max_rows"] = int(np.diff(plan.blk_row_start).max())


def one_degree_off(plan, world):
    plan.deg[box(3, 3)] += 1


def census_off_by_one(plan, world):
    plan.census[1] -= 1


def colour_mask_lacks_a_row(plan, world):
    body = box(4, 9)
    plan.body_color_mask[body] &= plan.body_color_mask[body] - np.uint64(1)  # (its lowest colour goes)


def hub_with_a_colour_mask(plan, world):
    plan.body_color_mask[BAR] = np.uint64(1)


def hub_rows_out_of_contact_order(plan, world):
    plan.hub_list[[3, 4]] = plan.hub_list[[4, 3]]


def block_starts_not_monotone(plan, world):
    plan.blk_row_start[3] = plan.blk_row_start[2] - 1


BLOCK, BLOCK_COLOUR = VARIANTS["rows by block"], VARIANTS["rows by colour, partition kept, rest colours"]
SPILL = VARIANTS["rows by colour, two colours per range"]
PLAIN, PLAIN_REST = VARIANTS["rows by colour, no partition, hub rows in contact order"], VARIANTS["rows by colour, no partition, rest colours"]
# name of the corruption, the plan it is made in, where it is made (break_rows: in the coloured row table, before masks and
# layout; break_plan: in the finished tables), the ONE violation the checker must name
CORRUPTIONS = [
    ("a duplicated colour on one body (rows by block)", BLOCK, "rows", duplicate_colour_on_one_body, "colour_clash"),
    ("a duplicated colour on one body (rows by colour)", PLAIN, "rows", duplicate_colour_on_one_body, "colour_clash"),
    ("a row dropped and another duplicated, the count unchanged (rows by block)", BLOCK, "rows", drop_one_row_duplicate_another, "row_set"),
    ("a row dropped and another duplicated, the count unchanged (rows by colour)", PLAIN_REST, "rows", drop_one_row_duplicate_another, "row_set"),
    ("an interior colour on a cut row", BLOCK, "rows", recolour(True, 0, pr.CUT_COLOR_BASE), "cut_row_interior_colour"),
    ("an interior colour on a cut row (rows by colour)", BLOCK_COLOUR, "rows", recolour(True, 0, pr.CUT_COLOR_BASE), "cut_row_interior_colour"),
    ("a cut colour on an interior row", BLOCK, "rows", recolour(False, pr.CUT_COLOR_BASE, pr.HUB_COLOR), "interior_row_cut_colour"),
    ("an upper colour in a world without blocks", PLAIN, "rows", recolour(False, pr.CUT_COLOR_BASE, pr.HUB_COLOR), "upper_colour_without_partition"),
    ("one missing bodyRest bit on the B side only", PLAIN_REST, "plan", clear_rest_bit_on_b_side, "body_rest"),
    ("one missing bodyRest bit on the B side only (partition kept)", BLOCK_COLOUR, "plan", clear_rest_bit_on_b_side, "body_rest"),
    ("a bodyActive bit too many", BLOCK, "plan", one_active_bit_too_many, "body_active"),
    ("a hub row with colour 12 (rows by block)", BLOCK, "rows", hub_row_gets_colour_12, "hub_colour"),
    ("a hub row with colour 12 (rows by colour)", PLAIN, "rows", hub_row_gets_colour_12, "hub_colour"),
    ("a hubList with one entry repeated", BLOCK, "plan", repeat_a_hub_list_entry, "hub_list"),
    ("a hubList with one entry repeated (contact order)", PLAIN, "plan", repeat_a_hub_list_entry, "hub_list"),
    ("two wide rows with the same partner", BLOCK, "plan", second_row_of_a_partner_made_wide, "wide_partner_twice"),
    ("a wide row that is not its partner's first with the hub", PLAIN_REST, "plan", later_row_of_a_partner_in_place_of_its_first, "wide_not_first"),
    ("rowColor out of order by one swap", PLAIN, "plan", swap_two_rows_across_a_colour_boundary, "row_order"),
    ("a static body stored with a non-negative id", BLOCK, "plan", static_body_stored_with_its_id, "static_encoding"),
    ("a wrong root", PLAIN, "plan", wrong_root, "root"),
    # beyond the issue's table
    ("a row in the hub group although a permitted colour is free", SPILL, "rows", coloured_row_into_the_hub_group, "hub_colour"),
    ("an interior row in the upper range although a lower colour is free", SPILL, "rows", interior_row_up_although_a_lower_colour_is_free, "interior_row_cut_colour"),
    ("two rows swapped across a block boundary", BLOCK, "plan", swap_two_rows_across_a_block_boundary, "block_segment"),
    ("a hub row inside a block's segment", BLOCK, "plan", hub_row_in_a_block_segment, "hub_segment"),
    ("a degree one too high", PLAIN, "plan", one_degree_off, "degree"),
    ("a census one too low", PLAIN, "plan", census_off_by_one, "census"),
    ("a bodyColorMask that lacks a row's colour", BLOCK, "plan", colour_mask_lacks_a_row, "body_colour_mask"),
    ("a colour mask on a hub", PLAIN, "plan", hub_with_a_colour_mask, "hub_body_colour_mask"),
    ("hub rows out of contact order", PLAIN, "plan", hub_rows_out_of_contact_order, "hub_list_order"),
    ("block starts that go down", BLOCK, "plan", block_starts_not_monotone, "block_starts"),
]


@pytest.mark.parametrize("case", CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_every_corruption_is_named_and_nothing_else(case):
    what, variant, stage, corrupt, want = case
    if stage == "rows":
        plan, world = build(break_rows=corrupt, **variant)
    else:
        plan, world = build(**variant)
        corrupt(plan, world)
    found = pr.check_plan(plan, world)
    assert sorted({x.name for x in found}) == [want], "%s:\n%s" % (what, pr.format_violations(found))
    assert all(x.where for x in found)


def test_exact_order_plans_are_checked_by_level():
    """Exact-order mode: the colour is the dependency level (thousands), colour 63 is a level like any other, no classes, no
    masks; proper per level, rows by level, census of the first levels."""
    world = synthetic_world()
    ns = world.non_static
    numbers = dict.fromkeys(pr.PLAN_FIELDS, 0)
    numbers.update(passes=1, solver=pr.SOLVER_EXACT, rest_first=pr.NO_REST, force_large=2, small_max_w=pr.TINY_ISLAND_MAX_W, hub_body=-1)
    is_row, _, _ = pr.large_contacts(world, numbers)
    ci = np.flatnonzero(is_row)
    ra, rb = world.body_a[ci], world.body_b[ci]
    last = np.zeros(N_BODIES, np.int64)
    level = np.zeros(len(ci), np.int64)
    # (k_island_dfs: level = 1 + the highest level on either body so far; walked body by body here, which chains the rows of a
    # layer and of the layers above it: more levels than colours)
    for k in np.lexsort((-np.minimum(ra, rb), np.maximum(ra, rb))):
        level[k] = 1 + max(last[ra[k]] if ns[ra[k]] else 0, last[rb[k]] if ns[rb[k]] else 0)
        for body in (ra[k], rb[k]):
            if ns[body]:
                last[body] = level[k]
    color = level - 1
    assert color.max() > pr.MAX_COLORS
    place = np.argsort(color, kind="stable")
    first = np.where(ns[ra], ra, rb)
    li_ref = np.stack([ci, np.where(ns[ra], ra, -(ra + 1)), np.where(ns[rb], rb, -(rb + 1)), world.labels[first]], 1)[place].astype(np.int32)
    deg = np.bincount(world.body_a[world.solid & ns[world.body_a]], minlength=N_BODIES) + np.bincount(world.body_b[world.solid & ns[world.body_b]], minlength=N_BODIES)
    zeros = np.zeros(N_BODIES, np.uint64)
    plan = pr.Plan(numbers, dict(large_island_contacts=len(ci), colors=int(color.max()) + 1, blocks=0, cut_constraints=0, block_max_rows=0),
                   li_ref=li_ref, row_color=color[place].astype(np.int32), deg=deg.astype(np.int32), body_color_mask=zeros, body_active=zeros, body_rest=zeros,
                   b_blk1=np.zeros(N_BODIES, np.int32), eff_blk=np.zeros(N_BODIES, np.int32), blk_row_start=np.zeros(1, np.int32),
                   census=np.bincount(color, minlength=pr.CENSUS_SLOTS)[:pr.CENSUS_SLOTS].astype(np.int32), hub_list=np.zeros(0, np.int32))
    assert (plan.row_color == pr.HUB_COLOR).any()
    found = pr.check_plan(plan, world)
    assert not found, pr.format_violations(found)
    # a row one level too low shares the level with the row it depends on
    broken = plan.copy()
    p = int(np.flatnonzero(broken.row_color == 70)[0])
    broken.row_color[p] = 69
    assert "colour_clash" in names(broken, world)
