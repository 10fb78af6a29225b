"""Worlds whose islands have an exact, stable size: for tests that stand an island ON a line of the reference-order tier.

The tier (box2d-mt_amd/csrc/b2d_world.h, b2d_kernels_island.h: k_island_classify, k_island_assign):

    weight of an island   w = max(bodies, solid contacts, 1)        (a contact with the static ground counts)
    tier rule             small if joints <= 64 and w <= smallMaxW  (128; B2HIP_SMALL_MAX_W up to 512), else the coloured solvers
    free                  one body, no contact, no joint: stepped by k_island_classify itself
    chunk rule            lanes = 256 if the largest small island of the step is <= 128, else 1 024;
                          chunkW = max(lanes - largest, lanes / 2); a chunk holds the islands whose weight prefix starts in
                          one window of chunkW, so there are ceil(sum w / chunkW) chunks, or one fewer if no island starts in
                          the last window

Three arrangements, built with plain b2hip.World calls (on any library that exports the C ABI; `Lockstep` makes the same
calls on several worlds at once):

    planks(..)   m dynamic planks side by side on the static ground (gap 0.1), plank k under n_k boxes at pitch 0.5, neighbours
                 tied by a bridging box that rests on both (or by a distance joint). With bridges
                     bodies = m + sum n_k + (m - 1),  solid contacts = sum (n_k + 1) + 2 (m - 1):  contacts > bodies for m > 1.
                 A plank with at most 27 contacts is no hub for the coloured solvers (HUB_DEGREE = 30).
                 One plank alone is n + 1 bodies and n + 1 contacts that all share the plank: a chain of n + 1 dependency
                 levels, the deepest an island of that weight can have (small side only: above 30 boxes the plank is a hub).
                 `riders` welds a box on top of the first boxes of plank 0 (joined bodies do not collide): a body and a joint
                 each, no contact - the only way to bodies > contacts for something that rests on static ground, where every
                 body needs a contact of its own. `rods` are distance joints between neighbouring boxes of a plank.
    chain(..)    nj links on revolute joints, the first to a static body, fixtures in group -1: one island of nj bodies, nj
                 joints and no contact.
    singles(..)  boxes resting on the ground apart from each other: islands of weight 1 (one body, one contact).

Every builder returns an `Island` with what it expects (bodies, contacts, joints) and the ids it made. census() reads what the
islands of the last step WERE from a world's labels and contact list, and expected_counters() applies the rules above to it:
tests/test_tier_worlds_cpu.py holds the builders to their expectation on the oracle, tests/test_gpu_tier_limits.py holds the
device's counters to the oracle's census on every step.
"""
import numpy as np

import b2hip

TINY_MAX_W, SMALL_MAX_W, MAX_JOINTS = 128, 512, 64
TINY_LANES, SMALL_LANES = 256, 1024
HUB_DEGREE = 30
PLANK_MAX_CONTACTS = 27  # what the arrangements keep a plank at where it must not become a hub
BOX, PITCH, GAP = 0.2, 0.5, 0.1
PLANK_Y, BOX_Y = 0.25, 0.7


class Lockstep:
    """The same call on several worlds; what they return (ids) must agree."""

    def __init__(self, *worlds):
        self.worlds = worlds

    def __getattr__(self, name):
        fns = [getattr(w, name) for w in self.worlds]

        def call(*a, **kw):
            out = [f(*a, **kw) for f in fns]
            assert all(o == out[0] for o in out[1:]), "%s returned %s" % (name, out)
            return out[0]
        return call


class Island:
    def __init__(self):
        self.bodies = self.contacts = self.joints = 0
        self.planks, self.boxes, self.bridges, self.riders = [], [], [], []
        self.plank_x, self.plank_hx = [], []
        self.gaps = []          # x of the middle of the gap behind plank k
        self.spare = []         # (x, y) of the free places on the last plank
        self.links, self.rods, self.welds = [], [], []   # joint ids
        self.joint_bodies = {}  # joint id -> (body a, body b)
        self.x_end = 0.0

    @property
    def w(self):
        return max(self.bodies, self.contacts, 1)

    @property
    def expected(self):
        return (self.bodies, self.contacts, self.joints)

    def plank_contacts(self, k):
        """Contacts of plank k as built: its boxes, the ground, the bridges on it."""
        on = len(self.boxes[k]) + 1
        if self.bridges:
            on += (k > 0) + (k < len(self.planks) - 1)
        return on


def ground(w, x_lo, x_hi):
    g = w.create_body(b2hip.STATIC, (0.5 * (x_lo + x_hi), -0.5))
    w.create_fixture(g, b2hip.box_shape(0.5 * (x_hi - x_lo) + 2.0, 0.5))
    return g


def small_box(w, x, y, **kw):
    b = w.create_body(b2hip.DYNAMIC, (x, y), **kw)
    w.create_fixture(b, b2hip.box_shape(BOX, BOX), density=1.0)
    return b


def planks_width(counts, spare=0):
    return sum(2.0 * (0.25 * (n + (spare if k == len(counts) - 1 else 0)) + 0.6) for k, n in enumerate(counts)) + GAP * (len(counts) - 1)


def planks(w, counts, x0=0.0, spare=0, bridges=True, links=False, riders=0, rods=0):
    """Planks with `counts[k]` boxes each from x0 to the right (the ground is the caller's). `spare`: free places on the last
    plank. `bridges` / `links`: neighbours tied by a bridging box / a distance joint."""
    counts = list(counts)
    m = len(counts)
    assert m == 1 or (bridges != links), "several planks are one island through bridges or through links"
    isl = Island()
    x = x0
    for k, n in enumerate(counts):
        slots = n + (spare if k == m - 1 else 0)
        hx = 0.5 * slots * 0.5 + 0.6
        cx = x + hx
        p = w.create_body(b2hip.DYNAMIC, (cx, PLANK_Y))
        w.create_fixture(p, b2hip.box_shape(hx, 0.25), density=1.0)
        isl.planks.append(p)
        isl.plank_x.append(cx)
        isl.plank_hx.append(hx)
        first = cx - 0.25 * (slots - 1)
        isl.boxes.append([small_box(w, first + PITCH * i, BOX_Y) for i in range(n)])
        if k == 0:
            first0 = first
        if k == m - 1:
            isl.spare = [(first + PITCH * i, BOX_Y) for i in range(n, slots)]
        x = cx + hx
        if k < m - 1:
            isl.gaps.append(x + 0.5 * GAP)
            x += GAP
    isl.x_end = x
    if m > 1 and bridges:
        isl.bridges = [small_box(w, gx, BOX_Y) for gx in isl.gaps]
    if m > 1 and links:
        for k in range(m - 1):
            isl.links.append(link_planks(w, isl, k))
    for i in range(riders):
        under = isl.boxes[0][i]
        r = small_box(w, first0 + PITCH * i, BOX_Y + 2.0 * BOX)
        j = w.create_weld_joint(under, r, anchor_a=(0.0, BOX), anchor_b=(0.0, -BOX))
        isl.riders.append(r)
        isl.welds.append(j)
        isl.joint_bodies[j] = (under, r)
    left = rods
    for row in isl.boxes:
        for a, b in zip(row[:-1], row[1:]):
            if left == 0:
                break
            j = w.create_distance_joint(a, b, length=PITCH)
            isl.rods.append(j)
            isl.joint_bodies[j] = (a, b)
            left -= 1
    assert left == 0, "no room for %d rods" % rods
    boxes = sum(counts)
    isl.bodies = m + boxes + len(isl.bridges) + riders
    isl.contacts = boxes + m + 2 * len(isl.bridges)
    isl.joints = len(isl.links) + riders + rods
    return isl


def link_planks(w, isl, k):
    """A distance joint across the gap behind plank k (a new one, for a link that was destroyed)."""
    j = w.create_distance_joint(isl.planks[k], isl.planks[k + 1], anchor_a=(isl.plank_hx[k], 0.0), anchor_b=(-isl.plank_hx[k + 1], 0.0), length=GAP)
    isl.joint_bodies[j] = (isl.planks[k], isl.planks[k + 1])
    return j


def bridged_counts(w_target, last_spare=0):
    """Boxes per plank for a bridged island of `w_target` solid contacts (the larger of its two numbers), no plank above 27
    contacts, `last_spare` of them left free on the last plank."""
    m = 2
    while True:
        boxes = w_target + 2 - 3 * m   # contacts = boxes + m + 2 (m - 1)
        room = (PLANK_MAX_CONTACTS - 3) * m - last_spare - 1  # (the end planks carry one bridge, the last one is left a little lighter)
        if 0 < boxes <= room:
            break
        m += 1
        assert m < 100
    counts = [boxes // m + (1 if k < boxes % m else 0) for k in range(m)]
    # move boxes off the last plank until its spare places fit
    k = 0
    while counts[-1] + 2 + last_spare > PLANK_MAX_CONTACTS:
        if counts[k] + 3 < PLANK_MAX_CONTACTS:
            counts[k] += 1
            counts[-1] -= 1
        k = (k + 1) % (m - 1)
    assert sum(counts) == boxes and max(counts) + 3 <= PLANK_MAX_CONTACTS
    return counts


def single_plank(w, weight, x0=0.0, riders=0):
    """One plank: `weight` bodies in all (riders included), weight - riders contacts."""
    return planks(w, [weight - 1 - riders], x0=x0, riders=riders)


def singles(w, count, x0=0.0, pitch=0.7):
    """`count` boxes resting on the ground, each an island of its own: returns (ids, x behind the last)."""
    ids = [small_box(w, x0 + pitch * i, BOX) for i in range(count)]
    return ids, x0 + pitch * count


def chain(w, nj, x=0.0, y=0.0):
    """A pendulum chain of nj links, stretched out to the right of a static body at (x, y)."""
    isl = Island()
    prev = w.create_body(b2hip.STATIC, (x, y))
    for i in range(nj):
        d = w.create_body(b2hip.DYNAMIC, (x + 0.12 + 0.24 * i, y))
        w.create_fixture(d, b2hip.box_shape(0.12, 0.03), density=1.0, group=-1)
        j = w.create_revolute_joint(prev, d, anchor_a=(0.0, 0.0) if i == 0 else (0.12, 0.0), anchor_b=(-0.12, 0.0))
        isl.joint_bodies[j] = (prev, d)
        isl.links.append(j)
        isl.boxes.append(d)
        prev = d
    isl.bodies, isl.contacts, isl.joints = nj, 0, nj
    return isl


# ---- what the islands of the last step were --------------------------------------------------------------------------------

def census(world, joint_bodies=()):
    """[(bodies, solid contacts, joints)] of the islands the last step solved, largest first. `world` is a b2hip.World on any
    library; `joint_bodies` the (body a, body b) of every live joint."""
    st = world.body_states()
    labels = world.island_labels()
    moving = (st["flags"] & 3) != 0
    c = world.contacts()
    n = len(st)
    nb = np.bincount(labels[labels >= 0], minlength=n)
    solid = (c["flags"] & 3) == 3
    a, b = c["body_a"][solid], c["body_b"][solid]
    of = np.where(moving[a], a, b)
    of = of[moving[of]]
    lab = labels[of]
    nc = np.bincount(lab[lab >= 0], minlength=n)
    nj = np.zeros(n, np.int64)
    for ja, jb in joint_bodies:
        q = ja if moving[ja] else jb
        if moving[q] and labels[q] >= 0:
            nj[labels[q]] += 1
    roots = np.flatnonzero(nb)
    return sorted(((int(nb[r]), int(nc[r]), int(nj[r])) for r in roots), reverse=True)


def chunk_width(largest):
    lanes = TINY_LANES if largest <= TINY_MAX_W else SMALL_LANES
    return max(lanes - largest, lanes // 2), lanes


def expected_counters(islands, small_max_w=TINY_MAX_W, force_large=0):
    """The tier rule and the chunk rule on a census: what b2hip_get_counters must say (solver_chunks as a (low, high) range)."""
    free = [i for i in islands if i == (1, 0, 0) and force_large != 2]
    rest = [i for i in islands if not (i == (1, 0, 0) and force_large != 2)]
    weight = lambda i: max(i[0], i[1], 1)
    small = [i for i in rest if (i[2] <= MAX_JOINTS and weight(i) <= small_max_w and force_large == 0) or force_large == 2]
    large = [i for i in rest if i not in small] if force_large != 2 else list(rest)  # (exact-order mode: all through the large-island solver)
    out = {"islands": len(islands), "free_islands": len(free), "small_islands": len(small), "large_islands": len(large),
           "small_island_bodies": sum(i[0] for i in small), "small_island_contacts": sum(i[1] for i in small)}
    if small:
        cw, lanes = chunk_width(max(weight(i) for i in small))
        total = sum(weight(i) for i in small)
        hi = -(-total // cw)
        out["solver_chunks"] = (max(hi - 1, 1), hi)  # (an island starts in the first window)
        out["chunk_width"], out["chunk_lanes"], out["small_weight"] = cw, lanes, total
    else:
        out["solver_chunks"] = (0, 0)
    return out


# ---- the cases: shared by tests/test_tier_worlds_cpu.py (the oracle alone) and tests/test_gpu_tier_limits.py ------------------
# A case builds its world with build(w), edits it with script(step, w, state) before step `step`, and says with
# pins(step, state) which censuses the step may have: a tuple of allowed lists, or None where the step is in transit (a box in
# the air is about to land). TIME_TO_SLEEP is 0.5 s: a pile that never moves is asleep after 30 steps of 1/60 s.

ASLEEP_AT, WAKE_AT, LINE_STEPS = 30, 45, 100
WIDE = {"B2HIP_SMALL_MAX_W": "512"}
EXACT = {"B2HIP_FORCE_LARGE": "2"}


class Case:
    def __init__(self, name, build, steps, pins, script=None, env=None, sleep=True, small_max_w=TINY_MAX_W):
        self.name, self.build, self.steps, self.pins, self.script = name, build, steps, pins, script
        self.env, self.sleep, self.small_max_w = dict(env or {}), sleep, small_max_w

    def widened(self):
        return Case(self.name + ", tier widened to 512", self.build, self.steps, self.pins, self.script, dict(self.env, **WIDE), self.sleep, SMALL_MAX_W)

    def exact(self):
        return Case(self.name + ", exact-order mode", self.build, self.steps, self.pins, self.script, dict(self.env, **EXACT), self.sleep, self.small_max_w)

    @property
    def force_large(self):
        return int(self.env.get("B2HIP_FORCE_LARGE", "0"))

    def __repr__(self):
        return self.name


class State:
    """What a case's script and pins work on: the islands as built, every live joint's bodies, the destroyed bodies."""

    def __init__(self, islands):
        self.islands = list(islands)
        self.joint_bodies = {}
        for isl in self.islands:
            self.joint_bodies.update(isl.joint_bodies)
        self.dead = []
        self.push = None  # the body the wake-up impulse goes to

    @property
    def expected(self):
        return sorted((isl.expected for isl in self.islands), reverse=True)


def wake_script(step, w, state):
    if step == WAKE_AT:
        # a push along the plank: the box slides a few centimetres and keeps its contact - the island wakes as it is
        w.apply_linear_impulse_to_center(state.push, (0.08, 0.0))


def line_pins(step, state):
    """A pile that rests, falls asleep, is woken at WAKE_AT and falls asleep again."""
    whole = state.expected
    if step < ASLEEP_AT or WAKE_AT <= step < WAKE_AT + ASLEEP_AT:
        return (whole,)
    if step < WAKE_AT:
        return ([],)
    return (whole, [])


def on_planks(counts, **kw):
    def build(w):
        ground(w, 0.0, planks_width(counts))
        isl = planks(w, counts, **kw)
        state = State([isl])
        state.push = isl.boxes[0][-1]
        return state
    return build


def line_case(weight, form, **kw):
    """One island of exactly `weight`: 'one plank' (bodies = contacts, the deepest level chain), 'bridged' (contacts > bodies,
    no hub), 'riders' (bodies > contacts, three weld joints)."""
    if form == "one plank":
        build = on_planks([weight - 1], **kw)
    elif form == "riders":
        build = on_planks([weight - 4], riders=3, **kw)
    else:
        build = on_planks(bridged_counts(weight), **kw)
    return Case("w = %d, %s" % (weight, form), build, LINE_STEPS, line_pins, wake_script)


FORMS = ("one plank", "bridged", "riders")
# (a) on the line, small side; (b) one over it (bridged: no plank is a hub)
SMALL_SIDE = [line_case(w, f) for w in (127, 128) for f in FORMS] + [line_case(w, f).widened() for w in (511, 512) for f in FORMS]
OVER = [line_case(129, "bridged"), line_case(513, "bridged").widened()]
# (c) 64 and 65 joints in an island that is full on the weight line as well
RODS_64, RODS_65 = line_case(128, "bridged", rods=64), line_case(128, "bridged", rods=65)
RODS_64.name, RODS_65.name = "w = 128 with 64 joints", "w = 128 with 65 joints"


def chain_case(nj):
    def build(w):
        return State([chain(w, nj)])
    return Case("chain of %d joints" % nj, build, 100, lambda step, state: (state.expected,))


CHAINS_SMALL, CHAIN_65 = [chain_case(63), chain_case(64)], chain_case(65)


# (d) chunk packing
def archipelago(weights):
    """Separate islands of the given weights on one ground: weight 1 a single box, the others planks (one plank and bridged by turns)."""
    def form(i, wt):
        return [wt - 1] if (wt < 8 or i % 2 == 0) else bridged_counts(wt)

    def build(w):
        width = sum(0.7 if wt == 1 else planks_width(form(i, wt)) for i, wt in enumerate(weights)) + 1.0 * (len(weights) + 1)
        ground(w, 0.0, width)
        x, islands = 1.0, []
        for i, wt in enumerate(weights):
            if wt == 1:
                isl = Island()
                isl.boxes = [[small_box(w, x + 0.35, BOX)]]
                isl.bodies = isl.contacts = 1
                isl.x_end = x + 0.7
            else:
                isl = planks(w, form(i, wt), x0=x)
            assert isl.w == wt
            islands.append(isl)
            x = isl.x_end + 1.0
        return State(islands)
    return build


def resting_pins(step, state):
    return (state.expected,) if step < ASLEEP_AT else ([],)


def drawn_weights(seed, high, count):
    """`count` weights from 1 .. high by seed, two single boxes behind them; every other seed has an island on the line too."""
    weights = np.random.default_rng(seed).integers(1, high + 1, size=count).tolist() + [1, 1]
    return weights + [high] if seed % 2 else weights


CHUNK_STEPS = 36
CHUNKS = [Case("%d islands of 1 .. 128, seed %d" % (40, s), archipelago(drawn_weights(s, 128, 40)), CHUNK_STEPS, resting_pins) for s in (1, 2, 3)]
CHUNKS += [Case("%d islands of 1 .. 512, seed %d" % (12, s), archipelago(drawn_weights(s, 512, 12)), CHUNK_STEPS, resting_pins).widened() for s in (1, 2, 3)]
CHUNKS.append(Case("600 single boxes", archipelago([1] * 600), CHUNK_STEPS, resting_pins))
CHUNKS.append(Case("largest island 129", archipelago([129, 1, 128, 100, 129, 77, 1, 50, 129, 33, 129, 20, 5, 129, 2, 129, 1, 129, 64, 129, 129, 129, 129, 129, 129]),
                   CHUNK_STEPS, resting_pins).widened())


# (e) across the line during a run, both ways
DROP = 0.3  # a box created this far above its place has landed within 20 steps
CROSS_STEPS = 200


def crossing_case(links):
    counts = [25, 25, 25, 26, 20] if links else bridged_counts(126, 6)

    def build(w):
        ground(w, 0.0, planks_width(counts, 6))
        isl = planks(w, counts, spare=6, bridges=not links, links=links)
        # (no plank becomes a hub, the last one with all six boxes that are dropped on it included)
        assert isl.w == 126 and isl.plank_contacts(len(counts) - 1) + 6 <= PLANK_MAX_CONTACTS
        assert max(isl.plank_contacts(k) for k in range(len(counts) - 1)) <= PLANK_MAX_CONTACTS
        state = State([isl])
        state.on = list(counts)           # boxes that have been put on each plank
        state.tied = [True] * (len(counts) - 1)
        return state

    def cut(w, state, k):
        isl = state.islands[0]
        if links:
            w.destroy_joint(isl.links[k])
            del state.joint_bodies[isl.links[k]]
        else:
            w.destroy_body(isl.bridges[k])
            state.dead.append(isl.bridges[k])
        state.tied[k] = False

    def tie(w, state, k):
        isl = state.islands[0]
        if links:
            isl.links[k] = link_planks(w, isl, k)
            state.joint_bodies[isl.links[k]] = isl.joint_bodies[isl.links[k]]
        else:
            isl.bridges[k] = small_box(w, isl.gaps[k], BOX_Y + DROP)
        state.tied[k] = True

    def drop(w, state):
        x, y = state.islands[0].spare[state.on[-1] - counts[-1]]
        small_box(w, x, y + DROP)
        state.on[-1] += 1

    def script(step, w, state):
        if step in (20, 40, 60, 80):
            drop(w, state)              # 127, 128, 129, 130
        elif step in (100, 120):
            cut(w, state, step // 20 - 5)   # the island splits into small ones
        elif step == 140:
            tie(w, state, 0)
            tie(w, state, 1)            # ... and is one again, with the colours and blocks it had
        elif step == 160:
            drop(w, state)
            drop(w, state)
        elif step == 180:
            cut(w, state, len(counts) - 2)

    def pins(step, state):
        if step % 20 != 19:
            return None
        out, k = [], 0
        while k < len(counts):
            e = k
            while e < len(counts) - 1 and state.tied[e]:
                e += 1
            boxes, planks_, ties = sum(state.on[k:e + 1]), e + 1 - k, e - k
            out.append((planks_ + boxes + (0 if links else ties), boxes + planks_ + (0 if links else 2 * ties), ties if links else 0))
            k = e + 1
        return (sorted(out, reverse=True),)

    return Case("126 and up, planks tied by %s" % ("distance joints" if links else "bridging boxes"), build, CROSS_STEPS, pins, script, sleep=False)


CROSSINGS = [crossing_case(False), crossing_case(True)]
ALL_CASES = SMALL_SIDE + OVER + [RODS_64, RODS_65] + CHAINS_SMALL + [CHAIN_65] + CHUNKS + CROSSINGS


def tier_changes(large_per_step):
    """(steps without a large island, steps with one, changes small -> large, changes large -> small)."""
    has = [n > 0 for n in large_per_step]
    up = sum(1 for p, q in zip(has[:-1], has[1:]) if q and not p)
    down = sum(1 for p, q in zip(has[:-1], has[1:]) if p and not q)
    return has.count(False), has.count(True), up, down
