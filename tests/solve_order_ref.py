"""From the device's large-island PLAN to the order the sequential sweep must visit the contacts in (numpy only).

The coloured large-island solvers - k_solve_blocks, k_blocks_sweep, the launch-per-colour kernels with k_large_warm /
k_large_rest / k_rest_hub / k_sweep_end / k_large_hub - are, by the parity contract (docs/SOLVER_LARGE_ISLANDS.md), ONE
sequential Gauss-Seidel sweep: "interior colours ascending, then cut colours, then hub constraints, on every body". Two rows
of one colour share no moving body (plan_ref.check_plan: colour_clash), so the order inside a colour cannot be observed, and
the whole sweep is fixed by a rank per row:

    a row of colour c < 63          rank c
    a row of the hub group (63)     63 + its place in hubList[0, nHubRows)
    body flag                       BF_LARGE of DW::b_flags, as plan_ref reads it

    entries, large = solve_order(plan, contacts, body_flags)

`plan` is what plan_ref.read_plan returns, `contacts` the b2hip_get_contacts list read at the same point (li_ref's first
column indexes it), `body_flags` b2hip_debug_read 4. `entries` (ORDER_DTYPE: fixture_a, fixture_b, rank) and `large` (one byte
per body) are what the oracle's b2o_set_solve_order takes: contacts are named by their fixture ids - at the C ABI a chain's
child edge is a fixture of its own, so the pair names a contact - never by array index. Joints carry no rank: a large
island's joints are walked in ascending joint id (k_joints_fill / k_joints_sort), which is the hook's joint rule.

Nothing of the device but the plan goes in. A kernel that depended on a further ordering fact would show as differing bits in
tests/test_gpu_solve_replay.py; the fact would then belong into the parity contract with the kernel line that establishes it,
and into this rule with that citation - not silently into the replay.
"""
import numpy as np

import plan_ref as pr

ORDER_DTYPE = np.dtype([("fixture_a", "<i4"), ("fixture_b", "<i4"), ("rank", "<i4")])


class PlanMismatch(ValueError):
    """The plan and the contact list do not describe the same rows (the order cannot be derived: nothing is guessed)."""


def row_ranks(plan):
    """rank per row of the plan: the colour, or 63 + the place in the hub list for the rows of the hub group."""
    n_rows = plan.n_rows
    color = np.asarray(plan.row_color, np.int64)[:n_rows]
    if plan.numbers["solver"] == pr.SOLVER_EXACT:
        raise PlanMismatch("exact-order mode sweeps levels of the reference's order, not colours")
    if len(color) != n_rows or (color < 0).any() or (color > pr.HUB_COLOR).any():
        raise PlanMismatch("rowColor: %d colours for %d rows, range [%s, %s]" % (len(color), n_rows, color.min() if len(color) else "-", color.max() if len(color) else "-"))
    rank = color.copy()
    hub_rows = np.flatnonzero(color == pr.HUB_COLOR)
    if len(hub_rows):
        n_hub = int(plan.numbers["hub_rows"])
        hl = np.asarray(plan.hub_list, np.int64)[:n_hub]
        if n_hub != len(hub_rows) or len(hl) != n_hub or (np.sort(hl) != hub_rows).any():
            raise PlanMismatch("hubList[0, %d) is no permutation of the %d rows of colour 63" % (n_hub, len(hub_rows)))
        rank[hl] = pr.HUB_COLOR + np.arange(n_hub)
    return rank


def solve_order(plan, contacts, body_flags):
    """(entries, large) for b2o_set_solve_order from a plan, the contact list it indexes and the body flags."""
    body_flags = np.asarray(body_flags, np.uint32)
    large = ((body_flags & pr.BF_LARGE) != 0).astype(np.uint8)
    n_rows = plan.n_rows
    entries = np.zeros(n_rows, ORDER_DTYPE)
    if n_rows == 0:
        return entries, large
    ref = np.asarray(plan.li_ref, np.int64).reshape(-1, 4)[:n_rows]
    ci = ref[:, 0]
    if len(ref) != n_rows or (ci < 0).any() or (ci >= len(contacts)).any():
        raise PlanMismatch("li_ref names contacts outside the list of %d" % len(contacts))
    if len(np.unique(ci)) != n_rows:
        raise PlanMismatch("a contact has two rows")
    # the row's bodies are the contact's (a static body is stored as -(id + 1))
    ra = np.where(ref[:, 1] >= 0, ref[:, 1], -(ref[:, 1] + 1))
    rb = np.where(ref[:, 2] >= 0, ref[:, 2], -(ref[:, 2] + 1))
    wrong = (ra != contacts["body_a"][ci]) | (rb != contacts["body_b"][ci])
    if wrong.any():
        i = int(np.flatnonzero(wrong)[0])
        raise PlanMismatch("row %d holds bodies (%d, %d), contact %d of the list bodies (%d, %d)" % (
            i, ra[i], rb[i], ci[i], contacts["body_a"][ci[i]], contacts["body_b"][ci[i]]))
    entries["fixture_a"] = contacts["fixture_a"][ci]
    entries["fixture_b"] = contacts["fixture_b"][ci]
    entries["rank"] = row_ranks(plan)
    return entries, large
