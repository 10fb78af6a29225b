// b2hip_host_toi.h - part of the ONE translation unit b2hip.hip: the host side of b2World::SolveTOI (b2World.cpp:1026-1093).
// Its state on the world: ToiSwitches / ToiHints / ToiStep / ToiStats (b2hip_host_world.h). The flow: docs/TOI.md, "Host flow".
// (No include guard on purpose: b2hip.hip includes it exactly once, behind b2hip_host_phases.h - the fragments share one scope.)

// Counters::toiUnsafe: the device's bits are TOI_UNSAFE_* (b2d_kernels_toi_chains.h); this one is the host's own, never on
// the device - the speculative component path assumed that this step's pair update left the hash grid fresh, and it had not.
#define TOI_UNSAFE_STALE_GRID 0x80

// k_toi_snapshot: the state the phase starts from (bodies, fat AABBs, contacts) saved, put back, or saved beside k_toi_first
// (all but the candidates' flags and impact times: k_toi_snap_cands copies those later).
enum class ToiSnap : int { Take = 0, Restore = 1, TakeAside = 2 };
static int toiSnapshot(b2hip_world* w, hipStream_t s, ToiSnap mode)
{
	DW& d = w->dw;
	if (s == w->stream) LAUNCH(w, k_toi_snapshot, gridFor(std::max(d.nBodies, d.capContacts)), 256, d, (int)mode);
	else LAUNCH_ON(w, s, k_toi_snapshot, gridFor(std::max(d.nBodies, d.capContacts)), 256, d, (int)mode);
	return 0;
}

// The device's TOI counters, zeroed on the stream before a kernel counts into them. list: nToiList .. nToiLog, what a first
// pass starts from. words: 3 - toiUnsafe, nToiGroups, nToiMoved; 1 - toiUnsafe alone (k_toi_first's "not chains" bit, which the
// components do not mind).
static int toiZeroCounters(b2hip_world* w, bool list, int words)
{
	if (list) HIP_TRY(hipMemsetAsync(&w->d_state.p->c.nToiList, 0, sizeof(int) * 5, w->stream));
	HIP_TRY(hipMemsetAsync(&w->d_state.p->c.toiUnsafe, 0, sizeof(int) * words, w->stream));
	return 0;
}

// The serial event loop walks contacts by body (CSR) and searches new pairs through the hash grid.
static int toiBuildAdjacency(b2hip_world* w, hipStream_t s)
{
	DW& d = w->dw;
	LAUNCH_ON(w, s, k_toi_adj_clear, gridFor(d.nBodies + 1), 256, d);
	LAUNCH_ON(w, s, k_toi_adj_count, gridFor(d.capContacts), 256, d);
	deviceExclusiveScan<int>(s, d.deg, d.adjStart, d.scanTmp, w->scanCtx, w->consts.p + 4, d.nBodies + 1);
	LAUNCH_ON(w, s, k_toi_adj_fill, gridFor(d.capContacts), 256, d);
	return 0;
}

static int toiBuildIndexes(b2hip_world* w, bool csr, bool gridKnownFresh = false)
{
	if (csr)
	{
		if (int rc = toiBuildAdjacency(w, w->stream)) return rc;
	}
	// make the grid reflect every fat AABB as of now (the end-of-step pair update skips the rebuild when nothing
	// moved, and TOI moves of earlier steps never enter the move buffer) - unless this step's pair update has just built it
	// from every proxy's box and nothing moved one since (Counters::gridFresh; the kernels below check it themselves, the
	// host saves their launches when the read-back it already has says so: 128 us of a million-proxy world's step)
	// (a sharded rank launches them anyway: other ranks' boxes may have arrived since the host last looked - the kernels know)
	if (gridKnownFresh && !w->spatial) return 0;
	return gridRebuildNow(w, 1, w->scanCtx);
}

static int toiSerial(b2hip_world* w)
{
	DW& d = w->dw;
	// (every caller has read this step's counters back since the pair update: phaseToiSync, the fall-backs of toiSettle)
	int rc = toiBuildIndexes(w, true, w->h_dstate->c.gridFresh != 0);
	if (rc) return rc;
	if ((rc = toiZeroCounters(w, false, 3))) return rc;
	LAUNCH(w, k_toi_loop, 1, TOI_LANES, d, w->sp);
	if (!w->spatial) LAUNCH(w, k_toi_clear, gridFor(d.nBodies), 256, d); // (spatial worlds: k_end_step does it, behind the exchange)
	w->toiStep.path = ToiStep::Serial;
	return 0;
}

// What the component-wise event loops need besides the first pass, on the side stream beside it (see phaseToiSync).
static inline bool toiAsideWanted(const b2hip_world* w)
{
	return w->toiHints.domainsSticky > 0 && w->toiStep.countersFresh && !w->spatial && w->stream2 != nullptr && !w->noSideStream && !w->debugSync && !w->debugTrace &&
		!w->toiStep.snapshotTaken && !w->toiSw.serialOnly && !w->toiSw.noDomains && !listenerOn(w) && w->dw.toiEventCap == 0 && !w->dw.toiContinue;
}
static int toiAsideLaunch(b2hip_world* w)
{
	DW& d = w->dw;
	HIP_TRY(hipEventRecord(w->evFork, w->stream));
	HIP_TRY(hipStreamWaitEvent(w->stream2, w->evFork, 0));
	// (the short launches first: the snapshot's bandwidth then falls into the tail of k_toi_first and the host's look at its
	// census - beside its start it took the first pass from 120 to 220 us: loaded latency)
	int rc = toiBuildAdjacency(w, w->stream2);
	if (rc) return rc;
	LAUNCH_ON(w, w->stream2, k_toi_dom_init, gridFor(d.nBodies), 256, d);
	LAUNCH_ON(w, w->stream2, k_toi_dom_union, gridFor(d.capContacts), 256, d);
	LAUNCH_ON(w, w->stream2, k_toi_dom_flatten, gridFor(d.nBodies), 256, d);
	if ((rc = toiSnapshot(w, w->stream2, ToiSnap::TakeAside))) return rc;
	HIP_TRY(hipEventRecord(w->evJoin, w->stream2));
	return 0;
}

// k_toi_first takes a lane per TOI candidate (grid-stride over the manager's slot table): sized from the candidate count of
// the last read-back, generously - a wrong guess only makes the lanes loop.
static inline int toiFirstGrid(b2hip_world* w)
{
	const size_t hint = (size_t)std::max(w->h_dstate->c.nToiOrder, 0);
	return gridFor(std::min<size_t>((size_t)w->dw.capContacts, std::max<size_t>(2 * hint + 4096, 65536)));
}

// The component path behind the first pass, its components and its snapshot: pending lists per component, the event loops, the
// cross-component check, what has to be taken back and replayed serially. pending: the pending impacts (the host's count, or
// its guess: every kernel strides). snapshot: 0 - taken here; 1 - taken beside the first pass, the candidates' part copied
// here; 2 - running on the side stream, waited for here.
static int toiDomainLaunches(b2hip_world* w, int pending, int snapshot)
{
	DW& d = w->dw;
	pending = std::max(pending, 1);
	LAUNCH(w, k_toi_dom_mark, gridFor(pending), 256, d);
	LAUNCH(w, k_toi_dom_count, gridFor(d.capContacts), 256, d);
	LAUNCH(w, k_toi_dom_scan, 1, 1024, d);
	LAUNCH(w, k_toi_dom_fill, gridFor(pending), 256, d);
	if (snapshot == 1) LAUNCH(w, k_toi_snap_cands, toiFirstGrid(w), 256, d);
	else if (snapshot == 2) HIP_TRY(hipStreamWaitEvent(w->stream, w->evJoin, 0));
	else if (int rc = toiSnapshot(w, w->stream, ToiSnap::Take)) return rc;
	w->toiStep.snapshotTaken = true;
	if (w->toiHints.domWide > 0 || w->toiSw.domWideOnly)
	{
		LAUNCH(w, k_toi_domains<TOI_LANES>, std::min(pending, 2048), TOI_LANES, d, w->sp);
		if (w->toiHints.domWide > 0) w->toiHints.domWide -= 1;
	}
	else LAUNCH(w, k_toi_domains<64>, std::min(pending, 2048), 64, d, w->sp);
	LAUNCH(w, k_toi_domains_end, std::min(pending, 1024), 256, d);
	// components tied together by a new contact: back to the snapshot, then the serial loop over just those
	LAUNCH(w, k_toi_dom_rollback, gridFor(std::max(std::max(d.nBodies, d.nProxies), d.capContacts)), 256, d);
	LAUNCH(w, k_toi_loop_partial, 1, TOI_LANES, d, w->sp);
	w->toiStep.path = ToiStep::Components; // (they always have the grid: ToiStep::hadGrid)
	return 0;
}

// The chains behind the first pass: one wave per dynamic body with a pending impact, verified afterwards (toiSettle).
// census: the first pass's counters if the host has read them (they size the launches), else nullptr (the capacities do: every
// kernel strides, and leaves at once if nothing is pending). fusedSnapshot: k_toi_group_contacts takes the snapshot as well.
// The hash grid is rebuilt only while a chain has recently moved a proxy out of its fat AABB (ToiHints::gridSticky).
static int toiChainLaunches(b2hip_world* w, const Counters* census, bool fusedSnapshot)
{
	DW& d = w->dw;
	const int haveGrid = w->toiHints.gridSticky > 0 ? 1 : 0;
	const int groups = census ? std::min(std::min(census->nToiList, d.nBodies), (int)TOI_GROUPS_MAX) : 1024;
	LAUNCH(w, k_toi_groups_begin, gridFor(census ? census->nToiList : std::min(d.capContacts, 1 << 16)), 256, d);
	LAUNCH(w, k_toi_group_contacts, gridFor(fusedSnapshot ? std::max(d.nBodies, d.capContacts) : d.capContacts), 256, d, fusedSnapshot ? 1 : 0);
	if (!fusedSnapshot)
		if (int rc = toiSnapshot(w, w->stream, ToiSnap::Take)) return rc;
	w->toiStep.snapshotTaken = true;
	if (haveGrid)
	{
		if (int rc = toiBuildIndexes(w, false, census != nullptr && census->gridFresh != 0)) return rc;
	}
	LAUNCH(w, k_toi_chains, std::min(groups, 1024), CHAIN_LANES, d, w->sp, haveGrid);
	w->toiStep.chainsHadGrid = haveGrid != 0;
	w->toiStep.path = ToiStep::Chains;
	return 0;
}

static int phaseToiSync(b2hip_world* w);

// The phase without a host round trip: k_toi_first, then the chain kernels at once. Each of them leaves immediately if no
// impact is pending (or if k_toi_first saw a bullet / kinematic partner: toiUnsafe), so the host learns the outcome from
// the read-back b2hip_step_end makes anyway, and falls back there (toiSettle: snapshot restore + serial loop; or - when the
// pair update had overflowed its optimistic small-sort path, so this phase did not see every contact - restore, finish the
// contacts, and the synchronous phase: toiRedoAfterLatePairs). One read-back and ~45 us less per step with continuous physics on.
static int phaseToi(b2hip_world* w)
{
	const ToiSwitches& sw = w->toiSw; ToiHints& h = w->toiHints; ToiStep& t = w->toiStep;
	if (sw.serialOnly || sw.syncOnly || listenerOn(w) || w->dw.toiEventCap > 0 || w->dw.toiContinue || w->spatial) return phaseToiSync(w);
	if (toiAsideWanted(w) && h.lastToiList > 0 && !sw.noSpecDomains)
	{
		// The component path without the look at the first pass's census (round 5): while it has been the path of the last
		// steps, its launches are queued behind k_toi_first at once, sized from the last step's pending count (they stride);
		// every one of them leaves if nothing is pending. What the census would have told - the pair update unfinished, nothing
		// pending, a capacity cut - b2hip_step_end learns from the read-back it makes anyway and settles as it does for the
		// speculative chains; the one thing assumed - that the pair update of THIS step has left the grid fresh, as it had
		// the step before - is checked there too (Counters::gridFresh), and a wrong guess is a serial replay from the snapshot.
		DW& d = w->dw;
		int rc = toiAsideLaunch(w);
		if (rc) return rc;
		t.countersFresh = false;
		LAUNCH(w, k_toi_first, toiFirstGrid(w), 256, d);
		if ((rc = toiZeroCounters(w, false, 1))) return rc;
		HIP_TRY(hipStreamWaitEvent(w->stream, w->evJoin, 0));
		// (B2HIP_DEBUG_ASSUME_FRESH_GRID=1, for the tests: the assumption is made whatever the last step said, and the device is
		// told the grid is stale - every such step takes the wrong-guess path of toiSettle)
		const bool assumeFresh = h.gridFreshLast || sw.assumeFreshGrid;
		if (sw.assumeFreshGrid) HIP_TRY(hipMemsetAsync(&w->d_state.p->c.gridFresh, 0, sizeof(int), w->stream));
		if (!assumeFresh) { rc = toiBuildIndexes(w, false, false); if (rc) return rc; }
		if ((rc = toiDomainLaunches(w, 2 * h.lastToiList + 256, 1))) return rc;
		// (k_toi_clear's work is done by k_end_step, which follows)
		t.speculative = true;
		t.specGridAssumed = assumeFresh;
		return 0;
	}
	if (h.syncSticky > 0)
	{
		// the serial loop was needed recently (bullets, kinematic partners, contact-creating events): decide from the
		// read-back again instead of paying a wasted snapshot + state download per step
		int rc = phaseToiSync(w);
		if (rc) return rc;
		if (w->h_dstate->c.nToiList == 0 || (t.verdictPending() && w->h_dstate->c.toiUnsafe == 0)) h.syncSticky -= 1;
		else h.syncSticky = 16;
		return 0;
	}
	if (!t.countersFresh)
		if (int rc = toiZeroCounters(w, true, 3)) return rc;
	t.countersFresh = false;
	LAUNCH(w, k_toi_first, toiFirstGrid(w), 256, w->dw);
	if (int rc = toiChainLaunches(w, nullptr, true)) return rc;
	// (k_toi_clear's work is done by k_end_step, which follows)
	t.speculative = true;
	return 0;
}

// The first arg-min pass runs over the whole contact array; the host looks at its census and chooses: the chains, the
// components, or the event loop (one persistent workgroup) - which only runs when some impact lies inside the step.
static int phaseToiSync(b2hip_world* w)
{
	DW& d = w->dw;
	const ToiSwitches& sw = w->toiSw; ToiHints& h = w->toiHints; ToiStep& t = w->toiStep;
	// one read-back serves both questions: did the optimistic small-sort path of the end-of-step pair update
	// apply (else finish it first: the TOI phase must see every contact), and is any impact pending
	int rc = 0;
	// While the component-wise event loops have been in use (bullets: config 5), what they need besides the first pass - the
	// snapshot (230 MB for a million bodies: bandwidth), the adjacency of all contacts and the components (a dozen short
	// launches: latency) - does not wait for it: none of that reads what k_toi_first writes except the candidates' flags and
	// impact times, which k_toi_snap_cands copies afterwards. It runs on the side stream (idle behind Solve) beside
	// k_toi_first - a few heavy lanes, ~120 us - and the host's look at its census: ~180 us of the step's critical path.
	// Void if the pair update has to be finished first (the contact array grows under it): then everything is done again below.
	bool aside = false;
	if (toiAsideWanted(w))
	{
		if ((rc = toiAsideLaunch(w))) return rc;
		aside = true;
	}
	bool asideValid = aside;
	for (int pass = 0; pass < 2; ++pass)
	{
		if (pass == 1 && aside)
		{
			// (the contact array is about to change, or has: the side stream's work is void - and must have ended)
			HIP_TRY(hipStreamWaitEvent(w->stream, w->evJoin, 0));
			asideValid = false;
		}
		// (the first pass of a step starts from the zeros of k_step_begin)
		if (pass == 1 || !t.countersFresh)
			if ((rc = toiZeroCounters(w, true, 3))) return rc;
		t.countersFresh = false;
		LAUNCH(w, k_toi_first, toiFirstGrid(w), 256, d);
		if ((rc = readState(w))) return rc;
		if (w->h_dstate->c.overflow & 3)
		{
			// the end-of-step pair update overflowed its buffer (or the contact array): grow, run the whole update again, look again
			if (pass == 1) return setError(B2HIP_ERR_CAPACITY, "pair buffer overflow");
			if (aside && asideValid) { HIP_TRY(hipStreamWaitEvent(w->stream, w->evJoin, 0)); asideValid = false; }
			if ((rc = growPairBuffers(w))) return rc;
			if ((rc = findNewContacts(w, true))) return rc;
			continue;
		}
		if (pass == 1 || w->h_dstate->c.nMoves == 0 || w->h_dstate->c.nPairs <= COUNT_RANK_MAX) break;
		if (aside && asideValid) { HIP_TRY(hipStreamWaitEvent(w->stream, w->evJoin, 0)); asideValid = false; }
		if ((rc = runSortAndCreate(w, true, w->h_dstate->c.nPairs))) return rc;
	}
	// (whatever follows writes what the side stream reads: it has had ~200 us, the wait is a formality)
	if (aside) HIP_TRY(hipStreamWaitEvent(w->stream, w->evJoin, 0));
	if (h.domainsSticky > 0) h.domainsSticky -= 1;
	const Counters& c = w->h_dstate->c;
	w->last.nToiList = c.nToiList;
	w->last.nToiCalls = c.nToiCalls;
	w->last.nToiEvents = 0;
	w->spContactsBeforeToi = c.nContacts;
	w->spToiOrderBefore = c.nToiOrder;
	// (sub-stepping: one event per call in the reference's serial order; a call that continues a step has impacts to compute
	// even when nothing is pending yet - the event loop's first batch)
	const bool subStepped = d.toiEventCap > 0 || d.toiContinue != 0;
	if (c.nToiList == 0 && !d.toiContinue) return 0;
	if (c.nToiList > d.capContacts) return setError(B2HIP_ERR_CAPACITY, "TOI list overflow");
	t.ran = true;
	if (c.toiUnsafe == 0 && !sw.serialOnly && !listenerOn(w) && !subStepped)
	{
		// every pending impact pairs a dynamic body with a static one: the chains
		// (toiSettle falls back to the serial loop from the snapshot if a chain met a case that is order dependent)
		w->toiStats.n[ToiStats::ChainsCensus] += 1;
		if ((rc = toiChainLaunches(w, &c, false))) return rc;
		if (!w->spatial) LAUNCH(w, k_toi_clear, gridFor(d.nBodies), 256, d);
		return 0;
	}
	if (!sw.serialOnly && !sw.noDomains && !listenerOn(w) && !subStepped)
	{
		// bullets / kinematic partners: the event loop runs per connected component of the contact graph, side by side
		// (b2d_kernels_toi_domains.h); toiSettle falls back to the serial loop from the snapshot if a component met
		// something that couples it to another one
		// The snapshot (230 MB for a million bodies: bandwidth) runs on the side stream beside the dozen short launches that build
		// the adjacency and the components (latency): nothing they write is anything it reads, the stream is drained (readState
		// above), and the side stream is idle behind Solve. The event loops wait for it.
		w->toiStats.n[ToiStats::ComponentsCensus] += 1;
		h.domainsSticky = 16;
		const bool snapAside = !asideValid && w->stream2 != nullptr && !w->noSideStream && !w->debugSync && !w->debugTrace;
		if (snapAside)
		{
			if ((rc = toiSnapshot(w, w->stream2, ToiSnap::Take))) return rc;
			HIP_TRY(hipEventRecord(w->evJoin, w->stream2));
		}
		// (asideValid: snapshot, adjacency and components are there - the grid, if this step's pair update has not left one)
		if ((rc = toiBuildIndexes(w, !asideValid, c.gridFresh != 0))) return rc;
		if (!asideValid)
		{
			LAUNCH(w, k_toi_dom_init, gridFor(d.nBodies), 256, d);
			LAUNCH(w, k_toi_dom_union, gridFor(d.capContacts), 256, d);
			LAUNCH(w, k_toi_dom_flatten, gridFor(d.nBodies), 256, d);
		}
		if ((rc = toiZeroCounters(w, false, 1))) return rc;
		h.lastToiList = c.nToiList;
		h.gridFreshLast = c.gridFresh != 0;
		if ((rc = toiDomainLaunches(w, c.nToiList, asideValid ? 1 : snapAside ? 2 : 0))) return rc;
		if (!w->spatial) LAUNCH(w, k_toi_clear, gridFor(d.nBodies), 256, d);
		return 0;
	}
	w->toiStats.n[ToiStats::SerialDirect] += 1;
	if ((hasPreSolve(w) || w->spatial) && !t.snapshotTaken)
	{
		// a PreSolve called from a sub-step may change that sub-step (toiPreSolveRounds): the phase must be able to start over
		// (a spatially sharded world sends the other ranks what differs from this snapshot: spAfterToi)
		if ((rc = toiSnapshot(w, w->stream, ToiSnap::Take))) return rc;
		t.snapshotTaken = true;
	}
	return toiSerial(w);
}

// The phase once more, through phaseToiSync: the one place that clears what a second run needs cleared. NOT cleared, on
// purpose: snapshotTaken (the second run goes back to where the FIRST one started, and a snapshot that is there keeps
// phaseToiSync's side-stream preparations off, as it always has) and ran (impacts were pending, and are again). Callers say
// what differs: whether the snapshot goes back first, what is redone or grown in between, whether the outcome is read back.
static int toiRunAgain(b2hip_world* w)
{
	w->toiStep.dropVerdict();
	w->toiStep.countersFresh = false;
	return phaseToiSync(w);
}

// The end-of-step pair update is finished late (b2hip_step_end): a phase queued without its census ran without the contacts
// created only now. redo: there is one; it is undone here if anything was pending, and redone behind the pair update - judged
// on its own, not by what the queued launches assumed of the grid (toiRunAgain drops "speculative").
static int toiUndoBeforeLatePairs(b2hip_world* w, bool& redo)
{
	redo = w->toiStep.speculative;
	return redo && w->h_dstate->c.nToiList > 0 ? toiSnapshot(w, w->stream, ToiSnap::Restore) : 0;
}
static int toiRedoAfterLatePairs(b2hip_world* w)
{
	w->toiStats.n[ToiStats::RedoLatePairs] += 1;
	return toiRunAgain(w);
}

// The grid hint: a rebuilt hash grid for 16 steps after a chain moved a proxy. countDown: false for a second look at one step.
static inline void toiGridHint(b2hip_world* w, int nToiMoved, bool countDown)
{
	if (!w->toiStep.verdictPending()) return;
	if (nToiMoved > 0) w->toiHints.gridSticky = 16;
	else if (w->toiHints.gridSticky > 0 && countDown) w->toiHints.gridSticky -= 1;
}

// The fall-back ladder. A parallel path's verdict is in (unsafe: Counters::toiUnsafe as b2hip_step_end's read-back shows it,
// or as a sharded rank's exchange header does: spAfterToi). In this order: the hints for the next steps; the queued components'
// one assumption; the snapshot back; the chains once more with the grid, if that is all they lacked; the serial loop; the
// statistics and the stickies. What a sharded rank does differently:
//  * the grid hint is updated where the header is read (spExchangeState: every exchange passes there, also those that bring
//    spAfterToi no verdict), counting down only if (!spToiSettled) - the exchange behind a fall-back sees the same step again;
//  * no read-back behind a rung: the outcome travels in the rank's header of the next exchange, which spAfterToi makes anyway
//    (so no B2HIP_TOI_WHY line either: the counters it prints are a read-back's);
//  * a capacity cut does not widen the components' event loops for the next 64 steps (reason not recorded).
// (The sharded copy of this ladder also reset ToiStep::countersFresh before its grid retry: toiRunAgain does, for both - a
// phase that has run has left it false already.)
static int toiSettle(b2hip_world* w, int unsafe, bool sharded)
{
	ToiHints& h = w->toiHints; ToiStep& t = w->toiStep;
	const Counters& c = w->h_dstate->c;
	const bool specComponents = t.specComponents();
	if (t.speculative)
	{
		// what phaseToiSync would have learnt from the census
		if (c.nToiList > w->dw.capContacts) return setError(B2HIP_ERR_CAPACITY, "TOI list overflow");
		w->last.nToiList = c.nToiList;
		w->last.nToiCalls = c.nToiCalls;
		t.ran = c.nToiList > 0;
		if (t.ran) w->toiStats.n[specComponents ? ToiStats::ComponentsQueued : ToiStats::ChainsQueued] += 1;
		else t.dropVerdict(); // (every kernel left at once: no verdict. "speculative" is not asked for again this step)
	}
	if (specComponents)
	{
		h.lastToiList = c.nToiList;
		h.gridFreshLast = c.gridFresh != 0;
		if (c.nToiList > 0) h.domainsSticky = 16;
		else if (h.domainsSticky > 0) h.domainsSticky -= 1;
		// (the event loops searched a grid that this step's pair update had NOT rebuilt - nothing moved, the first step in
		// many: as with any order-dependent case, back to the snapshot and the serial loop, which builds its own)
		if (t.verdictPending() && t.specGridAssumed && c.gridFresh == 0) unsafe |= TOI_UNSAFE_STALE_GRID;
	}
	if (!sharded) toiGridHint(w, c.nToiMoved, true);
	if (!t.verdictPending() || unsafe == 0) return 0;
	// a chain or a component met an order-dependent case: back to the state before them, then the reference's serial order
	int rc = toiSnapshot(w, w->stream, ToiSnap::Restore);
	if (rc) return rc;
	if (t.path == ToiStep::Chains && unsafe == TOI_UNSAFE_PAIR && !t.hadGrid() && !w->dw.noChainCreate)
	{
		// ... unless all that happened is that a chain moved a proxy out of its fat AABB while the hash grid was not kept
		// up (nothing had moved for 16 steps): the chains once more, with the grid - most such moves find nothing, or a
		// pair the chains' close-out can create itself. (The serial loop costs ~50 us per event: 15 ms for the 290 resting
		// impacts of a 50 000-box pyramid; this costs a second first pass.)
		h.gridSticky = 16;
		w->toiStats.n[ToiStats::GridRetry] += 1;
		if ((rc = toiRunAgain(w))) return rc;
		if (sharded) return 0; // (its outcome comes with the next exchange's headers)
		if ((rc = downloadState(w, -1))) return rc;
		unsafe = c.toiUnsafe;
		if (!t.verdictPending() || unsafe == 0) return 0;
		if ((rc = toiSnapshot(w, w->stream, ToiSnap::Restore))) return rc;
	}
	if (w->toiSw.why && !sharded) fprintf(stderr, "b2hip: TOI fallback to the serial loop, unsafe bits 0x%x (1 partner, 2 woke, 4 new pair, 8 capacity, 16 moved proxies), %d pending, %d components\n", unsafe, c.nToiList, c.nToiDomains);
	// (a capacity cut - possibly more candidate contacts in one event than the narrow component loops have lanes: the wide form next time)
	if ((unsafe & TOI_UNSAFE_CAPACITY) && !sharded) h.domWide = 64;
	if ((rc = toiSerial(w))) return rc; // (path = Serial: nothing left to be unsafe about)
	w->toiStats.n[ToiStats::SerialFallback] += 1;
	h.syncSticky = 16;
	return sharded ? 0 : downloadState(w, -1);
}

// The answers collected so far go to the device before the phase runs again (DW::toiVerdict, DW::nToiVerdict).
static int uploadToiVerdicts(b2hip_world* w)
{
	const std::vector<int4>& v = w->toiStep.verdicts;
	const size_t n = std::min(v.size(), w->toiVerdict.cap);
	w->dw.nToiVerdict = w->dw.toiVerdict != nullptr ? (int)n : 0;
	if (w->dw.nToiVerdict > 0) HIP_TRY(hipMemcpyAsync((void*)w->toiVerdict.p, v.data(), n * sizeof(int4), hipMemcpyHostToDevice, w->stream));
	return 0;
}

// A contact created inside a TOI sub-step did not fit the array (whatever path ran last, fallbacks included): never a
// silent drop. With the snapshot of this step's TOI phase at hand the phase is undone, the array doubled and the phase
// run again; without one (serial-only mode) it is an error.
static int settleToiOverflow(b2hip_world* w)
{
	int rc = 0;
	for (int attempt = 0; (w->h_dstate->c.overflow & 1) != 0; ++attempt)
	{
		if (!w->toiStep.snapshotTaken || attempt == 3) return setError(B2HIP_ERR_CAPACITY, "contact array full during a TOI sub-step");
		// (edits can only be pending here if a PreSolve called from a sub-step made them: toiPreSolveRounds)
		if (!w->dirtyList.empty() || !w->editOps.empty() || !w->proxyEdits.empty() || !w->pendingMoves.empty())
			return setError(B2HIP_ERR_CAPACITY, "contact array full during a TOI sub-step whose PreSolve edited the world");
		if ((rc = toiSnapshot(w, w->stream, ToiSnap::Restore))) return rc;
		if ((rc = ensureCapacity(w, 2 * (size_t)w->dw.capContacts))) return rc;
		if ((rc = uploadToiVerdicts(w))) return rc;
		HIP_TRY(hipMemsetAsync(&w->d_state.p->c.overflow, 0, sizeof(int), w->stream));
		w->toiStats.n[ToiStats::OverflowRerun] += 1;
		if ((rc = toiRunAgain(w))) return rc;
		if (w->toiStep.verdictPending())
		{
			// (the parallel paths report through toiUnsafe: toiSettle's last rung alone - no hints, no grid retry, no sticky,
			// as it has always been here; reason not recorded)
			if ((rc = downloadState(w, -1))) return rc;
			if (w->h_dstate->c.toiUnsafe != 0)
			{
				if ((rc = toiSnapshot(w, w->stream, ToiSnap::Restore))) return rc;
				if ((rc = toiSerial(w))) return rc;
				w->toiStats.n[ToiStats::SerialFallback] += 1;
			}
		}
		if ((rc = downloadState(w, -1))) return rc;
	}
	return 0;
}

static void toiCallbackFromLog(const ToiLogRec& r, b2hip_toi_callback* cb)
{
	memset(cb, 0, sizeof(*cb));
	cb->kind = r.info.x;
	cb->contact_index = r.info.y;
	cb->fixture_a = r.info.z;
	cb->fixture_b = r.info.w;
	toManifold(&cb->old_manifold, r.o0, r.o1, r.oimp, r.o3);
	toManifold(&cb->manifold, r.n0, r.n1, r.nimp, r.n3);
	cb->material.friction = r.mat.x;
	cb->material.restitution = r.mat.y;
	cb->material.tangent_speed = r.mat.z;
}

// b2ContactListener::PreSolve from INSIDE the TOI sub-steps (b2World.cpp:866,946 -> b2Contact::Update -> b2Contact.cpp:283-297).
// The reference calls it in the middle of its event loop, and what it does to the contact changes that sub-step: a contact
// switched off keeps the sweeps of its bodies and stays out of the sub-step's island (b2World.cpp:873-881, 948-954), an
// edited material is what the sub-step's solver reads. The event loop here is one kernel, so the phase is run to its end,
// its log (DW::toiLog: the Updates in the reference's call order) read, and PreSolve called for the logged Updates in
// order - each exactly once. An answer that changes nothing needs nothing: the contact stays on (or off, where the sub-step
// assumed the listener's last answer for this contact: CF_PRESOLVE_OFF, toiPreSolveOutcome) and its material as it was. The
// first one that does makes everything after it void: the phase goes back to its snapshot and runs again with the
// answers so far on the device (the loop applies them at the same log slots - it is deterministic, so the log repeats
// itself up to there), and the calls go on behind the slot that was answered. One extra run of the phase per changing answer.
static int toiPreSolveRounds(b2hip_world* w, std::vector<ToiLogRec>& recs)
{
	int asked = 0; // log slots whose PreSolve has been called
	for (int round = 0;; ++round)
	{
		const int n = std::min(w->h_dstate->c.nToiLog, w->dw.capToiLog);
		recs.resize((size_t)std::max(n, 0));
		if (n > 0) HIP_TRY(hipMemcpy((void*)recs.data(), w->toiLog.p, (size_t)n * sizeof(ToiLogRec), hipMemcpyDeviceToHost));
		if (!hasPreSolve(w) || w->dw.toiVerdict == nullptr) return 0;
		// (the log itself was cut short: no listener call from a truncated log - the step fails with the capacity error below)
		if (w->h_dstate->c.toiOverflow & 64) return 0;
		// The callbacks below may edit bodies (callbackWindow). h_state holds the state AFTER this step's phases by now, but the
		// mirror's epoch is only advanced at the very end of the step (refreshMirror): a body the host had touched before the
		// step (a force applied every frame) would not be pulled again and the edit would land on - and later upload - its
		// pre-step row. The read-back that just happened is the mirror from here on.
		if (n > asked) refreshMirror(w);
		bool again = false;
		for (int k = asked; k < n && !again; ++k)
		{
			const ToiLogRec& r = recs[(size_t)k];
			int4 v = make_int4(0, 0, 0, 0);
			if (r.info.x & 4)
			{
				b2hip_toi_callback cb;
				toiCallbackFromLog(r, &cb);
				b2hip_pre_solve_record rec;
				rec.contact_index = cb.contact_index;
				rec.fixture_a = cb.fixture_a;
				rec.fixture_b = cb.fixture_b;
				rec.enabled = 1;
				rec.old_manifold = cb.old_manifold;
				rec.manifold = cb.manifold;
				rec.material = cb.material;
				// (world edits made from the callback are taken like edits between steps: they reach the device before the next step)
				w->callbackWindow = true;
				if (w->preSolveBatchFn) w->preSolveBatchFn(w->preSolveUser, 1, &rec);
				else rec.enabled = w->preSolveFn(w->preSolveUser, rec.contact_index, rec.fixture_a, rec.fixture_b, &rec.old_manifold, &rec.manifold, &rec.material) ? 1 : 0;
				w->callbackWindow = false;
				int bits[3];
				memcpy(bits, &rec.material, sizeof(bits));
				v = make_int4(1 | (rec.enabled ? 0 : 2), bits[0], bits[1], bits[2]);
				// (bit 4 of the kind: the sub-step went on as if the contact had been switched off - the listener's last answer)
				const bool assumedOff = (r.info.x & 16) != 0;
				again = (rec.enabled != 0) == assumedOff || memcmp(&rec.material.friction, &r.mat.x, 4) != 0 || memcmp(&rec.material.restitution, &r.mat.y, 4) != 0 ||
					memcmp(&rec.material.tangent_speed, &r.mat.z, 4) != 0;
			}
			w->toiStep.verdicts.push_back(v);
			asked = k + 1;
		}
		if (!again) return 0;
		if (!w->toiStep.snapshotTaken) return setError(B2HIP_ERR_INVALID, "PreSolve changed a contact inside a TOI sub-step, and the phase kept no snapshot");
		if (round >= w->dw.capToiLog) return setError(B2HIP_ERR_INVALID, "TOI PreSolve rounds do not end");
		// (the host mirror of an edited body was refreshed from the state that is about to be taken back)
		if (!w->dirtyList.empty() || !w->editOps.empty() || !w->proxyEdits.empty() || !w->pendingMoves.empty())
			return setError(B2HIP_ERR_INVALID, "a PreSolve inside a TOI sub-step edited the world AND changed its contact: not supported");
		int rc = toiSnapshot(w, w->stream, ToiSnap::Restore);
		if (rc) return rc;
		if ((rc = uploadToiVerdicts(w))) return rc;
		if ((rc = toiRunAgain(w))) return rc;
		if ((rc = downloadState(w, -1))) return rc;
		if ((rc = settleToiOverflow(w))) return rc;
		w->toiStats.n[ToiStats::PreSolveRerun] += 1;
	}
}
