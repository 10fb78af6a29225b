// b2hip_host_phases.h - part of the ONE translation unit b2hip.hip: the phases of a step as launch sequences on the world's
// stream - pair update (findNewContacts), Collide, Solve (island build, census, colouring, the solver tiers: phaseSolve),
// SynchronizeFixtures, SolveTOI with its parallel paths and fallbacks, the read-back (downloadState).
// (No include guard on purpose: b2hip.hip includes it exactly once, in order - the fragments share one scope.)

// ------------------------------------------------------------------------------------------------
// Phases
// ------------------------------------------------------------------------------------------------
// spatially sharded worlds (defined behind the RCCL section; b2d_kernels_spatial.h)
static int spExchangeState(b2hip_world* w, int mode);
static int spExchangePairs(b2hip_world* w, long long* totalPairs, int* straddling);
static int spResolve(b2hip_world* w, int nVirt = 0);
static int spAfterToi(b2hip_world* w);
static int spBeginStep(b2hip_world* w);

static int radixBits(int maxKey)
{
	int bits = 1;
	while ((1 << bits) <= maxKey && bits < 31) ++bits;
	return bits;
}

// The passes of a stable LSD sort over bits [first, first + bits) of the keys: (shift, width) pairs of at most RADIX_BITS bits
// each, as few as cover the range, of (almost) equal width.
static void radixPasses(int first, int bits, std::vector<std::pair<int, int>>& out)
{
	const int passes = (bits + RADIX_BITS - 1) / RADIX_BITS;
	for (int p = 0, at = 0; p < passes; ++p)
	{
		const int width = (bits - at + (passes - p) - 1) / (passes - p);
		out.push_back(std::make_pair(first + at, width));
		at += width;
	}
}

// keys / payloads in (kin, vin), *nPtr of them; sorted by the bits the passes name; which buffers hold the result comes back in kin / vin
// One launch per pass behind one that counts every pass's digits (k_radix_prepare / k_radix_onepass, b2d_scan.h) wherever the
// status words cover the tiles; three launches per pass (B2HIP_SORT_ONEPASS=0: always) beyond RADIX_ONEPASS_MAX_TILES, for more
// than RADIX_MAX_PASSES passes and on a stream that is being captured.
static int radixSort(b2hip_world* w, uint64_t*& kin, uint64_t*& kout, int2*& vin, int2*& vout, const int* nPtr, int tilesCap, const std::vector<std::pair<int, int>>& passes, int overflowBit = 0)
{
	DW& d = w->dw;
	w->statSorts += 1;
	RadixStatus& rs = w->radixCtx;
	if (w->sortOnepass && radixOnepassFits(w->stream, rs, tilesCap, passes.size()))
	{
		w->statSortsOnepass += 1;
		if (rs.epoch + passes.size() > 0xffffu)
		{
			// (the tag is about to wrap: no word of 65 535 passes ago may read as published - as deviceExclusiveScan's epoch)
			HIP_TRY(hipMemsetAsync(rs.counts, 0, rs.countsCap * sizeof(unsigned), w->stream));
			HIP_TRY(hipMemsetAsync(rs.groups, 0, rs.groupsCap * sizeof(unsigned), w->stream));
			rs.epoch = 0u;
		}
		RadixLayout lay;
		lay.passes = (int)passes.size();
		for (int p = 0; p < RADIX_MAX_PASSES; ++p)
		{
			lay.shift[p] = p < lay.passes ? passes[p].first : 0;
			lay.width[p] = p < lay.passes ? passes[p].second : 0;
		}
		int* hist = rs.hist + rs.parity * (RADIX_MAX_PASSES * RADIX_DIGITS);
		int* histNext = rs.hist + (1u - rs.parity) * (RADIX_MAX_PASSES * RADIX_DIGITS);
		rs.parity = 1u - rs.parity;
		LAUNCH(w, k_radix_prepare, (tilesCap + RADIX_PREPARE_TILES - 1) / RADIX_PREPARE_TILES, RADIX_THREADS, kin, nPtr, tilesCap, lay, hist, histNext,
			overflowBit ? &d.st->c.overflow : (int*)nullptr, overflowBit);
		for (size_t p = 0; p < passes.size(); ++p)
		{
			const unsigned tag = ++rs.epoch;
			LAUNCH(w, k_radix_onepass, tilesCap, RADIX_THREADS, kin, vin, kout, vout, (const int*)(hist + p * RADIX_DIGITS), rs.counts, rs.groups, nPtr,
				passes[p].first, passes[p].second, tag, rs.abortWord);
			std::swap(kin, kout);
			std::swap(vin, vout);
		}
		return 0;
	}
	// (the length of the histogram matrix depends on the count only: once per sort, not once per pass)
	LAUNCH(w, k_radix_count, 1, 1, nPtr, 0, w->consts.p + 2, tilesCap, overflowBit ? &d.st->c.overflow : (int*)nullptr, overflowBit);
	for (size_t p = 0; p < passes.size(); ++p)
	{
		LAUNCH(w, k_radix_hist, tilesCap, RADIX_THREADS, kin, d.radixHist, nPtr, 0, passes[p].first, passes[p].second, tilesCap);
		deviceExclusiveScan<int>(w->stream, d.radixHist, w->radixHistScan.p, d.scanTmp, w->scanCtx, w->consts.p + 2, RADIX_DIGITS * tilesCap);
		LAUNCH(w, k_radix_scatter, tilesCap, RADIX_THREADS, kin, vin, kout, vout, w->radixHistScan.p, nPtr, 0, passes[p].first, passes[p].second);
		std::swap(kin, kout);
		std::swap(vin, vout);
	}
	return 0;
}

// Uploads `list` and runs `kernel(d, list, count)` (contacts to disable / reject, candidate pairs to drop)
template <typename K>
static int applyHostList(b2hip_world* w, K kernel, const std::vector<int>& list)
{
	if (list.empty()) return 0;
	HIP_TRY(hipMemcpyAsync(w->hostList.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, w->stream));
	LAUNCH(w, kernel, gridFor(list.size()), 256, w->dw, (const int*)w->hostList.p, (int)list.size());
	HIP_TRY(hipStreamSynchronize(w->stream));
	return 0;
}

// b2ContactManager::AddPair's user filter (b2ContactManager.cpp:283-287): the first occurrence of every candidate pair is
// shown to the user's b2hip_should_collide_fn (lower proxy id first, as AddPair passes them); refused pairs stop being
// first occurrences, so nothing is created for them. Between the "first" flags and the ranks of either ordering path.
// the user's filter on a list of fixture pairs: one call with all of them (batch form) or one call per pair
static void askFilter(b2hip_world* w, const std::vector<int>& pairs2, std::vector<int>& verdict)
{
	const int n = (int)pairs2.size() / 2;
	verdict.assign((size_t)n, 1);
	if (n == 0) return;
	if (w->filterBatchFn) w->filterBatchFn(w->filterUser, n, pairs2.data(), verdict.data());
	else for (int i = 0; i < n; ++i) verdict[i] = w->filterFn(w->filterUser, pairs2[2 * i], pairs2[2 * i + 1]) ? 1 : 0;
}

static int userFilterPairs(b2hip_world* w, const int2* proxies)
{
	int rc = readState(w);
	if (rc) return rc;
	const int n = std::min(w->h_dstate->c.nPairs, w->dw.capPairs);
	if (n <= 0 || (w->h_dstate->c.overflow & 3)) return 0;
	std::vector<int> first(n);
	std::vector<int2> pr(n);
	HIP_TRY(hipMemcpy(first.data(), w->pairFirst.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(pr.data(), proxies, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost));
	std::vector<int> refused, asked, which, verdict;
	for (int i = 0; i < n; ++i)
	{
		if (!first[i]) continue;
		asked.push_back(pr[i].x);
		asked.push_back(pr[i].y);
		which.push_back(i);
	}
	askFilter(w, asked, verdict);
	for (size_t k = 0; k < which.size(); ++k) if (!verdict[k]) refused.push_back(which[k]);
	return applyHostList(w, k_pairs_reject, refused);
}

// b2World::FindNewContacts. `sync` = the host may block on the pair count to pick the sort path
// (top-of-step call after fixtures were added); otherwise the small path runs optimistically and
// the caller checks Counters::nPairs at the end-of-step read-back.
// knownPairs: the candidate pairs in the buffer where the host has just read the count (-1: unknown) - the radix passes then
// launch and scan for that many tiles, not for the buffer's capacity (a rank of a sharded world keeps buffers of the whole
// world's size: eleven scans per step took the three-kernel form for 25 000 pairs)
static int runSortAndCreate(b2hip_world* w, bool largePath, long long knownPairs = -1)
{
	DW& d = w->dw;
	const uint64_t* sortedKeys = d.pairKey;
	const int2* sortedProxies = d.pairProxy;
	if (largePath)
	{
		// LSD radix sort on the two key halves
		int bits = radixBits(w->nextNode + 1);
		std::vector<std::pair<int, int>> passes;
		radixPasses(0, bits, passes);
		radixPasses(32, bits, passes);
		uint64_t* kin = d.pairKey;
		uint64_t* kout = d.pairKey2;
		int2* vin = d.pairProxy;
		int2* vout = d.pairProxy2;
		int tilesCap = d.capPairs / RADIX_TILE + 1;
		if (knownPairs >= 0) tilesCap = (int)std::min<long long>(tilesCap, knownPairs / RADIX_TILE + 2);
		if (int rcs = radixSort(w, kin, kout, vin, vout, &d.st->c.nPairs, tilesCap, passes)) return rcs;
		sortedKeys = kin;
		sortedProxies = vin;
		LAUNCH(w, k_pairs_sorted_first, gridFor(d.capPairs), 256, d, sortedKeys, w->consts.p + 3);
		if (hasFilter(w)) { int rcf = userFilterPairs(w, sortedProxies); if (rcf) return rcf; }
		deviceExclusiveScan<int>(w->stream, d.pairFirst, d.pairRank, d.scanTmp, w->scanCtx, w->consts.p + 3,
			knownPairs >= 0 ? (int)std::min<long long>(d.capPairs, knownPairs + 2) : d.capPairs);
		LAUNCH(w, k_pairs_sorted_total, 1, 1, d, w->consts.p + 3);
	}
	else
	{
		LAUNCH(w, k_pairs_first, 16, 256, d);
		if (hasFilter(w)) { int rcf = userFilterPairs(w, sortedProxies); if (rcf) return rcf; }
		LAUNCH(w, k_pairs_rank, 16, 256, d);
	}
	const int smallPath = largePath ? 0 : 1;
	LAUNCH(w, k_create_contacts, gridFor(largePath ? d.capPairs : COUNT_RANK_MAX), 256, d, sortedKeys, sortedProxies, smallPath);
	LAUNCH(w, k_create_finish, gridFor(d.nBodies), 256, d, smallPath);
	LAUNCH(w, k_toi_order_create, 1, 1024, d, smallPath); // (+ the commit of the update)
	return 0;
}

static int findNewContacts(b2hip_world* w, bool sync);
static int findNewContactsOnce(b2hip_world* w, bool sync);
// The pair update at the end of the step.
static int findNewContactsGraph(b2hip_world* w)
{
	// (a user contact filter is asked on the host in the middle of the update: synchronous)
	if (hasFilter(w) || w->spatial) return findNewContacts(w, true);
	// A scene that creates more pairs per step than the optimistic counting path ranks (the settled 50 086-box pyramid and the
	// 100 000-box Tumbler: ~25 000 and ~150 000 new fat-AABB pairs per step) would find that out at the end of the step, sort
	// with the radix path then - and run the TOI phase and the read-back a second time, every step. While that has happened
	// lately the host looks at the pair count right after the search instead (one small read-back) and takes the right path.
	// (Not looking at all - the radix passes queued behind the search for twice the last update's count, checking the size
	// themselves - was built and measured in round 5, same box, same states: Tumbler 3.49 against 3.50 ms, Pyramid 316 1.37
	// against 1.39, and the 1 M field 2.6 against 2.2: its updates alternate between 3 000 and 150 000 pairs, every second guess
	// was too small and the update ran twice. The gaps a kernel trace shows behind this read-back are the profiler's.)
	return findNewContacts(w, w->pairsLargeSticky > 0);
}

// The pair finder met more candidate pairs than the buffer holds (a dense start: every proxy is "moved" and overlaps dozens
// of others). Counters::nPairs counted all of them: size the buffers for that and let the caller run the search again
// (nothing was consumed: the creation kernels leave an overflowed set alone and the moves stay buffered).
static int growPairBuffers(b2hip_world* w)
{
	const Counters& c = w->h_dstate->c;
	if (c.overflow & 2) w->pairCapHint = 2 * (size_t)c.nPairs + 4096;
	// (bit 0: the new contacts did not fit the contact array - creation was skipped as a whole, see createBlocked)
	int rc = ensureCapacity(w, (size_t)c.nContacts + (size_t)std::max(c.nNewContacts, 0) + 1024);
	if (rc) return rc;
	HIP_TRY(hipMemsetAsync(&w->d_state.p->c.overflow, 0, sizeof(int), w->stream));
	return 0;
}

static int findNewContacts(b2hip_world* w, bool sync)
{
	w->contactsKnown = false; // (until the read-back behind it: contacts and TOI candidates are created)
	forestDrop(w);
	for (int attempt = 0; sync && attempt < 4; ++attempt)
	{
		int rc = findNewContactsOnce(w, true);
		if (rc != 1) return rc; // 1 = pair buffer overflow, buffers grown: search again
	}
	if (sync) return setError(B2HIP_ERR_CAPACITY, "pair buffer overflow");
	return findNewContactsOnce(w, false);
}

static int findNewContactsOnce(b2hip_world* w, bool sync)
{
	DW& d = w->dw;
	LAUNCH(w, k_bp_clear, gridFor(std::max(d.htMask, d.gridMask) + 1), 256, d);
	LAUNCH(w, k_bp_build, gridFor(std::max(d.capContacts, d.nProxies)), 256, d);
	deviceExclusiveScan<int>(w->stream, d.gridCount, d.gridStart, d.scanTmp, w->scanCtx, w->consts.p + 1, (int)(d.gridMask + 1));
	LAUNCH(w, k_grid_fill, gridFor(d.nProxies), 256, d, 0);
	if (int rk = ktBracket(w, 4, 7)) return rk;
	if (d.gridHalf) LAUNCH(w, k_find_pairs_window, gridFor((size_t)d.capMoves * 64, 256, 2048), 256, d);
	else LAUNCH(w, k_find_pairs_small, gridFor((size_t)d.capMoves * 64, 256, 2048), 256, d);
	if (int rk = ktBracket(w, 4, 7)) return rk;
	LAUNCH(w, k_find_pairs_large, 1024, 256, d);
	bool large = false;
	if (w->spatial)
	{
		// E2: every rank searched for the proxies ITS bodies moved; all ranks order and create the union. The headers of the
		// slabs tell every host what it needs to go on (one synchronisation): the size of the union -> the ordering path, and
		// whether a new pair joins bodies of different owners
		long long total = 0;
		int straddle = 0;
		int rc = spExchangePairs(w, &total, &straddle);
		if (rc) return rc;
		large = total > COUNT_RANK_MAX;
		rc = runSortAndCreate(w, large, total);
		if (rc) return rc;
		if (straddle == 0)
		{
			// CF_FOREIGN of the new contacts (nothing straddles: no resolution, nothing to read back)
			HIP_TRY(hipMemsetAsync(&w->d_state.p->c.nStraddle, 0, 4 * sizeof(int), w->stream));
			LAUNCH(w, k_sp_flag_contacts, gridFor(d.capContacts), 256, d);
			return 0;
		}
		// E3: a new contact joins components of different owners
		return spResolve(w);
	}
	if (sync)
	{
		int rc = startEarlyRows(w); // (before the host waits for the pair count)
		if (rc) return rc;
		rc = readState(w);
		if (rc) return rc;
		if (w->h_dstate->c.overflow & 3)
		{
			rc = growPairBuffers(w);
			return rc ? rc : 1;
		}
		if (w->h_dstate->c.nMoves == 0) { if (w->pairsLargeSticky > 0) w->pairsLargeSticky -= 1; return 0; }
		large = w->h_dstate->c.nPairs > COUNT_RANK_MAX;
		if (large) w->pairsLargeSticky = 16;
		else if (w->pairsLargeSticky > 0) w->pairsLargeSticky -= 1;
	}
	return runSortAndCreate(w, large, sync ? (long long)w->h_dstate->c.nPairs : -1);
}

static int phaseCollide(b2hip_world* w)
{
	// (the form of k_collide, b2d_kernels_collide.h: from 262 144 contacts on - a thousand workgroups - the replay of the dying
	// TOI candidates is a launch of its own and the evaluation runs four waves per SIMD; below, the launch costs more than the
	// occupancy gives)
	const bool split = w->collideSplitEnv < 0 ? w->last.nContacts >= 262144 : w->collideSplitEnv != 0;
	DW& d = w->dw;
	forestDrop(w); // (a narrow phase changes the contact array)
	if (int rk = ktBracket(w, 2, 5)) return rk;
	// (shape records staged through LDS where the world holds many distinct ones: b2d_kernels_collide.h)
	// Measured (tools/gpu_collide_variants.py, profiles/r04_collide_variants.txt): on the 1 M-body field (a record per body,
	// circles / boxes / n-gons mixed) staging + sorting a tile by shape-pair class 133 -> 124 us; on the 100 000-box Tumbler
	// (one record, one class) the sort costs 2 % - so both follow the number of distinct records unless the environment says otherwise.
	const bool many = w->shapes.size() > 4096;
	const bool stage = w->collideStage < 0 ? many : w->collideStage != 0;
	// (round 6, measured and left out: sorting also by "the old manifold had points" - the pairs that will run the clipping - to
	// give the one touching contact in six of a dense pile waves of its own: Tumbler 316 3.275 -> 3.338 ms, 1 M field 2.10 -> 2.14)
	const int sort = w->collideSortEnv < 0 ? (many ? 1 : 0) : (w->collideSortEnv != 0 ? 1 : 0);
	// (bit 2: the records of a workgroup's first contact staged in LDS, two staged 4-gons evaluated with unrolled loops -
	// b2d_kernels_collide.h; Tumbler 316: 2.95 -> 2.88 ms. B2HIP_COLLIDE_UNI=0: off, the comparison form of the tests)
	const int uni = w->collideUniOff ? 0 : 4;
	// (the form that stores the compacted contact array itself, b2d_kernels_collide.h: k_collide<0, false, true> - in place of the split
	// form and the three launches behind it, when nothing addresses a contact by its old index afterwards: no TOI candidate
	// alive whose death would be replayed, no PreSolve records, no end events, no other rank. The host must know the contact
	// count - the launch is one workgroup per chunk - and that no candidate is alive: both as of the last read-back, with
	// nothing queued since that changes either.)
	const bool known = w->contactsKnown;
	w->contactsKnown = false;
	bool compact = w->collideCompactOn && split && !stage && sort == 0 && known && w->h_dstate->c.nToiOrder == 0 && w->h_dstate->c.nContacts >= 0 &&
		!d.preSolveOn && !d.eventsOn && !w->spatial && d.shardCount <= 1 && (unsigned)d.capContacts <= TREE_SUM_MAX;
	if (compact)
	{
		hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
		(void)hipStreamIsCapturing(w->stream, &capturing);
		compact = capturing == hipStreamCaptureStatusNone; // (a captured launch would replay its tag)
	}
	const size_t chunks = compact ? ((size_t)w->h_dstate->c.nContacts + w->collideChunk - 1) / w->collideChunk : 0;
	if (compact && (chunks > w->collideCounts.cap || chunks / COLLIDE_GROUP + 1 > w->collideGroups.cap)) compact = false;
	if (compact)
	{
		if (w->collideEpoch >= 0xffffu)
		{
			// (the tag is about to wrap: no word of 65 535 launches ago may read as published - as radixSort's)
			HIP_TRY(hipMemsetAsync(w->collideCounts.p, 0, w->collideCounts.cap * sizeof(unsigned), w->stream));
			HIP_TRY(hipMemsetAsync(w->collideGroups.p, 0, w->collideGroups.cap * sizeof(unsigned), w->stream));
			w->collideEpoch = 0u;
		}
		CollideCompactArgs cc;
		cc.counts = w->collideCounts.p;
		cc.groups = w->collideGroups.p;
		cc.abortWord = w->scanCtx.abortWord;
		cc.tag = ++w->collideEpoch;
		cc.chunk = w->collideChunk;
		w->statCollideCompact += 1;
		// (with the island build's union pass as its tail when an island build follows: b2d_kernels_collide.h. The forest is seeded
		// by a launch of its own - k_step_begin is one wave, and the pass over the bodies belongs to the steps that take this
		// form. The colours are voided there too when the island build will run k_color_check: buildIslands, s.largeHint.)
		if (w->collideUnionOn && w->sp.dt > 0.0f && w->stepSolves)
		{
			const bool voidColors = w->largeHintSteps > 0;
			LAUNCH(w, k_union_seed, gridFor(d.nBodies), 256, d);
			LAUNCH(w, (k_collide<0, false, true, true>), (int)std::max<size_t>(chunks, 1), 256, d, uni, cc, voidColors ? 1 : 0);
			w->forestUnited = true;
			w->forestVoided = voidColors;
		}
		else LAUNCH(w, (k_collide<0, false, true>), (int)std::max<size_t>(chunks, 1), 256, d, uni, cc);
		return ktBracket(w, 2, 5);
	}
	if (stage) LAUNCH(w, (k_collide<1, true>), gridFor(d.capContacts), 256, d, sort);
	else if (split)
	{
		LAUNCH(w, (k_collide<0, false>), gridFor(d.capContacts), 256, d, sort | uni);
		LAUNCH(w, k_toi_order_destroy, 1, 256, d);
	}
	else LAUNCH(w, (k_collide<0, true>), gridFor(d.capContacts), 256, d, sort | uni);
	if (int rk = ktBracket(w, 2, 5)) return rk;
	deviceExclusiveScan<int>(w->stream, d.keepFlag, d.keepScan, d.scanTmp, w->scanCtx, &d.st->c.nContacts, d.capContacts);
	if (d.preSolveOn) LAUNCH(w, k_presolve_gather, gridFor(d.capContacts), 256, d);
	LAUNCH(w, k_compact_contacts, gridFor(d.capContacts), 256, d); // (its last workgroup switches the buffers)
	return 0;
}

int b2hip_debug_hash(b2hip_world* w, int which, uint64_t* out);
static void tracePoint(b2hip_world* w, const char* label)
{
	if (!w->debugTrace) return;
	uint64_t hb = 0, hi = 0;
	(void)b2hip_debug_hash(w, 0, &hb);
	(void)b2hip_debug_hash(w, 3, &hi);
	w->trace.push_back(std::make_pair(std::string(label), hb ^ (hi * 0x9E3779B97F4A7C15ull)));
}
#define TRACE(label) tracePoint(w, label)

// New block partition of the large-island bodies (b2d_kernels_solve_blocks.h): sort by Morton cell, cut the sorted sequence
// where the contact degrees add up to `targetDeg`, then look at the colours and the census again (classes have changed).
static int partitionLargeIslands(b2hip_world* w, int targetDeg)
{
	DW& d = w->dw;
	HIP_TRY(hipMemcpyAsync(&w->d_state.p->c.blkTargetDeg, &targetDeg, sizeof(int), hipMemcpyHostToDevice, w->stream));
	uint64_t* kin = d.pairKey;
	uint64_t* kout = d.pairKey2;
	int2* vin = d.pairProxy;
	int2* vout = d.pairProxy2;
	LAUNCH(w, k_part_keys, gridFor(d.nBodies), 256, d, kin, vin);
	// LSD radix sort: the body-id bits, then the 32 Morton bits (the pair buffers hold at least 8 entries per proxy)
	std::vector<std::pair<int, int>> passes;
	const int idBits = radixBits(d.nBodies + 1);
	radixPasses(0, idBits, passes);
	radixPasses(32, 32, passes);
	const int tilesCap = std::min(d.capPairs / RADIX_TILE + 1, d.nBodies / RADIX_TILE + 2); // (at most every body)
	const int* nPtr = &d.st->c.nLBodies;
	if (int rcs = radixSort(w, kin, kout, vin, vout, nPtr, tilesCap, passes)) return rcs;
	LAUNCH(w, k_part_weights, gridFor(d.nBodies), 256, d, vin, d.pairFirst);
	deviceExclusiveScan<int>(w->stream, d.pairFirst, d.pairRank, d.scanTmp, w->scanCtx, nPtr, d.nBodies);
	LAUNCH(w, k_part_assign, gridFor(d.nBodies), 256, d, vin, d.pairRank);
	LAUNCH(w, k_color_recheck_begin, gridFor(d.nBodies), 256, d);
	LAUNCH(w, k_color_check, gridFor(d.capContacts), 256, d, 0);
	LAUNCH(w, k_color_masks, gridFor(d.nBodies), 256, d);
	LAUNCH(w, k_block_census, 1, 1024, d, (DState*)nullptr);
	return 0;
}

// ---- b2World::Solve (b2World.cpp:1166-1431): island build, census read-back, then the solver tier of each island --------
// phaseSolve is the driver; the stages below hand one SolveStep on. What a stage decides for the rest of the step is written
// there: a recovery, for one, rewrites the colours and the solver choice before the large islands are solved a second time.
struct SolveStep
{
	Counters c;                       // the island census as the host last read it (stages refresh its colour census)
	bool poll = false;                // the census is published to pinned memory and polled (B2HIP_NO_CENSUS_POLL=1: copy + synchronise)
	bool largeHint = false;           // the world has had large islands lately: the island build took the colour census too
	bool exactLarge = false;          // B2HIP_FORCE_LARGE=2: every island through the large-island solver in the reference's order
	bool colorSmallQueued = false;    // k_color_small went out behind the census and has work to do
	bool colorAheadPublished = false; // ... in its no-partition mode: it publishes the state behind it
	bool plainIslands = false;        // no joints, no hub body
	bool blockShape = false;          // the large islands are to have a block partition
	bool hasJoints = false, hasHubs = false; // (hasHubs: anything for k_large_hub)
	bool sideStream = false;          // the small-island chain runs on the side stream ...
	bool smallDeferred = false;       // ... and is still to be launched (behind the large-island solver's first launches)
	int nLIslands = 0, nLBodies = 0, nLContacts = 0, nColors = 0; // what the large-island solver runs over
	bool useBlocks = false;           // k_solve_blocks
	bool useSweep = false;            // k_blocks_sweep (else a launch per colour)
	bool colorsOnDevice = false;      // k_solve_blocks reads the colour count on the device
	bool censusVoid = false;          // colours were handed out afresh: the colour census of this step is history
	bool colorSpill = false;          // some constraint found no free colour this step: it sits in the hub group (k_hub_flag lists it; hasHubs is set with it) and is swept in order
};

static const int RECOLOR_SLACK = 2; // colour afresh when the colours in use exceed the last fresh colouring's by more than this

// The island build, up to the publication of its census (b2dPublishCensus): by k_block_census, by k_island_edges when that is
// the last kernel, else by a launch of its own.
static int buildIslands(b2hip_world* w, const SolveStep& s)
{
	DW& d = w->dw;
	const bool adopt = w->adoptPasses;
	const int pubBy = !s.poll ? 0 : (s.largeHint ? 1 : ((d.nJoints == 0 && !adopt) ? 2 : 3));
	// (the passes over the contacts gather the solid ones of a tile of `solidRounds` x 256 contacts in LDS, b2d_kernels_island.h:
	// tiles as large as leave a thousand workgroups with one each - a lane per contact below 512 000 contacts)
	int solidRounds = 1;
	while (solidRounds < SOLID_TILE_ROUNDS_MAX && (long long)w->last.nContacts >= 2ll * solidRounds * 256 * 1024) solidRounds *= 2;
	if (w->solidRoundsEnv > 0) solidRounds = w->solidRoundsEnv;
	const int gSolid = gridFor((size_t)(d.capContacts + solidRounds - 1) / solidRounds);
	// (the contacts united by this step's narrow phase: the joints only, and k_color_check without its first loop)
	const bool united = w->forestUnited, voided = united && w->forestVoided && s.largeHint;
	forestDrop(w);
	LAUNCH(w, k_island_init, gridFor(d.nBodies), 256, d, united ? 1 : 0);
	if (!united) LAUNCH(w, k_island_union, gSolid, 256, d, solidRounds);
	else
	{
		w->statUnionSkipped += 1;
		if (d.nJoints > 0) LAUNCH(w, k_island_union, gridFor(d.nJoints), 256, d, 0);
	}
	LAUNCH(w, k_island_flatten, gridFor(d.nBodies), 256, d);
	LAUNCH(w, k_island_count, gSolid, 256, d, solidRounds);
	LAUNCH(w, k_island_classify, gridFor(d.nBodies), 256, d, w->forceLarge, w->sp);
	if (d.shardCount > 1 && !d.spatial) LAUNCH(w, k_shard_big, 1, 1024, d); // the big islands of a sharded world, dealt over the ranks
	deviceExclusiveScan<int4>(w->stream, d.rootScanIn, d.rootScanOut, w->scanTmp4.p, w->scanCtx, w->consts.p, d.nBodies);
	if (hipError_t le = hipGetLastError()) return setError(B2HIP_ERR_HIP, std::string("k_scan<int4> launch: ") + hipGetErrorString(le));
	deviceExclusiveScan<int>(w->stream, d.deg, d.adjStart, d.scanTmp, w->scanCtx, w->consts.p, d.nBodies);
	if (d.nJoints > 0) deviceExclusiveScan<int>(w->stream, d.rootJoints, d.rootJointStart, d.scanTmp, w->scanCtx, w->consts.p, d.nBodies);
	LAUNCH(w, k_island_assign, gridFor(d.nBodies), 256, d);
	LAUNCH(w, k_island_edges, gSolid, 256, d, pubBy == 2 ? w->h_pub.dev : (DState*)nullptr, solidRounds);
	// (a growing pile: hand home blocks on to newcomers up to four contacts away instead of partitioning again)
	if (adopt)
		for (int stage = 0; stage < 3; ++stage) LAUNCH(w, k_block_adopt, gridFor(d.capContacts), 256, d, stage);
	if (d.nJoints > 0) LAUNCH(w, k_joints_fill, gridFor(d.nJoints), 256, d);
	// (colour bookkeeping and block census only matter to large islands: skipped while the world has had none lately)
	if (s.largeHint)
	{
		LAUNCH(w, k_color_check, gridFor(d.capContacts), 256, d, voided ? 1 : 0);
		LAUNCH(w, k_color_masks, gridFor(d.nBodies), 256, d);
		LAUNCH(w, k_block_census, 1, 1024, d, pubBy == 1 ? w->h_pub.dev : (DState*)nullptr);
	}
	if (pubBy == 3) LAUNCH(w, k_publish_census, 1, 256, d, w->h_pub.dev);
	return 0;
}

// The host needs the island census to size the solver launches.
static int awaitIslandCensus(b2hip_world* w, SolveStep& s)
{
	DW& d = w->dw;
	int rc = 0;
	if (s.poll)
	{
		w->pubSeq = (w->pubSeq + 1) & 0x3fffffff; // (the device counts its publications the same way: DState::pubCount)
		// what the host would launch next in the usual case (a few new contacts on a settled pile to colour, a colour class to
		// compact) goes behind the census at once and runs while the host is busy with it; the kernel looks at the same
		// counters and returns if the case is another one
		// (round 6: ... and where no partition can be made this step - the large islands are beyond what the block solvers take,
		// the host's own hysteresis in largeIslandPolicy - the queued launch runs too and PUBLISHES what it leaves: the
		// launch-per-colour path polls that instead of a copy + synchronise)
		const int aheadMinRows = s.exactLarge ? 0 : (w->noBlocks ? 1 : (w->blocksTooBig ? 650 * std::max(w->blocksMaxWG, w->sweepMaxWG[2]) : 0));
		if (s.largeHint && !s.exactLarge) { LAUNCH(w, k_color_small, 1, 1024, d, 1, aheadMinRows, w->h_pub2.dev, (w->pubSeq2 + 1) & 0x3fffffff); s.colorSmallQueued = true; }
		rc = awaitCensus(w);
		if (rc == 0)
		{
			const bool settled = b2dPartitionSettled(w->h_dstate->c);
			s.colorAheadPublished = s.colorSmallQueued && b2dColorAheadNoPartition(w->h_dstate->c, aheadMinRows);
			if (s.colorAheadPublished) w->pubSeq2 = (w->pubSeq2 + 1) & 0x3fffffff; // (its publication is on its way, with this number)
			if (!settled && !s.colorAheadPublished) s.colorSmallQueued = false; // (it saw the same and returned)
		}
	}
	else rc = readState(w);
	if (rc) return rc;
	s.c = w->h_dstate->c;
	return 0;
}

// The colour census again, under one class (after a new partition, or without one), and the census read back.
static int recheckColors(b2hip_world* w, SolveStep& s)
{
	DW& d = w->dw;
	LAUNCH(w, k_color_recheck_begin, gridFor(d.nBodies), 256, d);
	LAUNCH(w, k_color_check, gridFor(d.capContacts), 256, d, 0);
	LAUNCH(w, k_color_masks, gridFor(d.nBodies), 256, d);
	LAUNCH(w, k_block_census, 1, 1024, d, (DState*)nullptr);
	if (int rc = readState(w)) return rc;
	s.c = w->h_dstate->c;
	return 0;
}

// What the world carries from step to step about its large islands: whether it has had any lately, whether k_block_adopt runs,
// whether they are too big for the block solvers (the partition is then dissolved), when they are coloured afresh.
static int largeIslandPolicy(b2hip_world* w, SolveStep& s)
{
	DW& d = w->dw;
	Counters& c = s.c;
	const bool exact = s.exactLarge;
	if (c.nLIslands > 0)
	{
		if (!s.largeHint)
		{
			// the first large island after a while: run what was skipped, look again
			LAUNCH(w, k_color_check, gridFor(d.capContacts), 256, d, 0);
			LAUNCH(w, k_color_masks, gridFor(d.nBodies), 256, d);
			LAUNCH(w, k_block_census, 1, 1024, d, (DState*)nullptr);
			if (int rc = readState(w)) return rc;
			c = w->h_dstate->c;
		}
		w->largeHintSteps = 120;
	}
	else if (w->largeHintSteps > 0) w->largeHintSteps -= 1;
	// (newcomers without a home block: from the next step on k_block_adopt hands blocks further, for a while)
	if (c.nOrphanRows > 0) w->adoptSticky = 16; else if (w->adoptSticky > 0) w->adoptSticky -= 1;
	w->adoptPasses = w->adoptSticky > 0 && !(w->blocksTooBig && c.nBlocks == 0); // (no partition, none to come: nobody has a block to hand on)
	s.plainIslands = d.nJoints == 0 && c.maxDegree <= HUB_DEGREE;
	// ---- large islands that no block solver can take: more constraints than the blocks that fit the device together hold
	// (1024-lane blocks of ~750 rows: ~190 000; the settled 100 000-box Tumbler has 350 000). They run launch per colour
	// whatever happens - and a partition would only cost them: it splits the colours into two ranges (interior / cut), 27
	// colours in use where one range needs 18, and every colour is a launch of every sweep (Tumbler: 6.1 -> 5.2 ms per step).
	// So the partition is dissolved (all constraints are one class again, coloured afresh once) until the islands have shrunk.
	const int cap1024 = s.plainIslands ? w->blocksMaxWG : w->sweepMaxWG[2];
	// (round 6: islands with joints / hubs leave the block sweeps much earlier - k_blocks_sweep is a launch per sweep whose
	// cut constraints go from workgroup to workgroup through memory, ~45 us per sweep with 256-lane blocks but ~78 us with the
	// 1024-lane blocks an island above ~60 000 constraints needs, while launch per colour with the top colours as rest
	// rows and the hub in the same launch has come down to ~70 us there: the Tumbler with 10 000 boxes 1.19 ms per step in
	// blocks against 1.45 without, with 22 500 boxes 1.92 against 1.61 (profiles/r06_sweep_blocks_crossover.txt))
	const long long tooBigAt = s.plainIslands ? 800ll * cap1024 : std::min<long long>(800ll * cap1024, w->sweepRowsMax);
	const long long fitsAgainAt = s.plainIslands ? 650ll * cap1024 : std::min<long long>(650ll * cap1024, (long long)w->sweepRowsMax * 13 / 16);
	if (!w->blocksTooBig && cap1024 > 0 && c.nLContacts > tooBigAt) w->blocksTooBig = true;
	else if (w->blocksTooBig && c.nLContacts < fitsAgainAt) w->blocksTooBig = false;
	if (w->blocksTooBig && c.nBlocks > 0 && !exact && !w->noBlocks)
	{
		if (w->tracePartition) fprintf(stderr, "[b2hip] partition dissolved: %d constraints in large islands, %d blocks of %d lanes (room for %d)\n", c.nLContacts, c.nBlocks, c.blkLanes, cap1024);
		const size_t nbAll = w->bodies.size();
		HIP_TRY(hipMemsetAsync(w->b_blk1.p, 0, nbAll * sizeof(int), w->stream));
		HIP_TRY(hipMemsetAsync(w->b_adopt.p, 0, nbAll * sizeof(int), w->stream));
		HIP_TRY(hipMemsetAsync(w->b_adoptStage.p, 0, 3 * nbAll * sizeof(int), w->stream));
		HIP_TRY(hipMemsetAsync(&w->d_state.p->c.nBlocks, 0, sizeof(int), w->stream));
		d.serialOrphans = 0; // (no body has a home block now: nothing is an orphan)
		// the colour census again, under the one class (as after a new partition), then every colour afresh
		if (int rc = recheckColors(w, s)) return rc;
		c.needRecolor = 1;
		s.colorSmallQueued = false;
	}
	// Without a partition every colour is a launch of every sweep, and colours handed out one new contact at a time creep
	// up (24 in use on the settled Tumbler where a colouring from scratch needs 19 - five colours are 0.3 ms of its step):
	// every 64th step the island is coloured afresh.
	// (round 5: ... if they HAVE crept up - more than two colours above what the last colouring from scratch needed; the
	// top colours of a sweep are hops of k_large_rest now, ~2.5 us each, and a colouring from scratch is 5 ms of claim /
	// resolve rounds with read-backs: the settled Tumbler's step 64, 128, ... took 9 - 11 ms against 4)
	if (w->blocksTooBig && !exact && !w->noBlocks && c.nLIslands > 0)
	{
		if (w->recolorCountdown <= 0)
		{
			// (a colouring from scratch lands anywhere between the busiest plain body's degree + 1 and + 8: the measure is the
			// better of what the last one reached and degree + 3, so that a poor one is not kept as the yardstick)
			const int yard = std::min(w->freshColors, c.maxDegreePlain + 3);
			if (w->freshColors <= 0 || c.nColors > yard + RECOLOR_SLACK)
			{
				c.needRecolor = 1;
				s.colorSmallQueued = false;
				w->freshColorsPending = true;
				w->recolorCountdown = 64;
			}
			else w->recolorCountdown = 16;
		}
		w->recolorCountdown -= 1;
	}
	else { w->recolorCountdown = 0; w->freshColors = 0; }
	// (from the next step on: in islands with joints / hubs the constraints of such newcomers are swept in order instead)
	w->serialOrphansNext = (!exact && !w->noBlocks && !w->noSweepBlocks && !w->blocksTooBig && c.nBlocks > 0 && (d.nJoints > 0 || c.maxDegree > HUB_DEGREE)) ? 1 : 0;
	return 0;
}

// ---- block partition of the large islands: (re)made when bodies without a home block joined, when a block outgrew a
// workgroup, or when too many constraints cross block boundaries (the pile has moved since the partition was made)
// (islands with joints or hub bodies are partitioned too: k_blocks_sweep does their contact sweeps block-wise, one launch
// per sweep, between the joint walks and the hub sweeps)
static int repartition(b2hip_world* w, SolveStep& s)
{
	const StepParams& sp = w->sp;
	Counters& c = s.c;
	s.blockShape = !s.exactLarge && !w->noBlocks && !w->blocksTooBig && c.nLIslands > 0 && (s.plainIslands || !w->noSweepBlocks) &&
		(sp.warmStarting ? 1 : 0) + sp.velIters > 0 && w->blocksMaxWG > 0;
	if (!s.blockShape || c.partitionCooldown != 0) return 0;
	// Block size: one 1024-lane block while the large islands fit it (nothing ever goes through memory then), else
	// 256-lane blocks (measured on the 10 011-box pyramid: 215 us against 235 / 245 us with 512 / 1024 lanes - the
	// workgroup barriers of the interior colours are cheaper and the position solves spread over more CUs)
	// (512 lanes once 256-lane blocks would be more than fit the device together)
	// (... and 1024 again once 512-lane blocks would not)
	auto lanesFor = [w](const Counters& k) { return w->blockLanes ? w->blockLanes : (k.nLContacts <= 900 ? 1024 : (k.nLContacts > 400 * w->blocksMaxWG ? 1024 : (k.nLContacts > 200 * w->blocksMaxWG ? 512 : 256))); };
	auto misfit = [](const Counters& k) { return k.nBlocks == 0 || k.nOrphanRows > 0 || k.blkMaxRows > k.blkLanes || k.blkMaxBodies > k.blkLanes || k.nSerialOrphans > 2048; };
	bool need = misfit(c) || (c.partitionAge > 240 && (4 * c.nCutRows > c.nLContacts || (c.blkLanes != lanesFor(c) && 2 * c.nLContacts < 900)));
	int lanes = lanesFor(c);
	int target = BLOCK_TARGET_DEG * lanes / BLOCK_LANES;
	// (the last partition did not last - a growing pile: leave the blocks room for the bodies they will adopt, if half as
	// many blocks again still fit the device together)
	{
		const int cap = s.plainIslands ? w->blocksMaxWG : (lanes == 512 ? w->sweepMaxWG[1] : (lanes == BLOCK_LANES ? w->sweepMaxWG[2] : w->sweepMaxWG[0]));
		if (c.nBlocks > 0 && c.partitionAge < 16 && c.nBlocks * 3 / 2 + 8 <= cap) target = target * 2 / 3;
		if (w->tracePartition) fprintf(stderr, "[b2hip] capacity for %d-lane blocks: %d\n", lanes, cap);
	}
	for (int attempt = 0; need && attempt < 3; ++attempt)
	{
		if (w->tracePartition)
			fprintf(stderr, "[b2hip] partition (attempt %d, target %d, lanes %d): blocks %d orphan rows %d max rows %d max bodies %d lanes %d age %d cut %d of %d\n",
				attempt, target, lanes, c.nBlocks, c.nOrphanRows, c.blkMaxRows, c.blkMaxBodies, c.blkLanes, c.partitionAge, c.nCutRows, c.nLContacts);
		HIP_TRY(hipMemcpyAsync(&w->d_state.p->c.blkLanes, &lanes, sizeof(int), hipMemcpyHostToDevice, w->stream));
		if (int rc = partitionLargeIslands(w, target)) return rc;
		s.colorSmallQueued = false; // (the colours are checked against the new partition: what is open after that is new work)
		if (int rc = readState(w)) return rc;
		c = w->h_dstate->c;
		need = misfit(c);
		target = target * 2 / 3;
	}
	if (need)
	{
		// does not fit (e.g. more blocks than workgroups can be resident): back to the other solvers for a while
		const int cooldown = 120;
		HIP_TRY(hipMemcpyAsync(&w->d_state.p->c.partitionCooldown, &cooldown, sizeof(int), hipMemcpyHostToDevice, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
	}
	return 0;
}

// The launches of the small-island chain (DFS order, chunking, k_solve_small) on `ss`: the main stream or the side stream.
static int launchSmallIslands(b2hip_world* w, const SolveStep& s, hipStream_t ss)
{
	DW& d = w->dw;
	const StepParams& sp = w->sp;
	const Counters& c = s.c;
	if (s.sideStream && !s.poll) HIP_TRY(hipStreamWaitEvent(ss, w->evFork, 0));
	LAUNCH_ON(w, ss, k_island_dfs, gridFor(c.nSIslands, 64, 1 << 20), 64, d);
	if (!s.sideStream) stampPhase(w, 5);
	if (!s.exactLarge)
	{
		const bool timeIt = w->kernelTiming == 1 && c.nLIslands == 0;
		if (timeIt) { int rck = ktRecord(w); if (rck) return rck; w->ktKind = 2; }
		if (c.nSmallJointed > 0)
		{
			if (c.chunkLanes == TINY_CHUNK_LANES) LAUNCH_ON(w, ss, (k_solve_small<TINY_CHUNK_LANES, true>), c.nChunks, TINY_CHUNK_LANES, d, sp);
			else LAUNCH_ON(w, ss, (k_solve_small<SMALL_CHUNK_LANES, true>), c.nChunks, SMALL_CHUNK_LANES, d, sp);
		}
		else if (c.chunkLanes == TINY_CHUNK_LANES) LAUNCH_ON(w, ss, (k_solve_small<TINY_CHUNK_LANES, false>), c.nChunks, TINY_CHUNK_LANES, d, sp);
		else LAUNCH_ON(w, ss, (k_solve_small<SMALL_CHUNK_LANES, false>), c.nChunks, SMALL_CHUNK_LANES, d, sp);
		if (timeIt) { int rck = ktRecord(w); if (rck) return rck; }
	}
	if (s.sideStream) HIP_TRY(hipEventRecord(w->evJoin, ss));
	else stampPhase(w, 6);
	return 0;
}

// Small and large islands share nothing (different bodies, contacts, island tables): when both tiers are present the
// small-island chain runs on a side stream beside the large-island solver and joins before SynchronizeFixtures. With a
// handful of small islands that chain is one or two workgroups of big kernels whose cost is instruction fetch from a cold
// cache (~2 us per KB of code executed: 83 us for a dozen free bodies next to the 10k-body pyramid) - time the large
// solver's resident grid leaves plenty of idle CUs for.
// (On the side stream the launches are issued AFTER the large-island solver's own first launches - the solver is what the
// step waits for, and every launch the host makes first delays it by ~3 us: s.smallDeferred.)
static int solveSmallIslands(b2hip_world* w, SolveStep& s)
{
	if (s.c.nSIslands == 0)
	{
		stampPhase(w, 5);
		stampPhase(w, 6);
		return 0;
	}
	s.sideStream = !s.exactLarge && s.c.nLIslands > 0 && !w->debugTrace && !w->kernelTimingLaunches && !w->noSideStream;
	if (!s.sideStream) return launchSmallIslands(w, s, w->stream);
	// fork here (the side stream needs the island build, nothing of the large-island solver); launches later.
	// With the census polled the host has SEEN the island build finish (the publication is its last act): the side
	// stream needs no event to wait for - an event record is a packet of its own on the main stream, ~6 us between
	// the colouring and the solver
	if (!s.poll) HIP_TRY(hipEventRecord(w->evFork, w->stream));
	s.smallDeferred = true;
	stampPhase(w, 5);
	stampPhase(w, 6);
	return 0;
}

static int launchDeferredSmallIslands(b2hip_world* w, SolveStep& s)
{
	if (!s.smallDeferred) return 0;
	s.smallDeferred = false;
	return launchSmallIslands(w, s, w->stream2);
}

// What the large-island solver runs over: the census's large islands, or in exact-order mode every island, with the
// dependency levels of the reference's own constraint order as colours.
static int sizeLargeIslands(b2hip_world* w, SolveStep& s)
{
	DW& d = w->dw;
	const Counters& c = s.c;
	s.nLIslands = c.nLIslands;
	s.nLBodies = c.nLBodies;
	s.nLContacts = c.nLContacts;
	if (!s.exactLarge || c.nSIslands == 0) return 0;
	LAUNCH(w, k_exact_begin, gridFor(c.nSContacts + 1), 256, d);
	LAUNCH(w, k_exact_convert, gridFor(std::max(c.nSContacts, c.nSBodies)), 256, d);
	if (int rc = readState(w)) return rc;
	s.nColors = w->h_dstate->c.nColors;
	s.nLIslands = c.nSIslands;
	s.nLBodies = c.nSBodies;
	s.nLContacts = c.nSContacts;
	return 0;
}

// The solver of the large islands: k_solve_blocks (bodies in LDS, one workgroup per block of the partition) whenever the
// partition fits; k_blocks_sweep (one launch per sweep over the same blocks) for islands that need joint walks / hub
// sweeps in between; else a launch per colour.
static void chooseLargeSolver(b2hip_world* w, SolveStep& s)
{
	const StepParams& sp = w->sp;
	const Counters& c = s.c;
	const bool partitionFits = s.blockShape && c.nBlocks > 0 && c.nOrphanRows == 0 && c.blkMaxRows <= c.blkLanes && c.blkMaxBodies <= c.blkLanes;
	s.useBlocks = !s.exactLarge && s.plainIslands && !s.hasHubs && !w->debugTrace && !w->kernelTimingLaunches && partitionFits &&
		c.nBlocks <= w->blocksMaxWG && (sp.velIters + 2) * (MAX_COLORS + 1) < 65536 && (sp.posIters + 1) * (MAX_COLORS + 1) < 65536;
	const int sweepMaxWG = c.blkLanes == 512 ? w->sweepMaxWG[1] : (c.blkLanes == BLOCK_LANES ? w->sweepMaxWG[2] : w->sweepMaxWG[0]);
	s.useSweep = !s.useBlocks && !s.exactLarge && partitionFits && !s.plainIslands && !w->debugTrace && !w->kernelTimingLaunches &&
		c.nBlocks <= sweepMaxWG;
	w->dw.blockSort = (s.useBlocks || s.useSweep) ? 1 : 0;
}

// The grid-wide colouring rounds (k_color_claim / k_color_resolve) until every constraint has a colour: `batch` rounds
// before the first read-back, eight between the later ones.
static int colorRoundsUntilDone(b2hip_world* w, SolveStep& s, int uncolored, int batch)
{
	DW& d = w->dw;
	const int gC = gridFor(std::max(s.nLContacts, 1));
	for (; uncolored > 0; batch = 8)
	{
		for (int r = 0; r < batch; ++r)
		{
			LAUNCH(w, k_color_claim, gC, 256, d);
			LAUNCH(w, k_color_resolve, gC, 256, d);
		}
		if (int rc = readState(w)) return rc;
		uncolored = w->h_dstate->c.nUncolored;
		s.nColors = w->h_dstate->c.nColors;
		if (w->h_dstate->c.overflow & 4) { if (!w->recoverOn) return setError(B2HIP_ERR_CAPACITY, "more than 64 constraint colours on one body"); s.colorSpill = s.hasHubs = true; }
	}
	return 0;
}

// Colours for the constraints of the large islands that have none (or all of them afresh).
static int colorLargeIslands(b2hip_world* w, SolveStep& s)
{
	DW& d = w->dw;
	Counters& c = s.c;
	if (s.exactLarge || !(c.needRecolor || c.nUncolored > 0 || c.nCompact > 0)) return 0;
	bool roundsToo = c.needRecolor || c.nUncolored > COLOR_SMALL_MAX; // the grid-wide rounds run (asked for by the census, or to finish what k_color_small left)
	if (!roundsToo)
	{
		// the usual case (a few new contacts on a settled island, a colour class to compact): one workgroup colours them;
		// k_solve_blocks reads the colour count from the device, the launch-per-colour path needs it: published by the
		// kernel and polled - a copy + synchronise otherwise, B2HIP_NO_CENSUS_POLL=1
		const bool pubColors = s.poll && !s.useBlocks;
		if (!s.colorSmallQueued)
		{
			if (pubColors) w->pubSeq2 = (w->pubSeq2 + 1) & 0x3fffffff;
			LAUNCH(w, k_color_small, 1, 1024, d, 0, 0, pubColors ? w->h_pub2.dev : (DState*)nullptr, w->pubSeq2); // (else: it went out behind the census)
		}
		if (s.useBlocks)
		{
			s.colorsOnDevice = true;
			w->colorSmallPending = true;
			return 0;
		}
		int rc;
		if ((s.colorSmallQueued && s.colorAheadPublished) || (!s.colorSmallQueued && pubColors))
		{
			rc = awaitColors(w);
			if (rc == 0) c.nColors = w->h_dstate->c.nColors;
			if (rc == 0) memcpy(c.colorRows, w->h_dstate->c.colorRows, sizeof(c.colorRows));
		}
		else rc = readState(w);
		if (rc) return rc;
		s.nColors = w->h_dstate->c.nColors;
		// (round 6: neither ends the step any more. A constraint without a free colour on its two bodies is swept in order
		// with the hub rows - k_hub_flag; rounds that did not converge are finished by the grid-wide rounds below)
		if (w->h_dstate->c.overflow & 4) { if (!w->recoverOn) return setError(B2HIP_ERR_CAPACITY, "more than 64 constraint colours on one body"); s.colorSpill = s.hasHubs = true; }
		if (w->h_dstate->c.nUncolored == 0) return 0;
		if (!w->recoverOn) return setError(B2HIP_ERR_CAPACITY, "incremental colouring did not converge");
		c.nUncolored = w->h_dstate->c.nUncolored;
		w->colorRecoveries += 1;
		if (w->traceRecovery) fprintf(stderr, "[b2hip] k_color_small left %d constraints without a colour: the grid-wide rounds finish\n", c.nUncolored);
	}
	// a colour clash on some body -> colour the large islands from scratch; otherwise only the constraints that have no
	// colour yet join the Jones-Plassmann rounds (existing masks stay)
	s.censusVoid = true; // (thousands of constraints get their colours now: the colour census of this step is history)
	int uncolored = c.nUncolored;
	if (c.needRecolor)
	{
		LAUNCH(w, k_color_begin, gridFor(d.capContacts), 256, d);
		uncolored = s.nLContacts; // upper bound (hub constraints excluded on the device); refreshed by the read-back
	}
	if (int rc = colorRoundsUntilDone(w, s, uncolored, c.needRecolor ? 8 : 2)) return rc;
	if (w->freshColorsPending) { w->freshColors = s.nColors < 63 ? s.nColors : 63; w->freshColorsPending = false; }
	return 0;
}

// The hand-over rows of k_solve_blocks / k_blocks_sweep / k_large_rest / k_rest_hub carry a 15-bit epoch of their launch
// (w->dfEpoch): they are wiped whenever it comes round, so that a row nobody has written since cannot carry a matching tag.
static int wipeHandoverRows(b2hip_world* w)
{
	if ((w->dfEpoch >> 14) == w->dfWipedAt) return 0;
	HIP_TRY(hipMemsetAsync(w->b_cutv.p, 0, w->b_cutv.cap * sizeof(float4), w->stream));
	HIP_TRY(hipMemsetAsync(w->b_posv.p, 0, w->b_posv.cap * sizeof(float4), w->stream));
	w->dfWipedAt = w->dfEpoch >> 14;
	return 0;
}

// Every decision of one pass of the large-island solve, made before its first launch (planLargePass) and read by the stages
// of LargePass: none depends on what a launch of the pass produces.
struct LargePlan
{
	bool safe = false;            // the second pass of a recovered step: no rest flow, no snapshot, no timing-mode-5 record
	bool useSweepEnd = false;     // sweeps end in k_sweep_end / k_rest_hub (else k_large_hub, k_large_joints, k_large_pos_end apart)
	int restFirst = 0x7fffffff;   // colours [restFirst, nColors) are the rest colours of k_large_rest (0x7fffffff: none)
	long long restRows = 0;       // an upper bound of their rows: sizes the grids of k_large_rest and k_rest_hub
	bool useRest = false;         // there are rest colours (only where the rows lie by colour: never beside k_blocks_sweep)
	int tailFirst = 0;            // colours [tailFirst, nColors) are swept inside k_sweep_end (the rest colours' start with useRest)
	bool tailAny = false;         // ... and one of them owns a constraint
	int bigEnd = 0;               // colours [0, bigEnd) are launches of their own
	bool leftoverApart = false;   // the hub rows behind the fixed point go to k_large_hub between two launches of k_sweep_end
	bool fuseHub = false;         // k_large_rest and k_sweep_end of one sweep as ONE launch, k_rest_hub
	bool bodyWarm = false;        // the warm start body by body in one launch, k_large_warm
	bool hubBuildOne = false;     // the hub list by one launch of k_hub_build (else k_hub_flag, scan, k_hub_fill, k_hub_order)
	bool sortInIntegrate = false; // k_large_integrate sorts the joints of every island too (else k_joints_sort apart)
	bool afterFused = false;      // k_large_after_velocity (else impulses stored, positions integrated, k_large_pos_begin apart)
	bool censusGrid = false;      // colour launches are sized from this step's colour census (else all alike: gK)
	uint64_t colorMask = ~0ull;   // bit per colour below 64: it owns a constraint
	int gB = 0, gC = 0, gJ = 0;   // grids over the large islands' bodies, their contacts, the islands themselves (joint walks)
	int gK = 0;                   // grid of a colour launch sized from the mean colour
	bool waitsBetweenWorkgroups = false; // the pass uses a kernel whose workgroups wait for one another: snapshot before, look behind
};

static inline bool colorUsed(const LargePlan& p, int col) { return col >= 64 || ((p.colorMask >> col) & 1ull) != 0; }

// The plan of one pass from the step, the switches and the census the host holds. Launches nothing. `safe`: the pass that
// follows a recovery (recoverLarge has taken the solver choice back to a launch per colour).
static LargePlan planLargePass(const b2hip_world* w, const SolveStep& s, const bool safe)
{
	const DW& d = w->dw;
	const StepParams& sp = w->sp;
	const Counters& c = s.c;
	const int nColors = s.nColors;
	LargePlan p;
	p.safe = safe;
	p.gB = gridFor(s.nLBodies);
	p.gC = gridFor(std::max(s.nLContacts, 1));
	p.gJ = gridFor(std::max(s.nLIslands, 1), 64, 1 << 16);
	p.useSweepEnd = w->sweepEnd && !s.exactLarge && !w->debugTrace;
	// ---- the end of every sweep without a launch per colour (b2d_kernels_sweep_end.h). The REST colours - from the highest
	// colour down while this step's colour census (k_color_check, published with the island census) keeps them below
	// restRowsMax rows together - are swept by ONE launch of k_large_rest, as data flow per body; k_color_fill notes them
	// on their bodies. Which colours are "rest" changes nothing in the result (the order on every body is the launches'):
	// a launch-count matter. Not on a step that colours afresh: its census is void.
	if (p.useSweepEnd && w->restFlow && !safe && !d.blockSort && !c.needRecolor && !s.censusVoid && nColors > 0 && nColors < MAX_COLORS)
	{
		long long sum = 0;
		int t = nColors;
		while (t > 0 && sum + c.colorRows[t - 1] <= (long long)w->restRowsMax)
		{
			sum += c.colorRows[t - 1];
			t -= 1;
		}
		if (nColors - t >= 2) p.restFirst = t;
	}
	// (the census is this step's before k_color_small handed out its colours - at most COLOR_SMALL_MAX rows more)
	p.restRows = COLOR_SMALL_MAX;
	for (int col = p.restFirst; col < nColors && col < MAX_COLORS; ++col) p.restRows += c.colorRows[col];
	p.useRest = p.useSweepEnd && p.restFirst < nColors;
	// (round 6: one single-workgroup launch sorts the hub group's segment of the row array in place - k_hub_build - where the
	// last step's list was short enough for its keys to sit in LDS; the four launches of layoutRows otherwise)
	// (... and on a step with constraints that found no colour free, however long the list: k_hub_flag hands the scan TWO counts
	// in one int - the rows of the fixed point below bit 20, everything else above it - so k_hub_fill places at most 2 047 rows
	// behind the wide ones; orphans are held below that by repartition()'s misfit, rows without a colour are not.
	// tests/test_gpu_large_plan.py, Tumbler 60 with two colours per range: 4 370 of them. k_hub_build has no such limit.
	// With the fixed point on, the rows of every hub but the primary one are behind the wide ones too: a world that had more than
	// 1 024 such rows in the last step - the census still carries its counts - stays with k_hub_build as well.)
	const bool manyBehindWide = d.hubWide && c.nHubRows - c.nHubWide > 1024;
	p.hubBuildOne = s.hasHubs && !w->noHubBuild && (w->last.nHubRows <= HUB_BUILD_LDS || s.colorSpill || manyBehindWide);
	p.gK = gridFor(std::max(s.nLContacts / std::max(nColors, 1), 1) * 2);
	// A colour launch is a chain of dependent loads per lane (~4.5 us whatever it holds): a lane that makes a second trip
	// of the grid-stride loop pays the chain twice - the Tumbler's five biggest colours (41 000 - 42 000 rows against a grid
	// of 39 000 lanes sized from the MEAN colour) took 8 us instead of 6. Sized per colour from this step's census now
	// (+ what k_color_small may still add), in workgroups of 256 lanes so that the rows spread over all CUs.
	p.censusGrid = !s.exactLarge && nColors > 0 && nColors <= MAX_COLORS && !c.needRecolor && !s.censusVoid;
	p.waitsBetweenWorkgroups = s.useBlocks || s.useSweep || p.useRest;
	p.sortInIntegrate = s.hasJoints && !s.exactLarge && !w->debugTrace;
	// (the warm start body by body in one launch - k_large_warm - where the sweep would be a launch per colour: k_large_init
	// leaves the deltas for it)
	p.bodyWarm = w->bodyWarm && w->sweepEnd && !s.exactLarge && !w->debugTrace && !s.useSweep && sp.warmStarting && nColors <= MAX_COLORS;
	// colours that own no constraint (the partition keeps two colour ranges apart) are not launched
	// (the mask of the host's LAST copy: s.c can be an older one once the colours were awaited)
	p.colorMask = s.exactLarge ? ~0ull : ((uint64_t)w->h_dstate->c.colorMaskLo | ((uint64_t)w->h_dstate->c.colorMaskHi << 32));
	// ---- the end of every sweep in ONE single-workgroup launch (b2d_kernels_sweep_end.h): the tail colours - those this
	// step's colour census (k_color_check, published with the island census) found small, from the highest colour down -
	// the hub rows, the joint walk, the verdict of a position iteration. Which colours are "tail" changes nothing in the
	// result (k_sweep_end does k_large_velocity's / k_large_position's arithmetic row for row): a pure launch-count matter.
	p.tailFirst = p.useRest ? p.restFirst : nColors;
	if (p.useSweepEnd && w->sweepTail && !p.useRest && !s.useSweep && !c.needRecolor && !s.censusVoid && nColors <= MAX_COLORS)
	{
		long long sum = 0;
		while (p.tailFirst > 0 && c.colorRows[p.tailFirst - 1] <= w->tailRowsMax && sum + c.colorRows[p.tailFirst - 1] <= 8ll * w->tailRowsMax)
		{
			sum += c.colorRows[p.tailFirst - 1];
			p.tailFirst -= 1;
		}
	}
	for (int col = p.tailFirst; col < nColors && !p.useRest; ++col) p.tailAny = p.tailAny || colorUsed(p, col);
	p.bigEnd = s.useSweep ? 0 : p.tailFirst;
	// The hub rows the one fixed point cannot take are swept lane after lane inside k_sweep_end - a handful on the Tumbler
	// (boxes in the corners). An island that kept many of them in the LAST step (several hubs, constraints swept in order for
	// lack of a home block; the census still carries that step's counts) gets k_large_hub's eight prefetching waves for
	// them: k_sweep_end up to the fixed point, k_large_hub, k_sweep_end for what follows the hub rows. (Either way a valid
	// sweep; which one is decided from counters a snapshot carries, so a loaded world decides alike.)
	p.leftoverApart = p.useSweepEnd && s.hasHubs && d.hubWide && c.nHubRows - c.nHubWide > SE_LEFT_INLINE_MAX;
	// ---- k_large_rest and k_sweep_end of one sweep as ONE launch (k_rest_hub, round 6): the rest rows in gF workgroups of
	// 512 lanes, the hub rows / joints / verdict in one more that waits for what it needs of them as tagged rows. All
	// workgroups must be resident together (restHubMaxWG: the occupancy query at world creation).
	p.fuseHub = p.useRest && w->restHub && (s.hasHubs || s.hasJoints) && !p.leftoverApart && w->restHubMaxWG > 1;
	// (one launch for the three: k_large_after_velocity; apart where a trace wants to see each)
	p.afterFused = !w->debugTrace && sp.posIters > 0;
	return p;
}

static inline int gridOfColor(const SolveStep& s, const LargePlan& p, int col)
{
	if (!p.censusGrid || col < 0 || col >= MAX_COLORS) return p.gK;
	return gridFor((size_t)s.c.colorRows[col] + 512, 256, 1 << 16);
}

// ---- the row layout and the solver proper, as ONE unit that can run a second time in its SAFE form (round 6, VERDICT r05
// item 5): b2World::Step has no failure path (b2World.cpp:1613-1710), and a wait between workgroups that times out - a
// co-tenant on the device, a workgroup that was not resident - used to fail the step and leave a dead world. The unit
// saves what the solver changes (k_solver_snapshot: rows of the large islands' bodies, impulses and flags of their
// contacts, their joints) before its first solver launch; behind its last one a one-lane kernel publishes the overflow
// word, the host looks at it (a poll of mapped memory: ~5 us with the next launch's latency - only where the unit used a
// kernel whose workgroups wait for one another), and on a timed-out wait puts the saved state back and runs the unit
// again on the plain path: rows by colour, a launch per colour, tail colours and hub rows in k_sweep_end's ONE workgroup -
// nothing in it waits for another workgroup. Same colouring, same arithmetic, same order on every body: the bits the
// fast path would have produced (tests/test_gpu_recovery.py).
// One pass over (w, s, plan): a dispatch per kernel family - from a run-time lane count / mode to the instantiation - and the
// stages in the order of b2Island::Solve (b2Island.cpp:256-336); run() is the unit.
struct LargePass
{
	b2hip_world* const w;
	SolveStep& s;
	const LargePlan p;
	DW& d;
	const StepParams& sp;
	LargePass(b2hip_world* w_, SolveStep& s_, bool safe) : w(w_), s(s_), p(planLargePass(w_, s_, safe)), d(w_->dw), sp(w_->sp) {}

	// Every launch of k_solve_blocks / k_blocks_sweep / k_large_rest / k_rest_hub tags its hand-over rows with an epoch of its own.
	template <typename Launch>
	int withEpoch(Launch launch)
	{
		if (int rc = wipeHandoverRows(w)) return rc;
		if (int rc = launch()) return rc;
		w->dfEpoch += 1;
		return 0;
	}

	// k_blocks_sweep in `mode` (0 warm start, 1 velocity, 2 position) over the blocks of the partition; WHOLE_SOLVE: k_solve_blocks,
	// the whole sweep structure in one resident grid. (The compiler emits the instantiations in the order the dispatches name
	// them first - here k_solve_blocks<512, 256, 1024>, then k_blocks_sweep's: a reordered ladder moves kernels in the code object.)
	static const int WHOLE_SOLVE = -1;
	int launchBlocks(int mode)
	{
		const Counters& c = s.c;
		return withEpoch([&]() -> int
		{
			if (mode == WHOLE_SOLVE && c.blkLanes == 512) LAUNCH(w, k_solve_blocks<512>, c.nBlocks, 512, d, sp, w->gridBar.p, w->dfEpoch);
			else if (mode == WHOLE_SOLVE && c.blkLanes == 256) LAUNCH(w, k_solve_blocks<256>, c.nBlocks, 256, d, sp, w->gridBar.p, w->dfEpoch);
			else if (mode == WHOLE_SOLVE && c.blkLanes == BLOCK_LANES) LAUNCH(w, k_solve_blocks<BLOCK_LANES>, c.nBlocks, BLOCK_LANES, d, sp, w->gridBar.p, w->dfEpoch);
			else if (mode != WHOLE_SOLVE && c.blkLanes == 512) LAUNCH(w, k_blocks_sweep<512>, c.nBlocks, 512, d, sp, mode, w->gridBar.p, w->dfEpoch);
			else if (mode != WHOLE_SOLVE && c.blkLanes == 256) LAUNCH(w, k_blocks_sweep<256>, c.nBlocks, 256, d, sp, mode, w->gridBar.p, w->dfEpoch);
			else if (mode != WHOLE_SOLVE && c.blkLanes == BLOCK_LANES) LAUNCH(w, k_blocks_sweep<BLOCK_LANES>, c.nBlocks, BLOCK_LANES, d, sp, mode, w->gridBar.p, w->dfEpoch);
			else return setError(B2HIP_ERR_INVALID, "block partition made for an unknown workgroup size");
			return 0;
		});
	}

	// the hub sweeps: eight waves that fetch their chunks of hub constraints ahead of their turn (one wave on request)
	int launchHub(int mode, int useGuess, int behindWide)
	{
		if (w->hubWaves == 1) LAUNCH(w, k_large_hub<1>, 1, 64, d, mode, useGuess, behindWide);
		else LAUNCH(w, k_large_hub<8>, 1, 512, d, mode, useGuess, behindWide);
		return 0;
	}

	// The rest colours of one sweep as data flow per body.
	int launchRest(int mode)
	{
		int gR = (int)((p.restRows + 255) / 256);
		// (the workgroups wait for one another: no more of them than are resident together - the rest walk in strides)
		if (w->restMaxWG > 0) gR = std::min(gR, w->restMaxWG);
		return withEpoch([&]() -> int
		{
			if (mode == 0) LAUNCH(w, k_large_rest<0>, gR, 256, d, p.restFirst, s.nColors, w->gridBar.p, w->dfEpoch);
			else if (mode == 1) LAUNCH(w, k_large_rest<1>, gR, 256, d, p.restFirst, s.nColors, w->gridBar.p, w->dfEpoch);
			else LAUNCH(w, k_large_rest<2>, gR, 256, d, p.restFirst, s.nColors, w->gridBar.p, w->dfEpoch);
			return 0;
		});
	}

	// Tail colours [tf, te) and what follows them (`what`: SE_*), in one workgroup.
	int launchSweepEnd(int mode, int tf, int te, int what)
	{
		if (mode == 0) LAUNCH(w, k_sweep_end<0>, 1, SWEEP_END_LANES, d, sp, tf, te, what, w->sweepStamps ? w->gridBar.p : (int*)nullptr);
		else if (mode == 1) LAUNCH(w, k_sweep_end<1>, 1, SWEEP_END_LANES, d, sp, tf, te, what, w->sweepStamps ? w->gridBar.p : (int*)nullptr);
		else LAUNCH(w, k_sweep_end<2>, 1, SWEEP_END_LANES, d, sp, tf, te, what, w->sweepStamps ? w->gridBar.p : (int*)nullptr);
		return 0;
	}

	// The rest colours and the end of the sweep in one launch (velocity and position sweeps only).
	int launchRestHub(int mode, int what)
	{
		// (a grid that does not hold every row walks them in strides)
		int gF = (int)((p.restRows + SWEEP_END_LANES - 1) / SWEEP_END_LANES);
		gF = std::max(1, std::min(gF, w->restHubMaxWG - 1));
		return withEpoch([&]() -> int
		{
			if (mode == 2) w->restArrived += gF; // (the verdict of a position iteration waits for them: bar[5])
			if (mode == 1) LAUNCH(w, k_rest_hub<1>, gF + 1, SWEEP_END_LANES, d, sp, p.restFirst, s.nColors, what, w->gridBar.p, w->dfEpoch, w->restArrived, w->sweepStamps ? w->gridBar.p : (int*)nullptr);
			else LAUNCH(w, k_rest_hub<2>, gF + 1, SWEEP_END_LANES, d, sp, p.restFirst, s.nColors, what, w->gridBar.p, w->dfEpoch, w->restArrived, (int*)nullptr);
			return 0;
		});
	}

	// The rows of the large islands by colour (unless the block solvers sort their own), rest colours noted on their bodies,
	// the hub group's rows listed in order.
	int layoutRows()
	{
		if (!d.blockSort) LAUNCH(w, k_color_scan, 1, 64, d); // (segments by colour: the block solvers sort their rows themselves)
		LAUNCH(w, k_color_fill, p.gC, 256, d, p.restFirst < MAX_COLORS ? p.restFirst : MAX_COLORS);
		if (!s.hasHubs) return 0;
		const int order = (!w->noHubOrder && (d.hubWide || w->hubOrderAll)) ? 1 : 0;
		if (p.hubBuildOne) LAUNCH(w, k_hub_build, 1, 1024, d, d.hubWide ? 1 : 0, order, d.blockSort ? 1 : 0);
		else
		{
			// the hub constraints in contact-index order (deterministic whatever the atomics of k_color_fill did)
			LAUNCH(w, k_hub_flag, gridFor(d.capContacts), 256, d);
			deviceExclusiveScan<int>(w->stream, d.keepFlag, d.keepScan, d.scanTmp, w->scanCtx, &d.st->c.nContacts, d.capContacts);
			LAUNCH(w, k_hub_fill, gridFor(d.capContacts), 256, d);
			// (the hub meets its partners in the order of their highest colour: b2d_kernels_solve_large.h, k_hub_order)
			if (order) LAUNCH(w, k_hub_order, 1, 1024, d, d.hubWide ? 0 : 1);
		}
		w->hubSteps += 1;
		return 0;
	}

	// one resident grid for the whole sweep structure; colour boundaries are barriers inside the blocks, the cut rows
	// hand-overs between them (b2d_kernels_solve_blocks.h)
	int solveResident()
	{
		int rc = 0;
		if (w->kernelTiming == 1) { rc = ktRecord(w); if (rc) return rc; w->ktKind = 4; }
		if ((rc = launchBlocks(WHOLE_SOLVE))) return rc;
		w->blockSteps += 1;
		w->blocksThisStep = true;
		if (w->kernelTiming == 1) { rc = ktRecord(w); if (rc) return rc; }
		return launchDeferredSmallIslands(w, s);
	}

	// b2Island.cpp:193-254: velocities integrated, joints in their order, the constraints of the contacts set up.
	int setUp()
	{
		TRACE("before_integrate");
		if (w->debugTrace)
		{
			const size_t nb = w->bodies.size();
			(void)w->dbgPreVel.ensure(nb, w->stream); (void)w->dbgVel.ensure(nb, w->stream); (void)w->dbgLi.ensure(nb + 64, w->stream);
			HIP_TRY(hipMemcpyAsync(w->dbgPreVel.p, w->b_vel.p, nb * 16, hipMemcpyDeviceToDevice, w->stream));
			HIP_TRY(hipMemcpyAsync(w->dbgLi.p, w->li_bodies.p, nb * 4, hipMemcpyDeviceToDevice, w->stream));
			HIP_TRY(hipMemcpyAsync(w->dbgLi.p + nb, &w->d_state.p->c, 64 * 4 > sizeof(Counters) ? sizeof(Counters) : 64 * 4, hipMemcpyDeviceToDevice, w->stream));
		}
		// (timing mode 5: ONE event pair around the whole large-island solver family of the launch-per-colour path - integrate,
		// constraint set-up, every sweep, impulses stored, positions, write-back and sleep)
		if (w->kernelTiming == 5 && !p.safe) { int rc = ktRecord(w); if (rc) return rc; w->ktKind = 8; w->familyLaunchesAtStart = w->launchCount; }
		LAUNCH(w, k_large_integrate, p.gB, 256, d, sp, p.sortInIntegrate ? 1 : 0);
		if (w->debugTrace) HIP_TRY(hipMemcpyAsync(w->dbgVel.p, w->b_vel.p, w->bodies.size() * 16, hipMemcpyDeviceToDevice, w->stream));
		TRACE("integrate");
		if (s.hasJoints && !s.exactLarge && !p.sortInIntegrate) LAUNCH(w, k_joints_sort, p.gJ, 64, d);
		LAUNCH(w, k_large_init, p.gC, 256, d, sp, p.bodyWarm ? 1 : 0);
		TRACE("init");
		return 0;
	}

	// The colours of one sweep that are launches (mode 0 warm start, 1 velocity iteration `it`, 2 position iteration `it`):
	// ONE launch of k_blocks_sweep over the blocks, else a launch per colour in [0, bigEnd).
	int sweepColours(int mode, int it)
	{
		if (s.useSweep) return launchBlocks(mode);
		const bool timeIt = mode == 1 && w->kernelTiming == 1;
		for (int col = 0; col < p.bigEnd; ++col)
		{
			if (!colorUsed(p, col)) continue;
			if (timeIt) { int rc = ktRecord(w); if (rc) return rc; w->ktKind = 1; }
			if (mode == 2) LAUNCH(w, k_large_position, gridOfColor(s, p, col), 256, d, col);
			else LAUNCH(w, k_large_velocity, gridOfColor(s, p, col), 256, d, col, mode);
			if (timeIt) { int rc = ktRecord(w); if (rc) return rc; }
			if (mode > 0 && w->debugTrace) TRACE(((mode == 1 ? "vel" : "pos") + std::to_string(it) + "_c" + std::to_string(col)).c_str());
		}
		return 0;
	}

	// What follows the colours in the sweep of (mode, it), as k_sweep_end's / k_rest_hub's `what` word.
	int whatFollows(int mode, int it) const
	{
		int what = s.hasHubs ? SE_HUB | (it > 0 ? SE_GUESS : 0) : 0;
		// (b2Island.cpp:256-268: the joints' InitVelocityConstraints follows the contacts' warm start; the first velocity
		// iteration then begins with the joints. The joint walk of an iteration is the last act of the sweep before it)
		if (mode == 0 && s.hasJoints) what |= SE_JOINTS_INIT | (sp.velIters > 0 ? SE_JOINTS_VEL : 0);
		if (mode == 1 && s.hasJoints && it + 1 < sp.velIters) what |= SE_JOINTS_VEL;
		if (mode == 2) what |= (s.hasJoints ? SE_JOINTS_POS : 0) | SE_POS_END | (it + 1 < sp.posIters ? SE_POS_BEGIN : 0);
		return what;
	}

	// The end of the sweep of (mode, it), behind its launched colours: the rest colours, the tail colours, the hub rows, the
	// joint walk, the verdict of a position iteration. The warm start (mode 0, it 0) never fuses, a position sweep only with
	// restHub > 1. `coloursDone`: every colour has had its sweep (after k_large_warm) - only what follows the colours is left.
	int endOfSweep(int mode, int it, bool coloursDone = false)
	{
		const int what = whatFollows(mode, it);
		if (p.fuseHub && (mode == 1 || (mode == 2 && w->restHub > 1))) return launchRestHub(mode, what);
		if (p.useRest && !coloursDone)
			if (int rc = launchRest(mode)) return rc;
		if (!p.useSweepEnd)
		{
			if (s.hasHubs)
				if (int rc = launchHub(mode, it > 0 ? 1 : 0, 0)) return rc;
			if (mode == 2 && s.hasJoints) LAUNCH(w, k_large_joints, p.gJ, 64, d, sp, 2);
			if (mode == 2) LAUNCH(w, k_large_pos_end, 1, 256, d);
			return 0;
		}
		const bool tail = !(s.useSweep || p.useRest || coloursDone);
		if (!what && !(tail && p.tailAny)) return 0;
		const int tf = tail ? p.tailFirst : 0, te = tail ? s.nColors : 0;
		if (!(p.leftoverApart && (what & SE_HUB))) return launchSweepEnd(mode, tf, te, what);
		// (leftover hub rows apart: up to the fixed point, k_large_hub behind it, then what follows the hub rows)
		if (int rc = launchSweepEnd(mode, tf, te, (what & (SE_HUB | SE_GUESS)) | SE_HUB_WIDE_ONLY)) return rc;
		if (int rc = launchHub(mode, (what & SE_GUESS) ? 1 : 0, 1)) return rc;
		const int behind = what & ~(SE_HUB | SE_GUESS);
		return behind ? launchSweepEnd(mode, 0, 0, behind) : 0;
	}

	int warmStart()
	{
		if (sp.warmStarting)
		{
			if (p.bodyWarm) LAUNCH(w, k_large_warm, p.gB, 256, d);
			else if (int rc = sweepColours(0, 0)) return rc;
			if (int rc = endOfSweep(0, 0, p.bodyWarm)) return rc;
		}
		TRACE("warmstart");
		if (s.hasJoints && !(p.useSweepEnd && sp.warmStarting)) LAUNCH(w, k_large_joints, p.gJ, 64, d, sp, 0);
		return 0;
	}

	int velocityIteration(int it)
	{
		// (with k_sweep_end the joint walk of iteration it is the last act of the sweep before it)
		if (s.hasJoints && !(p.useSweepEnd && (it > 0 || sp.warmStarting))) LAUNCH(w, k_large_joints, p.gJ, 64, d, sp, 1);
		if (int rc = sweepColours(1, it)) return rc;
		return endOfSweep(1, it);
	}

	// b2Island.cpp:280-297: impulses stored, positions integrated (and the first position iteration begun).
	int afterVelocity()
	{
		if (p.afterFused) LAUNCH(w, k_large_after_velocity, gridFor(std::max(s.nLContacts, s.nLBodies)), 256, d, sp);
		else
		{
			LAUNCH(w, k_large_store_impulses, p.gC, 256, d);
			TRACE("store_impulses");
			LAUNCH(w, k_large_integrate_positions, p.gB, 256, d, sp);
			TRACE("integrate_positions");
		}
		return 0;
	}

	int positionIteration(int it)
	{
		// (k_sweep_end begins the next iteration itself, k_large_after_velocity the first)
		if ((!p.useSweepEnd || it == 0) && !(p.afterFused && it == 0)) LAUNCH(w, k_large_pos_begin, gridFor(s.nLIslands), 256, d);
		if (int rc = sweepColours(2, it)) return rc;
		return endOfSweep(2, it);
	}

	// (for b2hip_debug_read 27: what this pass was planned as)
	void recordPlan() const
	{
		b2hip_world::PlanRecord& r = w->planRecord;
		r.passes += 1;
		r.solver = s.exactLarge ? 3 : (s.useBlocks ? 1 : (s.useSweep ? 2 : 0));
		r.safe = p.safe ? 1 : 0;
		r.restFirst = p.restFirst; r.tailFirst = p.tailFirst; r.bigEnd = p.bigEnd;
		r.useRest = p.useRest ? 1 : 0; r.fuseHub = p.fuseHub ? 1 : 0;
		r.blockSort = d.blockSort; r.hubWide = d.hubWide; r.serialOrphans = d.serialOrphans;
		r.nColors = s.nColors; r.hasHubs = s.hasHubs ? 1 : 0; r.hasJoints = s.hasJoints ? 1 : 0;
		r.hubBuildOne = p.hubBuildOne ? 1 : 0; r.useSweepEnd = p.useSweepEnd ? 1 : 0; r.leftoverApart = p.leftoverApart ? 1 : 0;
	}

	int run()
	{
		recordPlan();
		int rc = layoutRows();
		if (rc) return rc;
		stampPhase(w, 7);
		if (!p.safe && w->recoverOn && p.waitsBetweenWorkgroups) LAUNCH(w, k_solver_snapshot, gridFor(std::max(s.nLBodies, s.nLContacts)), 256, d, 0);
		if (s.useBlocks) rc = solveResident();
		else
		{
			// b2Island::Solve sweep by sweep: k_blocks_sweep or a launch per colour
			rc = launchDeferredSmallIslands(w, s);
			if (rc == 0) rc = setUp();
			if (rc == 0 && s.useSweep) w->sweepSteps += 1;
			if (rc == 0) rc = warmStart();
			for (int it = 0; rc == 0 && it < sp.velIters; ++it) rc = velocityIteration(it);
			if (rc == 0) rc = afterVelocity();
			for (int it = 0; rc == 0 && it < sp.posIters; ++it) rc = positionIteration(it);
		}
		if (rc) return rc;
		LAUNCH(w, k_large_finalize, p.gB, 256, d, sp);
		TRACE("finalize");
		LAUNCH(w, k_large_sleep, p.gB, 256, d, sp);
		return 0;
	}
};

// Did every wait between workgroups come to its end? (the overflow word, published by one lane behind the solver; polled)
// If not - or if k_solve_blocks ran on an incomplete colouring - the saved state goes back and the large islands are
// solved once more, on the safe path.
static int recoverLarge(b2hip_world* w, SolveStep& s)
{
	DW& d = w->dw;
	w->solverSeq = (w->solverSeq + 1) & 0x7fff;
	LAUNCH(w, k_solver_status, 1, 64, d, w->h_solverWord.dev, w->solverSeq);
	if (int rc = pollPublished(w, (volatile const int*)&w->h_solverWord[1], w->solverSeq, "solver status")) return rc;
	const int flags = w->h_solverWord[0];
	// (k_solve_blocks read the colours on the device: were they complete?)
	const bool colorsBad = s.colorsOnDevice && ((flags & 4) != 0 || w->h_solverWord[2] != 0);
	if (s.colorsOnDevice) w->colorSmallPending = false; // (looked at here)
	if (!(flags & 64) && !colorsBad) return 0;
	if (w->tracePartition || w->traceRecovery) fprintf(stderr, "[b2hip] a wait between workgroups of the large-island solver timed out (overflow 0x%x): saved state back, the solve once more launch by launch\n", flags);
	LAUNCH(w, k_solver_snapshot, gridFor(std::max(s.nLBodies, s.nLContacts)), 256, d, 1);
	LAUNCH(w, k_solver_recover_reset, gridFor(d.nBodies), 256, d, w->gridBar.p);
	w->restArrived = 0;
	if (int rc = readState(w)) return rc;
	if (colorsBad)
	{
		if (w->traceRecovery) fprintf(stderr, "[b2hip] the resident solver ran on an incomplete colouring (overflow 0x%x, %d without a colour): colouring finished, the solve once more\n", flags, w->h_solverWord[2]);
		// finish the colouring first: the grid-wide rounds over what k_color_small left open
		if (int rc = colorRoundsUntilDone(w, s, w->h_dstate->c.nUncolored, 8)) return rc;
		if (w->h_dstate->c.overflow & 4) s.colorSpill = s.hasHubs = true;
		s.censusVoid = true;
		w->colorRecoveries += 1;
	}
	s.nColors = std::min(w->h_dstate->c.nColors, (int)HUB_COLOR);
	s.c.nColors = s.nColors;
	memcpy(s.c.colorRows, w->h_dstate->c.colorRows, sizeof(s.c.colorRows));
	if (flags & 64) w->solverRecoveries += 1;
	// the solver choice of the second pass: rows by colour, a launch per colour
	s.useBlocks = s.useSweep = false;
	s.colorsOnDevice = false;
	d.blockSort = 0;
	return LargePass(w, s, true).run();
}

static int solveLargeIslands(b2hip_world* w, SolveStep& s)
{
	if (!s.exactLarge) s.nColors = s.c.nColors;
	s.hasJoints = w->dw.nJoints > 0;
	chooseLargeSolver(w, s);
	if (int rc = colorLargeIslands(w, s)) return rc;
	if (s.colorSpill) w->colorRecoveries += 1;
	// A constraint that found no colour free joined the hub group AFTER k_color_check had counted it among its home block's
	// rows (Counters / blkRowStart): laid out by block it would leave its block's segment one row short - a stale row there,
	// which k_blocks_sweep / k_solve_blocks would solve - and push the hub group's segment past the last row k_large_init
	// fills (found by tests/test_gpu_large_plan.py: Tumbler 60 with two colours per range; the 31 cut colours can run out without
	// any switch, on two bodies with 31 other cut constraints between them). Such a step lays its rows out by colour - k_color_scan takes the
	// groups from the counts as they stand now - and runs launch per colour, like the second pass of a recovered step.
	if (s.colorSpill && (s.useBlocks || s.useSweep))
	{
		if (w->traceRecovery) fprintf(stderr, "[b2hip] a constraint without a free colour is swept with the hub rows: rows by colour, a launch per colour this step\n");
		s.useBlocks = s.useSweep = false;
		s.colorsOnDevice = false;
		w->dw.blockSort = 0;
	}
	// (a constraint without a colour carries HUB_COLOR: the colours to launch end below it)
	if (!s.exactLarge && s.nColors > HUB_COLOR) s.nColors = HUB_COLOR;
	LargePass pass(w, s, false);
	if (int rc = pass.run()) return rc;
	if (w->kernelTiming == 5 && w->ktKind == 8)
	{
		w->familyLaunches = (int)(w->launchCount - w->familyLaunchesAtStart);
		if (int rc = ktRecord(w)) return rc;
	}
	if (w->recoverOn && pass.p.waitsBetweenWorkgroups)
		if (int rc = recoverLarge(w, s)) return rc;
	TRACE("sleep");
	if (s.sideStream) HIP_TRY(hipStreamWaitEvent(w->stream, w->evJoin, 0));
	return 0;
}

static void recordSolveCounters(b2hip_world* w, const SolveStep& s)
{
	const Counters& c = s.c;
	w->last.nSIslands = c.nSIslands;
	w->last.nFreeIslands = c.nFreeIslands;
	w->last.nSBodies = c.nSBodies;
	w->last.nSContacts = c.nSContacts;
	w->last.nChunks = c.nChunks;
	w->last.nLIslands = s.nLIslands;
	w->last.nLBodies = s.nLBodies;
	w->last.nLContacts = s.nLContacts;
	w->last.nIslands = c.nIslands;
	w->last.nColors = s.nColors;
	w->last.nTouching = c.nTouching;
	w->last.nDestroy = c.nDestroy;
	w->last.nBlocks = c.nBlocks;
	w->last.nCutRows = c.nCutRows;
	w->last.blkMaxRows = c.blkMaxRows;
	w->last.partitions = c.partitions;
}

static int phaseSolve(b2hip_world* w)
{
	w->trace.clear();
	w->blocksThisStep = false;
	w->dw.serialOrphans = w->serialOrphansNext;
	if (w->kernelTiming <= 1)
	{
		// (the event pairs of the solver kernels belong to this phase; those of k_collide / k_sync_fixtures / k_find_pairs_small -
		// timing modes 2 to 4 - are taken in other phases of the step and cleared by b2hip_step_begin)
		w->ktUsed = 0;
		w->ktKind = 0;
	}
	SolveStep s;
	s.poll = !w->noCensusPoll;
	s.largeHint = w->largeHintSteps > 0;
	s.exactLarge = w->forceLarge == 2;
	int rc = buildIslands(w, s);
	if (rc == 0) rc = awaitIslandCensus(w, s);
	if (rc == 0) rc = largeIslandPolicy(w, s);
	if (rc == 0) rc = repartition(w, s);
	if (rc) return rc;
	stampPhase(w, 4);
	s.hasHubs = !s.exactLarge && (s.c.maxDegree > HUB_DEGREE || s.c.nSerialOrphans > 0);
	rc = solveSmallIslands(w, s);
	if (rc == 0) rc = sizeLargeIslands(w, s);
	if (rc) return rc;
	if (s.nLIslands > 0)
	{
		if ((rc = solveLargeIslands(w, s))) return rc;
		stampPhase(w, 8);
	}
	else
	{
		stampPhase(w, 7);
		stampPhase(w, 8);
	}
	recordSolveCounters(w, s);
	return 0;
}

static int phaseSyncFixtures(b2hip_world* w)
{
	DW& d = w->dw;
	if (int rk = ktBracket(w, 3, 6)) return rk;
	LAUNCH(w, k_sync_fixtures, gridFor(d.nProxies >= 262144 ? ((size_t)d.nProxies + 3) / 4 : (size_t)d.nProxies), 256, d); // (SYNC_TILE proxies per workgroup and round in a large world)
	if (int rk = ktBracket(w, 3, 6)) return rk;
	return 0;
}

// Makes the hash grid reflect every proxy's fat AABB as of now, without touching the pair census (k_grid_clear): force 1
// unless Counters::gridFresh says it already does (the TOI phase), force 2 whatever it says (the batched queries, with a
// scan context of their own: `sf`).
static int gridRebuildNow(b2hip_world* w, int force, ScanFlags& sf)
{
	DW& d = w->dw;
	LAUNCH(w, k_grid_clear, gridFor(d.gridMask + 1), 256, d, force);
	LAUNCH(w, k_grid_count, gridFor(d.nProxies), 256, d, force);
	deviceExclusiveScan<int>(w->stream, d.gridCount, d.gridStart, d.scanTmp, sf, w->consts.p + 1, (int)(d.gridMask + 1));
	LAUNCH(w, k_grid_fill, gridFor(d.nProxies), 256, d, force);
	return 0;
}

// The read-back of a step (and of a between-step destroy): k_end_step writes the state rows and, behind them, the counters
// straight into the pinned host buffer, its last workgroup the sequence number - which the host polls. No copy, no stream
// synchronisation (the kernel is the last thing on the stream).
static int awaitState(b2hip_world* w, size_t nb)
{
	const DState* tail = (const DState*)(w->h_state + B2D_STATE_TAIL(nb));
	if (int rc = pollPublished(w, (volatile const int*)&tail->pubSeq, w->stateSeq, "state read-back")) return rc;
	memcpy(w->h_dstate, (const void*)tail, offsetof(DState, pubSeq));
	return 0;
}

static inline bool shadowValid(const b2hip_world* w)
{
	return w->shadowDev != nullptr && w->shadowDev == w->stateOut.p && w->shadowHost == w->h_state && w->shadowRows == (size_t)w->dw.nBodies;
}
static inline void shadowWritten(b2hip_world* w)
{
	w->shadowDev = w->stateOut.p;
	w->shadowHost = w->h_state;
	w->shadowRows = (size_t)w->dw.nBodies;
}

// Behind SynchronizeFixtures the rows of all bodies but those the TOI phase will still move are final: a large world sends
// them now, on a second stream, under the pair update and the TOI phase (40 bytes per body over PCIe: 0.75 ms for a million
// bodies, the longest single item of that step), and k_end_step sends the rows that changed since (its shadow comparison).
// (two halves: the point on the main stream from which the rows may be read is marked right behind SynchronizeFixtures; the
// launches on the second stream are issued once the host has queued the pair search - or the main stream would wait for
// the host to get through these calls)
static int forkEarlyRows(b2hip_world* w)
{
	DW& d = w->dw;
	const bool lazy = w->lazyReadback || (w->spatial && !w->spFullRows);
	if (w->earlyRowsMin <= 0 || d.nBodies < w->earlyRowsMin || w->noStatePoll || lazy || w->rowsEarlyPending || w->rowsForked || w->debugSync || w->debugTrace) return 0;
	// (a user contact filter is called by the pair update while the copy would be running: a ShouldCollide that reads a body
	// - pullBody reads h_state - could see a row half old, half new. No early rows then: ADVICE round 4.)
	if (hasFilter(w)) return 0;
	if (!w->rowStream)
	{
		HIP_TRY(hipStreamCreateWithFlags(&w->rowStream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&w->rowFork, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&w->rowJoin, hipEventDisableTiming));
	}
	HIP_TRY(hipEventRecord(w->rowFork, w->stream));
	w->rowsForked = true;
	return 0;
}

static int startEarlyRows(b2hip_world* w)
{
	DW& d = w->dw;
	if (!w->rowsForked) return 0;
	w->rowsForked = false;
	HIP_TRY(hipStreamWaitEvent(w->rowStream, w->rowFork, 0));
	// The rows are gathered into the device's copy (stateOut: ~30 us for a million bodies) and leave from there by a copy - the
	// DMA engine's, which does not stand in the way of the kernels running meanwhile. (Stores from a kernel straight into host
	// memory, as k_end_step's are, do: with enough of them in flight to fill the link, the pair update beside them ran 1.5 x
	// slower - measured, 1 M bodies: 3.77 ms per step without the early launch, 3.29 at best with such a kernel, 3.11 with the copy.)
	DW dEarly = d;
	dEarly.stampMask = 0u; // (the phase stamps belong to the main stream's next kernel)
	hipLaunchKernelGGL(k_end_step, dim3(gridFor(d.nBodies)), dim3(256), 0, w->rowStream, dEarly, 0, (const int*)nullptr, w->stateOut.p, 0, END_STEP_EARLY, (float*)nullptr, 0, 0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(w->h_state, w->stateOut.p, (size_t)d.nBodies * 10 * sizeof(float), hipMemcpyDeviceToHost, w->rowStream));
	HIP_TRY(hipEventRecord(w->rowJoin, w->rowStream));
	shadowWritten(w);
	w->rowsEarlyPending = true;
	w->rowsWentEarly = true;
	return 0;
}

static int downloadState(b2hip_world* w, int clearForces, bool skipRowsIfRedo)
{
	DW& d = w->dw;
	const size_t nb = w->bodies.size();
	w->rowsForked = false; // (marked, never launched: a step without a pair update)
	if (w->rowsEarlyPending)
	{
		HIP_TRY(hipStreamWaitEvent(w->stream, w->rowJoin, 0));
		w->rowsEarlyPending = false;
	}
	// (lazy: every read-back of a step end leaves the rows where they are; a read-back outside a step is a full one)
	// (... and so does a spatially sharded world with the lean exchange: the rows of the bodies THIS rank owns go to the host
	// packed - k_end_step, DW::spOwnOut - the table of all rows on demand)
	const bool lazy = (w->lazyReadback || (w->spatial && !w->spFullRows)) && w->stepActive && !w->noStatePoll;
	w->rowsPending.store(lazy, std::memory_order_release);
	w->stateSeq = (w->stateSeq + 1) & 0x3fffffff;
	if (w->stateSeq == 0) w->stateSeq = 1;
	((DState*)(w->h_state + B2D_STATE_TAIL(nb)))->pubSeq = 0; // (whatever was there: not this number)
	const int clear = clearForces < 0 ? w->def.auto_clear_forces : clearForces;
	if (w->noStatePoll)
	{
		// B2HIP_NO_STATE_POLL=1, for comparison: into the device staging array, one copy, stream synchronisation
		LAUNCH(w, k_end_step, gridFor(d.nBodies), 256, d, clear, (const int*)w->gridBar.p, w->stateOut.p, w->stateSeq, 0, (float*)nullptr, 0, 0);
		w->rowsWentEarly = false;
		if (clear) w->forceOnDevice = false;
		HIP_TRY(hipMemcpyAsync(w->h_state, w->stateOut.p, B2D_STATE_TAIL(nb) * sizeof(float) + sizeof(DState), hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
		memcpy(w->h_dstate, w->h_state + B2D_STATE_TAIL(nb), offsetof(DState, pubSeq));
		w->shadowDev = nullptr; // (the staging array is the shadow's memory)
		return 0;
	}
	const int rowMode = shadowValid(w) ? 2 : 1;
	// The first read-back behind this step's early launch looks only at the tiles somebody has written a row of since
	// (DW::b_rowDirty) - unless it has forces to clear in every tile, or sweeps to reset that earlier calls of a sub-stepped
	// step advanced. Any later read-back of the step (fall-backs, a finished pair update) compares every row again.
	const bool clearing = clear && w->forceOnDevice;
	if (w->traceLaunches) fprintf(stderr, "[b2hip] host: read-back: rows went early %d, row mode %d, lazy %d, clearing %d (clear %d), marks %d\n", (int)w->rowsWentEarly, rowMode, (int)lazy, (int)clearing, clear, w->rowMarks);
	const int marks = (w->rowsWentEarly && rowMode == 2 && !lazy && !w->spatial && !clearing && !d.toiContinue && d.toiEventCap == 0) ? w->rowMarks : 0;
	w->rowsWentEarly = false;
	LAUNCH(w, k_end_step, gridFor(d.nBodies), 256, d, clear, (const int*)w->gridBar.p, w->h_state.dev, w->stateSeq,
		lazy ? END_STEP_LAZY : skipRowsIfRedo ? END_STEP_SKIP_IF_REDO : END_STEP_FULL, w->stateOut.p, rowMode, marks);
	if (w->traceLaunches) { fprintf(stderr, "[b2hip] host: awaiting the read-back %d\n", w->stateSeq); fflush(stderr); }
	const int rc = awaitState(w, nb);
	if (w->traceLaunches) { fprintf(stderr, "[b2hip] host: read-back %d arrived (rc %d), marked tiles %d of %d\n", w->stateSeq, rc, w->h_dstate->c.endBlocksDone, (d.nBodies + 255) / 256); fflush(stderr); }
	// (rowsSkipped: 0 - the rows were stored; the shadow of a full write is valid from here on)
	if (rc == 0 && rowMode == 1 && w->h_dstate->c.rowsSkipped == 0) shadowWritten(w);
	// (the forces are cleared row by row inside the tile loop: not when the rows were skipped)
	if (rc == 0 && clear && w->h_dstate->c.rowsSkipped != 1) w->forceOnDevice = false;
	if (rc == 0 && (w->h_dstate->c.overflow & 0x1000)) return setError(B2HIP_ERR_INVALID, "B2HIP_ROW_MARKS_CHECK: a body's read-back row changed behind the early launch without a mark (DW::b_rowDirty)");
	return rc;
}

// The rows a lazy step end left on the device (b2hip_set_lazy_readback), fetched when the first caller asks for a body's
// state: the row half of k_end_step on its own. Several user threads may ask at once (b2Body getters from range tasks).
static int fetchRows(b2hip_world* w)
{
	DEVICE_GUARD(w);
	DW& d = w->dw;
	const size_t nb = (size_t)d.nBodies; // (bodies created since the step are not on the device yet: the step's count)
	w->stateSeq = (w->stateSeq + 1) & 0x3fffffff;
	if (w->stateSeq == 0) w->stateSeq = 1;
	((DState*)(w->h_state + B2D_STATE_TAIL(nb)))->pubSeq = 0;
	const int rowMode = shadowValid(w) ? 2 : 1;
	LAUNCH(w, k_end_step, gridFor(d.nBodies), 256, d, 0, (const int*)nullptr, w->h_state.dev, w->stateSeq, END_STEP_ROWS, w->stateOut.p, rowMode, 0);
	const int rc = pollPublished(w, (volatile const int*)&((const DState*)(w->h_state + B2D_STATE_TAIL(nb)))->pubSeq, w->stateSeq, "lazy state read-back");
	if (rc == 0 && rowMode == 1) shadowWritten(w);
	return rc;
}

static void ensureRows(b2hip_world* w)
{
	if (!w->rowsPending.load(std::memory_order_acquire)) return;
	std::lock_guard<std::mutex> lock(w->rowsMutex);
	if (!w->rowsPending.load(std::memory_order_relaxed)) return;
	if (fetchRows(w) != 0)
	{
		// (the rows cannot be had: the world is as good as lost - every later call says why)
		w->failed = true;
		w->failedWhy = g_lastError;
	}
	w->rowsPending.store(false, std::memory_order_release);
}

static void refreshMirror(b2hip_world* w)
{
	// h_state now holds the state of every body; HostBody rows are pulled from it on demand (pullBody)
	w->stateCount = w->bodies.size();
	++w->mirrorEpoch;
	++w->stepEpoch;
}

// A phase that fails leaves the device state half-stepped: the world unlocks (so that it can still be inspected and
// destroyed) and every later call reports the failure instead of stepping on.
static int stepFailed(b2hip_world* w, int rc)
{
	if (rc)
	{
		w->stepActive = false;
		w->failed = true;
		w->failedWhy = g_lastError;
	}
	return rc;
}

static int checkUsable(b2hip_world* w, const char* what, bool mutator)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	if (w->failed) return setError(B2HIP_ERR_INVALID, std::string(what) + ": the world is in a failed state (" + w->failedWhy + ")");
	if (mutator && w->stepActive && !w->callbackWindow) return setError(B2HIP_ERR_INVALID, std::string(what) + " inside a step");
	return 0;
}

