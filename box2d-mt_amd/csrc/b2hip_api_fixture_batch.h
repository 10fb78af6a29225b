// b2hip_api_fixture_batch.h - batched fixture filter, sensor, thick-shape and material sets between steps (include/b2hip.h,
// block J: b2hip_fixture_set_filters, b2hip_fixture_set_sensors, b2hip_fixture_set_thicks, b2hip_fixture_set_materials;
// kernels: b2d_kernels_fixture_batch.h).
//
// Four more write calls of the family of b2hip_api_body_writes.h and b2hip_api_body_lifecycle.h. The single calls edit the
// host's HostFixture, push the fixture onto proxyEdits (five blocking copies per fixture at the next flushEdits) and queue one
// or two contact-array ops for k_apply_edits; these calls edit the same HostFixture fields at once - so that a later
// uploadProxyEdits or snapshot writes the words the device already has - and send the device the ids and one record per entry
// through the pinned buffer. No proxyEdits, pendingMoves, queueOp or markDirty.
//   pending edits  go first, queued contact ops included (lifecycleBegin): they lie underneath the call.
//   the move       a re-filtered fixture of an active body buffers (TouchProxy) gets its place from the host, in entry order
//                  behind the moves the device holds: the order the loop's pendingMoves are appended in. The pairs are sorted,
//                  so no step can tell; a snapshot taken before the step carries the buffer, and equals the loop's this way.
//   the wake       of b2hip_fixture_set_sensor goes through the host's mirror (setAwake -> markDirty -> eight rows uploaded).
//                  Here the host's row is brought up to date the same way (pullBody: a copy out of h_state, fetched first only
//                  if a batched write or a lazy world has left it pending) and gets the awake bit and the zero sleep time, so
//                  it is what the single call leaves once its upload is done; the device's row is edited by k_fixture_words.
//                  The body is NOT queued for upload, and h_state is not marked stale: a pulled row is the newer one until the
//                  next read-back, as behind the single call.
//   the TOI list   borrows the pair update's key buffer (free between steps), like block I's.

extern "C++"
{
// the ids, on the host: each in [0, fixture count), alive, each once; the first offender is named
static int fixtureBatchIds(b2hip_world* w, const char* what, int n, const int32_t* fixtures)
{
	const size_t nf = w->fixtures.size();
	if (w->fbSeen.size() < nf) w->fbSeen.resize(nf, 0u);
	if (++w->fbEpoch == 0u)
	{
		std::fill(w->fbSeen.begin(), w->fbSeen.end(), 0u);
		w->fbEpoch = 1u;
	}
	for (int i = 0; i < n; ++i)
	{
		const int32_t f = fixtures[i];
		const std::string who = std::string(what) + ": entry " + std::to_string(i) + " names fixture " + std::to_string(f);
		if (f < 0 || (size_t)f >= nf) return setError(B2HIP_ERR_INVALID, who + ", outside [0, b2hip_fixture_count)");
		if (w->fixtures[(size_t)f].dead) return setError(B2HIP_ERR_INVALID, who + ", which is destroyed");
		if (w->fbSeen[(size_t)f] == w->fbEpoch) return setError(B2HIP_ERR_INVALID, who + " a second time");
		w->fbSeen[(size_t)f] = w->fbEpoch;
	}
	return 0;
}

// What every call of the block checks, in the header's order; then pending edits to the device. *done: nothing is left to do
// (n == 0).
static int fixtureBatchBegin(b2hip_world* w, const char* what, int n, const int32_t* fixtures, const void* values, const char* badMask, bool* done)
{
	*done = false;
	if (int rc = bodyWritesArgs(what, n, fixtures, values, what)) return rc; // (a write call has no output: any non-null pointer)
	if (int rc = queryUsable(w, what)) return rc;
	if (badMask) return setError(B2HIP_ERR_INVALID, std::string(what) + badMask);
	if (int rc = fixtureBatchIds(w, what, n, fixtures)) return rc;
	*done = n == 0;
	return B2HIP_OK;
}

// the ids and the records to the device; `named` a word per fixture, every one 0 between calls (k_fixture_unname)
static int fixtureBatchStage(b2hip_world* w, int n, const int32_t* fixtures, const std::vector<uint4>& recs)
{
	int rc = w->fxNamed.ensure(std::max<size_t>(w->fixtures.size(), 1), w->stream, false, true);
	if (!rc) rc = w->lcWords.ensure(4, w->stream, false, true);
	if (!rc) rc = bodyWritesStage(w, n, fixtures, recs.data(), recs.size() * sizeof(uint4), 0);
	return rc;
}

// Sensors and thick shapes behind k_fixture_words (and bullets behind k_body_flag_sets, b2hip_api_body_props.h): the contact
// pass, the list of the contacts whose TOI candidacy changes, the replay. The list can be longer than the partition - contacts
// BECOME candidates - so the pass counts every change and stores what fits the room; a count above the room grows the pair
// buffers and lists again (the pass has changed nothing it reads). listPass(room): the launch of the pass, which names its
// contacts' entries from a table of its own; unname(): the launch that puts that table back to 0.
template <typename ListPass, typename Unname>
static int toiCandidacyBatch(b2hip_world* w, int n, ListPass listPass, Unname unname)
{
	hipStream_t s = w->stream;
	const int nContacts = std::max(w->h_dstate->c.nContacts, 0);
	int listed = 0;
	for (int round = 0;; ++round)
	{
		// (B2HIP_TEST_FIXTURE_LIST_ROOM: less room for the first listing, so that a small world lists twice)
		const int room = round == 0 && w->fixtureListRoom >= 0 ? std::min(w->fixtureListRoom, w->dw.capPairs) : w->dw.capPairs;
		HIP_TRY(hipMemsetAsync(w->lcWords.p, 0, sizeof(int), s));
		if (int rc = listPass(room)) return rc;
		HIP_TRY(hipMemcpyAsync(&listed, w->lcWords.p, sizeof(int), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (listed < 0 || listed > nContacts) return setError(B2HIP_ERR_HIP, "the batch listed more contacts than the world holds");
		if (listed <= room) break;
		if (round > 0) return setError(B2HIP_ERR_HIP, "the batch's list of contacts grew between two identical passes");
		w->statFixtureRelists += 1;
		if (listed > w->dw.capPairs)
		{
			w->pairCapHint = std::max(w->pairCapHint, (size_t)listed);
			if (int rc = ensureCapacity(w, (size_t)w->lastContacts)) return rc;
			if (listed > w->dw.capPairs) return setError(B2HIP_ERR_HIP, "the pair buffers did not grow to hold the batch's list");
		}
	}
	DW& d = w->dw;
	if (int rc = unname()) return rc;
	w->statFixtureLongSorts += listed > w->lifecycleSortMax ? 1 : 0;
	if (listed > 0 && listed <= w->lifecycleSortMax)
		LAUNCH(w, k_fixture_toi_sort_replay, 1, 1024, d, (const unsigned long long*)d.pairKey, (const int*)w->lcWords.p);
	else if (listed > 0)
	{
		// (r ascending, then nContacts - 1 - i ascending: the low word first, LSD)
		std::vector<std::pair<int, int>> passes;
		radixPasses(0, radixBits(std::max(nContacts, 1)), passes);
		radixPasses(32, radixBits(n), passes);
		uint64_t *kin = d.pairKey, *kout = d.pairKey2;
		int2 *vin = d.pairProxy, *vout = d.pairProxy2; // (payloads nobody reads)
		if (int rc = radixSort(w, kin, kout, vin, vout, w->lcWords.p, listed / RADIX_TILE + 1, passes)) return rc;
		LAUNCH(w, k_fixture_toi_replay, 1, 64, d, (const unsigned long long*)kin, (const int*)w->lcWords.p, listed);
	}
	if (int rc = readState(w)) return rc; // (the counters as they are on the device; the pinned buffer is the next call's)
	if (w->h_dstate->c.overflow & SCAN_ABORT_BIT) return setError(B2HIP_ERR_HIP, "a look-back of the sort gave up waiting for a predecessor tile");
	return B2HIP_OK;
}

template <int KIND>
static int fixtureBatchContacts(b2hip_world* w, int n)
{
	const int nContacts = std::max(w->h_dstate->c.nContacts, 0);
	auto listPass = [&](int room) -> int {
		LAUNCH(w, k_fixture_contacts<KIND>, gridFor((size_t)std::max(nContacts, 1)), 256, w->dw, (const int*)w->fxNamed.p, (unsigned long long*)w->dw.pairKey, room,
		       w->lcWords.p);
		return B2HIP_OK;
	};
	auto unname = [&]() -> int {
		LAUNCH(w, k_fixture_unname, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, w->dw.nProxies, w->fxNamed.p);
		return B2HIP_OK;
	};
	return toiCandidacyBatch(w, n, listPass, unname);
}

// b2hip_fixture_set_sensors / b2hip_fixture_set_thicks: an entry that has the requested value already takes no part.
template <int KIND>
static int fixtureSetFlags(b2hip_world* w, const char* what, int n, const int32_t* fixtures, const uint8_t* flag)
{
	bool done;
	if (int rc = fixtureBatchBegin(w, what, n, fixtures, flag, nullptr, &done)) return rc;
	if (done) return B2HIP_OK;
	DEVICE_GUARD(w);
	if (int rc = lifecycleBegin(w)) return rc;
	std::vector<uint4> recs((size_t)n);
	bool any = false;
	for (int i = 0; i < n; ++i)
	{
		const HostFixture& f = w->fixtures[(size_t)fixtures[i]];
		const bool want = flag[i] != 0, changes = (KIND == FIXTURE_SET_SENSORS ? f.isSensor : f.thick) != want;
		recs[(size_t)i] = make_uint4((want ? 1u : 0u) | (changes ? 2u : 0u), 0u, 0u, (uint32_t)f.body);
		any = any || changes;
	}
	if (!any) return B2HIP_OK;
	for (int i = 0; i < n; ++i)
	{
		if ((recs[(size_t)i].x & 2u) == 0u) continue;
		HostFixture& f = w->fixtures[(size_t)fixtures[i]];
		if (KIND == FIXTURE_SET_THICKS)
		{
			f.thick = flag[i] != 0;
			continue;
		}
		f.isSensor = flag[i] != 0;
		// setAwake (b2hip_host_world.h), without the upload: the head of this file
		HostBody& b = w->bodies[(size_t)f.body];
		if (b.type == B2HIP_STATIC_BODY && (b.flags & BF_AWAKE) != 0) continue;
		pullBody(w, f.body);
		b.flags |= BF_AWAKE;
		b.sleepTime = 0.0f;
	}
	if (w->failed) return setError(B2HIP_ERR_HIP, std::string(what) + ": " + w->failedWhy); // (pullBody could not read a force row)
	int rc = fixtureBatchStage(w, n, fixtures, recs);
	if (rc) return lifecycleDone(w, rc);
	auto device = [&]() -> int {
		LAUNCH(w, k_fixture_words<KIND>, gridFor((size_t)n), 256, w->dw, (const int*)w->bcIds.p, (const FixtureSetRec*)w->bwIn.p, n, 0, 0, w->fxNamed.p);
		return fixtureBatchContacts<KIND>(w, n);
	};
	return lifecycleDone(w, device());
}
} // extern "C++"

int b2hip_fixture_set_filters(b2hip_world* w, int n, const int32_t* fixtures, const b2hip_fixture_filter* filters)
{
	const char* what = "b2hip_fixture_set_filters";
	bool done;
	if (int rc = fixtureBatchBegin(w, what, n, fixtures, filters, nullptr, &done)) return rc;
	if (done) return B2HIP_OK;
	DEVICE_GUARD(w);
	if (int rc = lifecycleBegin(w)) return rc;
	// b2Fixture::Refilter touches the proxy of a fixture whose body is active (b2hip_fixture_refilter): one buffered move each
	std::vector<uint4> recs((size_t)n);
	int moves = 0;
	for (int i = 0; i < n; ++i)
	{
		const HostFixture& f = w->fixtures[(size_t)fixtures[i]];
		const bool touches = (w->bodies[(size_t)f.body].flags & BF_ACTIVE) != 0;
		recs[(size_t)i] = make_uint4((uint32_t)filters[i].category_bits | ((uint32_t)filters[i].mask_bits << 16), (uint32_t)(uint16_t)filters[i].group_index,
		                             touches ? (uint32_t)moves : 0xffffffffu, (uint32_t)f.body);
		moves += touches ? 1 : 0;
	}
	const int buffered = w->h_dstate->c.nMoves;
	if (buffered < 0 || (size_t)buffered + (size_t)moves > (size_t)w->dw.capMoves)
		return setError(B2HIP_ERR_UNSUPPORTED, std::string(what) + ": the move buffer holds " + std::to_string(buffered) + " of " + std::to_string(w->dw.capMoves) +
		                " entries and the batch can add " + std::to_string(moves) + ": step the world first");
	for (int i = 0; i < n; ++i)
	{
		HostFixture& f = w->fixtures[(size_t)fixtures[i]];
		f.categoryBits = filters[i].category_bits;
		f.maskBits = filters[i].mask_bits;
		f.groupIndex = filters[i].group_index;
	}
	w->refilterPending = true; // (a user contact filter sees the flagged contacts: collideImpl)
	int rc = fixtureBatchStage(w, n, fixtures, recs);
	if (rc) return lifecycleDone(w, rc);
	auto device = [&]() -> int {
		const int nContacts = std::max(w->h_dstate->c.nContacts, 0);
		LAUNCH(w, k_fixture_words<FIXTURE_SET_FILTERS>, gridFor((size_t)n), 256, w->dw, (const int*)w->bcIds.p, (const FixtureSetRec*)w->bwIn.p, n, buffered, moves,
		       w->fxNamed.p);
		LAUNCH(w, k_fixture_contacts<FIXTURE_SET_FILTERS>, gridFor((size_t)std::max(nContacts, 1)), 256, w->dw, (const int*)w->fxNamed.p, (unsigned long long*)nullptr, 0,
		       (int*)nullptr);
		LAUNCH(w, k_fixture_unname, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, w->dw.nProxies, w->fxNamed.p);
		return readState(w); // (the move counter as it is on the device; the pinned buffer is the next call's)
	};
	return lifecycleDone(w, device());
}

int b2hip_fixture_set_sensors(b2hip_world* w, int n, const int32_t* fixtures, const uint8_t* sensor)
{
	return fixtureSetFlags<FIXTURE_SET_SENSORS>(w, "b2hip_fixture_set_sensors", n, fixtures, sensor);
}

int b2hip_fixture_set_thicks(b2hip_world* w, int n, const int32_t* fixtures, const uint8_t* thick)
{
	return fixtureSetFlags<FIXTURE_SET_THICKS>(w, "b2hip_fixture_set_thicks", n, fixtures, thick);
}

int b2hip_fixture_set_materials(b2hip_world* w, int n, const int32_t* fixtures, const b2hip_fixture_material* materials, int mask)
{
	const char* what = "b2hip_fixture_set_materials";
	const int all = B2HIP_MATERIAL_DENSITY | B2HIP_MATERIAL_FRICTION | B2HIP_MATERIAL_RESTITUTION;
	bool done;
	if (int rc = fixtureBatchBegin(w, what, n, fixtures, materials, (mask & ~all) != 0 || mask == 0 ? ": mask must be a non-empty subset of the three B2HIP_MATERIAL_* bits" : nullptr,
	                               &done))
		return rc;
	if (done) return B2HIP_OK;
	DEVICE_GUARD(w);
	if (int rc = lifecycleBegin(w)) return rc;
	// (the density is the host's alone: the next ResetMassData reads it; existing contacts keep their mixture)
	std::vector<uint4> recs((size_t)n);
	for (int i = 0; i < n; ++i)
	{
		HostFixture& f = w->fixtures[(size_t)fixtures[i]];
		if (mask & B2HIP_MATERIAL_DENSITY) f.density = materials[i].density;
		if (mask & B2HIP_MATERIAL_FRICTION) f.friction = materials[i].friction;
		if (mask & B2HIP_MATERIAL_RESTITUTION) f.restitution = materials[i].restitution;
		uint32_t bits[2];
		memcpy(&bits[0], &f.friction, 4);
		memcpy(&bits[1], &f.restitution, 4);
		recs[(size_t)i] = make_uint4(bits[0], bits[1], 0u, 0u);
	}
	int rc = fixtureBatchStage(w, n, fixtures, recs);
	if (rc) return lifecycleDone(w, rc);
	auto device = [&]() -> int {
		LAUNCH(w, k_fixture_words<FIXTURE_SET_MATERIALS>, gridFor((size_t)n), 256, w->dw, (const int*)w->bcIds.p, (const FixtureSetRec*)w->bwIn.p, n, 0, 0, w->fxNamed.p);
		HIP_TRY(hipStreamSynchronize(w->stream)); // (the pinned buffer is the next call's)
		return B2HIP_OK;
	};
	return lifecycleDone(w, device());
}
