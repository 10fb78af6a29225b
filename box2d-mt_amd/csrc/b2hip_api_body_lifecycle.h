// b2hip_api_body_lifecycle.h - batched body destruction and activation sets between steps (include/b2hip.h, block I:
// b2hip_destroy_bodies, b2hip_set_actives; kernels: b2d_kernels_body_lifecycle.h).
//
// Two more write calls of the family of b2hip_api_body_writes.h, whose head says which of the host's caches must not be
// believed over the device afterwards. The single calls edit the host's mirror, queue one contact-array op per body for
// k_apply_edits and leave the rest to the next flushEdits; these calls do in entry order what is host-only in them - proxy ids
// freed and handed out (freeProxyKey / allocProxyKey), the dead marks, the seed order, the host's copy of the active bit - and
// send the device three things through the pinned buffer: the ids, per entry what happens to it, per fixture of a named body
// its id, its new proxy id and what happens to it. The rows, the proxies and the contacts are then edited on the device
// (k_lifecycle_rows, k_lifecycle_proxies, k_destroy_contacts_of_set, the TOI partition), and the tail of applyEditOps follows
// as behind the single calls' ops: the compaction of the contact array and, because destroyed touching contacts wake bodies,
// a full read-back. No editBody / markDirty, no proxyEdits, fatEdits, pendingMoves or queueOp.
//   destroyed bodies  are pulled first (pullBody: a host-side copy of the row out of h_state), so that the dead body's host row
//                     is what b2hip_destroy_body leaves; nobody edits it again, so it is not marked as not pulled. Its force
//                     row is zeroed on the device AND on the host, and pullBody has dropped a forceDev mark: BODY_FORCES_*
//                     does not come into it.
//   (de)activated     are marked as not pulled (bodyWritesMirror, BODY_FORCES_NONE: neither call touches a force row).
//   end events        of destroyed contacts are appended on the device behind those of the last step; the step that follows
//                     starts its list afresh, so they are fetched here and delivered with that step's (carriedEvents), as the
//                     single calls' ops - applied inside that step - deliver theirs. So are those of single calls' ops that
//                     were still queued and that the call applied first (lifecycleBegin).

extern "C++"
{
// The events the device has appended since it held `eventsBefore` of them (h_dstate is current), kept for the next step's list.
static int lifecycleCarryEvents(b2hip_world* w, int eventsBefore)
{
	const int eventsNow = std::min(w->h_dstate->c.nEvents, w->dw.capContacts);
	if (w->eventsOn && eventsNow > eventsBefore && eventsBefore >= 0)
	{
		const size_t have = w->carriedEventKeys.size(), more = (size_t)(eventsNow - eventsBefore);
		w->carriedEventKeys.resize(have + more);
		w->carriedEventInfo.resize(have + more);
		HIP_TRY(hipMemcpy(w->carriedEventKeys.data() + have, w->evKey.p + eventsBefore, more * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(w->carriedEventInfo.data() + have, w->evInfo.p + eventsBefore, more * sizeof(int4), hipMemcpyDeviceToHost));
	}
	return B2HIP_OK;
}

// What the tail of applyEditOps leaves behind destroy ops, for a batch: the contact array compacted, the rows read back.
static int lifecycleTail(b2hip_world* w, int eventsBefore)
{
	int rc = editOpsTail(w, true, true);
	if (rc) return rc;
	if (w->h_dstate->c.overflow & SCAN_ABORT_BIT) return setError(B2HIP_ERR_HIP, "a look-back of the sort gave up waiting for a predecessor tile");
	return lifecycleCarryEvents(w, eventsBefore);
}

// The contact half of a batch, behind the kernel that has named its bodies in lcNamed (entry + 1): every contact of a named body
// is destroyed in one grid-wide pass, the names are taken back, the slots of the TOI partition are given back in the loop's
// order, and the tail of applyEditOps follows. nToi, nContacts, eventsBefore: the counters as lifecycleBegin read them.
// (b2hip_set_types, b2hip_api_body_props.h, ends here too.)
static int lifecycleContacts(b2hip_world* w, int n, int nToi, int nContacts, int eventsBefore)
{
	hipStream_t s = w->stream;
	DW& d = w->dw;
	int rc = 0;
	HIP_TRY(hipMemsetAsync(w->lcWords.p, 0, sizeof(int), s));
	// (the list's room is the pair update's key buffer, free between steps: lifecycleBegin has made it hold nToi keys)
	LAUNCH(w, k_destroy_contacts_of_set, gridFor((size_t)std::max(nContacts, 1)), 256, d, (const int*)w->lcNamed.p, (unsigned long long*)d.pairKey, nToi, w->lcWords.p);
	LAUNCH(w, k_lifecycle_unname, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, d.nBodies, w->lcNamed.p);
	if (nToi > 0) // (a world without TOI candidates pays nothing here)
	{
		int listed = 0;
		HIP_TRY(hipMemcpyAsync(&listed, w->lcWords.p, sizeof(int), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (listed < 0 || listed > nToi) return setError(B2HIP_ERR_HIP, "the batch listed more contacts with a TOI slot than the partition holds");
		w->statLifecycleLongSorts += listed > w->lifecycleSortMax ? 1 : 0;
		if (listed > 0 && listed <= w->lifecycleSortMax)
			LAUNCH(w, k_lifecycle_toi_sort_replay, 1, 1024, d, (unsigned long long*)d.pairKey, (const int*)w->lcWords.p);
		else if (listed > 0)
		{
			// (r ascending, then nContacts - 1 - i ascending: the low word first, LSD)
			std::vector<std::pair<int, int>> passes;
			radixPasses(0, radixBits(std::max(nContacts, 1)), passes);
			radixPasses(32, radixBits(n), passes);
			uint64_t *kin = d.pairKey, *kout = d.pairKey2;
			int2 *vin = d.pairProxy, *vout = d.pairProxy2; // (payloads nobody reads)
			if ((rc = radixSort(w, kin, kout, vin, vout, w->lcWords.p, listed / RADIX_TILE + 1, passes))) return rc;
			LAUNCH(w, k_lifecycle_toi_replay, 1, 64, d, (const unsigned long long*)kin, (const int*)w->lcWords.p, nToi);
		}
	}
	return lifecycleTail(w, eventsBefore);
}

// The device side of a batch whose host bookkeeping is done: `ops` one LIFECYCLE_* per entry, `recs` the fixture records.
// contacts: some entry destroys or deactivates (the contact pass and the tail run, as a queued EDIT_DESTROY_BODY makes
// applyEditOps run them whether or not a contact goes).
static int lifecycleDevice(b2hip_world* w, int n, const int32_t* bodies, const std::vector<int>& ops, const std::vector<int4>& recs, bool contacts)
{
	hipStream_t s = w->stream;
	DW& d = w->dw;
	const int nToi = contacts ? std::max(w->h_dstate->c.nToiOrder, 0) : 0, nContacts = std::max(w->h_dstate->c.nContacts, 0);
	const int eventsBefore = w->h_dstate->c.nEvents;
	const size_t opInts = ((size_t)n + 3) & ~(size_t)3; // (the fixture records start 16-byte aligned)
	std::vector<int> blob(opInts + 4 * recs.size(), 0);
	memcpy(blob.data(), ops.data(), (size_t)n * sizeof(int));
	if (!recs.empty()) memcpy(blob.data() + opInts, recs.data(), recs.size() * sizeof(int4));
	int rc = w->lcNamed.ensure(std::max<size_t>(w->bodies.size(), 1), s, false, true); // (every word 0 between calls: k_lifecycle_unname)
	if (!rc) rc = w->lcWords.ensure(4, s, false, true);
	if (!rc) rc = bodyWritesStage(w, n, bodies, blob.data(), blob.size() * sizeof(int), 0);
	if (rc) return rc;
	const int* dOps = (const int*)w->bwIn.p;
	const LifecycleProxy* dRecs = (const LifecycleProxy*)(dOps + opInts);
	LAUNCH(w, k_lifecycle_rows, gridFor((size_t)n), 256, (const int*)w->bcIds.p, dOps, n, d.nBodies, w->b_flags.p, w->b_vel.p, w->b_force.p, w->b_mass.p,
	       w->lcNamed.p);
	if (!recs.empty()) LAUNCH(w, k_lifecycle_proxies, gridFor(recs.size()), 256, d, dRecs, (int)recs.size());
	if (!contacts)
	{
		HIP_TRY(hipStreamSynchronize(s)); // (the pinned buffer is the next call's)
		return B2HIP_OK;
	}
	return lifecycleContacts(w, n, nToi, nContacts, eventsBefore);
}

// Pending edits to the device, then the counters as they are there: the contact count, the slots of the TOI partition, the
// buffered moves and the events so far in h_dstate. The pair update's buffers are made to hold a key per TOI slot.
// Queued contact operations of single calls are applied here, between steps, where the step that follows starts its event list
// afresh: the end events they append are carried like the batch's own (the single route applies them inside that step).
static int lifecycleBegin(b2hip_world* w)
{
	int eventsBefore = -1;
	if (w->eventsOn && !w->editOps.empty() && w->d_state.p)
	{
		HIP_TRY(hipMemcpyAsync(&eventsBefore, &w->d_state.p->c.nEvents, sizeof(int), hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
	}
	int rc = bodyWritesEdits(w);
	if (!rc) rc = readState(w);
	if (!rc) rc = lifecycleCarryEvents(w, eventsBefore);
	if (rc) return rc;
	const size_t nToi = (size_t)std::max(w->h_dstate->c.nToiOrder, 0);
	if (nToi > (size_t)w->dw.capPairs)
	{
		w->pairCapHint = std::max(w->pairCapHint, nToi);
		rc = ensureCapacity(w, (size_t)w->lastContacts);
	}
	return rc;
}

// A failure behind the host's bookkeeping - a copy, a launch, a sort that gave up - leaves the device partly edited: the world
// is marked failed, and every later call says so (a REFUSED call, by contrast, has applied nothing).
static int lifecycleDone(b2hip_world* w, int rc)
{
	if (rc)
	{
		w->failed = true;
		w->failedWhy = g_lastError;
	}
	return rc;
}

static bool lifecycleJointed(const b2hip_world* w)
{
	// (bodyContactsIds has just marked the named bodies: bcSeen == bcEpoch)
	auto named = [&](int b) { return b >= 0 && (size_t)b < w->bcSeen.size() && w->bcSeen[(size_t)b] == w->bcEpoch; };
	for (size_t j = 0; j < w->joints.size(); ++j)
	{
		const RevoluteJoint& jn = w->joints[j];
		if (jn.type == B2D_JOINT_DEAD) continue;
		if (named(jn.bodyA) || named(jn.bodyB)) return true;
		if (jn.type == B2D_JOINT_GEAR)
		{
			const GearRec& g = w->gears[(size_t)jn.enableLimit];
			if (named(g.bodyC) || named(g.bodyD)) return true;
		}
	}
	return false;
}
} // extern "C++"

int b2hip_destroy_bodies(b2hip_world* w, int n, const int32_t* bodies)
{
	const char* what = "b2hip_destroy_bodies";
	// (the call has neither records nor an output: the ids stand in for the one, any non-null pointer for the other)
	if (int rc = bodyWritesArgs(what, n, bodies, bodies, what)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = bodyContactsIds(w, what, n, bodies, true, true)) return rc;
	if (n == 0) return B2HIP_OK;
	if (lifecycleJointed(w))
	{
		// b2hip_destroy_joint wakes both bodies through the host's mirror, in an order against the other entries' edits that
		// can be observed: a batch that names a body with a live joint IS the loop of single calls - between the pending edits,
		// which lie underneath it as underneath any batch, and the application of what the loop queued, so that the contacts
		// are gone when the call returns whichever route it took
		if (int rc = lifecycleBegin(w)) return rc;
		for (int i = 0; i < n; ++i)
			if (int rc = b2hip_destroy_body(w, bodies[i])) return lifecycleDone(w, rc);
		return lifecycleDone(w, lifecycleBegin(w));
	}
	if (int rc = lifecycleBegin(w)) return rc;
	std::vector<int> ops((size_t)n, LIFECYCLE_DESTROY);
	std::vector<int4> recs;
	for (int i = 0; i < n; ++i)
	{
		const int id = bodies[i];
		pullBody(w, id);
		HostBody& b = w->bodies[(size_t)id];
		for (int k = (int)b.fixtures.size() - 1; k >= 0; --k) // newest first (dropFixture)
		{
			HostFixture& f = w->fixtures[(size_t)b.fixtures[(size_t)k]];
			freeProxyKey(w, f.proxyKey);
			f.dead = true;
			w->proxyListsStale = true;
			recs.push_back(make_int4(b.fixtures[(size_t)k], f.proxyKey, LIFECYCLE_DESTROY, id));
		}
		b.fixtures.clear();
		if (b.worldIndex >= 0)
		{
			// b2RemoveAndSwapBack on m_nonStaticBodies (b2World.cpp:662-667)
			const int slot = b.worldIndex, last = w->nonStatic.back();
			w->nonStatic[(size_t)slot] = last;
			w->bodies[(size_t)last].worldIndex = slot;
			w->nonStatic.pop_back();
			b.worldIndex = -1;
			w->orderDirty = true;
		}
		b.dead = 1;
		b.type = B2HIP_STATIC_BODY;
		b.flags &= ~(BF_ACTIVE | BF_AWAKE | BF_BULLET);
		b.vx = b.vy = b.w = 0.0f;
		b.fx = b.fy = b.torque = 0.0f;
		b.invMass = b.invI = 0.0f;
	}
	return lifecycleDone(w, lifecycleDevice(w, n, bodies, ops, recs, true));
}

int b2hip_set_actives(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* active)
{
	const char* what = "b2hip_set_actives";
	if (int rc = bodyWritesArgs(what, n, bodies, active, what)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = bodyContactsIds(w, what, n, bodies, true, true)) return rc;
	if (n == 0) return B2HIP_OK;
	if (int rc = lifecycleBegin(w)) return rc;
	// Both refusals before anything is written. The proxy ids are freed and handed out in entry order on the world's
	// allocator, of which a copy is kept: a refusal puts the copy back.
	std::vector<int> ops((size_t)n, LIFECYCLE_NONE), part;
	std::vector<int4> recs;
	const std::vector<FreeUnit> freeUnits0 = w->freeUnits;
	const int leafCount0 = w->leafCount, nextNode0 = w->nextNode;
	size_t creates = 0;
	for (int i = 0; i < n; ++i)
	{
		const int id = bodies[i];
		const HostBody& b = w->bodies[(size_t)id];
		if (((b.flags & BF_ACTIVE) != 0) == (active[i] != 0)) continue;
		ops[(size_t)i] = active[i] != 0 ? LIFECYCLE_ACTIVATE : LIFECYCLE_DEACTIVATE;
		part.push_back(id);
		for (int k = (int)b.fixtures.size() - 1; k >= 0; --k) // newest first
		{
			const int fid = b.fixtures[(size_t)k];
			const HostFixture& f = w->fixtures[(size_t)fid];
			if (active[i] == 0)
			{
				if (f.noProxy) continue;
				freeProxyKey(w, f.proxyKey);
				recs.push_back(make_int4(fid, -1, LIFECYCLE_DEACTIVATE, id));
				continue;
			}
			const int key = allocProxyKey(w);
			if (key < 0)
			{
				w->freeUnits = freeUnits0;
				w->leafCount = leafCount0;
				w->nextNode = nextNode0;
				return setError(B2HIP_ERR_UNSUPPORTED, std::string(what) + ": entry " + std::to_string(i) + " names body " + std::to_string(id) +
				                ": proxy id reuse after the broad-phase tree was emptied is not modelled");
			}
			recs.push_back(make_int4(fid, key, LIFECYCLE_ACTIVATE, id));
			creates += 1;
		}
	}
	const int buffered = w->h_dstate->c.nMoves;
	if (creates > 0 && (buffered < 0 || (size_t)buffered + creates > (size_t)w->dw.capMoves))
	{
		w->freeUnits = freeUnits0;
		w->leafCount = leafCount0;
		w->nextNode = nextNode0;
		return setError(B2HIP_ERR_UNSUPPORTED, std::string(what) + ": the move buffer holds " + std::to_string(buffered) + " of " + std::to_string(w->dw.capMoves) +
		                " entries and the batch can add " + std::to_string(creates) + ": step the world first");
	}
	if (part.empty()) return B2HIP_OK;
	bool deactivates = false;
	for (size_t k = 0; k < recs.size(); ++k)
	{
		HostFixture& f = w->fixtures[(size_t)recs[k].x];
		f.proxyKey = recs[k].y;
		f.noProxy = recs[k].z == LIFECYCLE_DEACTIVATE;
	}
	for (int i = 0; i < n; ++i)
	{
		if (ops[(size_t)i] == LIFECYCLE_NONE) continue;
		// b2hip_set_active tests the host's copy of the bit before it pulls anything: it follows the batch at once (as the
		// static body's awake bit at the end of b2hip_set_awakes)
		HostBody& b = w->bodies[(size_t)bodies[i]];
		if (ops[(size_t)i] == LIFECYCLE_ACTIVATE) b.flags |= BF_ACTIVE;
		else { b.flags &= ~(uint32_t)BF_ACTIVE; deactivates = true; }
	}
	w->proxyListsStale = true;
	// (the mirror before the tail: its read-back is the newer one)
	if (int rc = bodyWritesMirror(w, (int)part.size(), part.data(), BODY_FORCES_NONE)) return lifecycleDone(w, rc);
	return lifecycleDone(w, lifecycleDevice(w, n, bodies, ops, recs, deactivates));
}
