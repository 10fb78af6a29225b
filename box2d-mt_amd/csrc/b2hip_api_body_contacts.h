// b2hip_api_body_contacts.h - per-body contact lists and contact totals between steps
// (include/b2hip.h; kernels: b2d_kernels_body_contacts.h).
//
// What a call sees is what b2hip_get_contacts and b2hip_get_body_states see at the same moment: the edits made since the last
// step are uploaded (flushEdits - it uploads the host mirror, so it does the same whether it runs now or at the next step)
// and the queued contact-array operations are applied (applyEditOps, as flushForRead does for b2hip_get_contacts); then the
// device state is read for the contact count and the current contact array. From there on the call only reads what the step
// reads: its own arrays (b2hip_world::bc*) and the queries' list arrays and scan scratch (qOffsets, qItems, qFlags, ...) are
// all it writes. It builds no grid, so it does not go through queryBegin / queryEnd (queryEnd puts back a counter that only
// queryBegin saves): a third small skeleton beside queryFixed / queryList, the same list steps - count, scan, the offsets
// back, fill, sort, way out. The pinned buffer carries the ids in, then the offsets out, then the records out.

extern "C++"
{
// the arrays of the current contact buffer, as b2hip_get_contacts picks them
struct BodyContactArrays
{
	const int4* ids;
	const uint32_t* flags;
	const float4 *man0, *man1, *imp;
	const int4* man3;
	int nContacts;
};

// checked before the world is looked at: n, [cap,] null pointers (a totals call has no cap and no records: 0, nullptr)
static int bodyContactsArgs(const char* what, int n, const int32_t* bodies, int cap, const void* out, const void* records)
{
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (cap < 0) return setError(B2HIP_ERR_INVALID, std::string(what) + ": negative cap");
	if (!out || (n > 0 && !bodies) || (cap > 0 && !records)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	return 0;
}

// the ids, on the host: each in [0, body count), each once; the first offender is named. The batched body writes and the
// state gather (b2hip_api_body_writes.h) check theirs here too: `alive` refuses a destroyed body as well, `unique` false
// lets an id occur again (a read).
static int bodyContactsIds(b2hip_world* w, const char* what, int n, const int32_t* bodies, bool alive = false, bool unique = true)
{
	const size_t nb = w->bodies.size();
	if (w->bcSeen.size() < nb) w->bcSeen.resize(nb, 0u);
	if (++w->bcEpoch == 0u)
	{
		std::fill(w->bcSeen.begin(), w->bcSeen.end(), 0u);
		w->bcEpoch = 1u;
	}
	for (int i = 0; i < n; ++i)
	{
		const int32_t b = bodies[i];
		if (b < 0 || (size_t)b >= nb)
			return setError(B2HIP_ERR_INVALID, std::string(what) + ": entry " + std::to_string(i) + " names body " + std::to_string(b) +
			                ", outside [0, b2hip_body_count)");
		if (alive && w->bodies[(size_t)b].dead)
			return setError(B2HIP_ERR_INVALID, std::string(what) + ": entry " + std::to_string(i) + " names body " + std::to_string(b) + ", which is destroyed");
		if (!unique) continue;
		if (w->bcSeen[(size_t)b] == w->bcEpoch)
			return setError(B2HIP_ERR_INVALID, std::string(what) + ": entry " + std::to_string(i) + " names body " + std::to_string(b) + " a second time");
		w->bcSeen[(size_t)b] = w->bcEpoch;
	}
	return 0;
}

// Each body's contact indices ascending: in LDS; a list of more than QUERY_SORT_MAX by marking its contacts in a flag per
// CONTACT and compacting the marks (querySortIds' long-list path, whose flags are one per proxy).
static int bodyContactsSort(b2hip_world* w, int n, const int32_t* offsets, int nContacts)
{
	LAUNCH(w, k_query_sort, gridFor((size_t)n, 1, 16384), QUERY_SORT_THREADS, (const int*)w->qOffsets.p, n, w->qItems.p);
	for (int i = 0; i < n; ++i)
	{
		const int len = offsets[i + 1] - offsets[i];
		if (len <= QUERY_SORT_MAX) continue;
		int rc = w->qFlags.ensure((size_t)nContacts, w->stream, false, true); // (k_query_compact_big leaves it zero)
		if (rc) return rc;
		LAUNCH(w, k_query_mark, gridFor((size_t)len), 256, (const int*)(w->qItems.p + offsets[i]), len, w->qFlags.p);
		LAUNCH(w, k_query_compact_big, 1, 1024, w->qFlags.p, nContacts, w->qItems.p + offsets[i]);
	}
	return 0;
}

// The lists of the batch, all contacts or the touching ones: afterwards qOffsets / `offsets` (n + 1, complete) and qItems
// (each body's contact indices ascending) hold them, bcIds the batch, bcCounts[0 .. n) every body's count of ALL its
// contacts, `a` the current contact arrays. Called with n > 0 on a world that queryUsable has passed.
static int bodyContactsLists(b2hip_world* w, const char* what, int n, const int32_t* bodies, bool touchingOnly, int32_t* offsets,
                             BodyContactArrays& a)
{
	int rc = flushEdits(w);
	if (!rc) rc = applyEditOps(w, true);
	if (!rc) rc = readState(w);
	if (rc) return rc;
	const int cur = w->h_dstate->cur;
	a.nContacts = w->h_dstate->c.nContacts;
	a.ids = w->c_ids[cur].p; a.flags = w->c_flags[cur].p; a.man0 = w->c_man0[cur].p; a.man1 = w->c_man1[cur].p;
	a.imp = w->c_imp[cur].p; a.man3 = w->c_man3[cur].p;
	const int nb = (int)w->bodies.size();
	hipStream_t s = w->stream;
	const size_t offsetBytes = ((size_t)n + 1) * sizeof(int);
	rc = w->bcSlot.ensure((size_t)nb, s, false, false);
	if (!rc) rc = w->bcIds.ensure((size_t)n, s, false, false);
	if (!rc) rc = w->bcCounts.ensure(2 * ((size_t)n + 1), s, false, false);
	if (!rc) rc = w->qOffsets.ensure((size_t)n + 1, s, false, false);
	if (!rc) rc = w->qScanWork.ensure(3 * ((size_t)n / SCAN_TILE + 8), s, false, false);
	if (!rc) rc = w->qScanWords.ensure(((size_t)n + 1) / SCAN_TILE + 8, s, true, true);
	if (!rc) rc = w->qWords.ensure(4, s, true, true);
	if (!rc) rc = queryPinned(w, offsetBytes);
	if (rc) return rc;
	w->qScan.words = w->qScanWords.p;
	w->qScan.count = w->qScanWords.cap;
	w->qScan.abortWord = w->qWords.p + 2;
	memcpy(w->qPinned, bodies, (size_t)n * sizeof(int32_t));
	HIP_TRY(hipMemcpyAsync(w->bcIds.p, w->qPinned, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
	const int words[3] = { n, 0, 0 }; // scan length, (unused here), scan abort word
	HIP_TRY(hipMemcpyAsync(w->qWords.p, words, sizeof(words), hipMemcpyHostToDevice, s));
	HIP_TRY(hipStreamSynchronize(s)); // (`words` is on this stack frame)
	HIP_TRY(hipMemsetAsync(w->bcSlot.p, 0xff, (size_t)nb * sizeof(int), s)); // -1: not asked for
	HIP_TRY(hipMemsetAsync(w->bcCounts.p, 0, 2 * ((size_t)n + 1) * sizeof(int), s));
	int* countAll = w->bcCounts.p;
	int* countTouching = w->bcCounts.p + (size_t)n + 1;
	int* listed = touchingOnly ? countTouching : countAll; // the counter the lists are made of; the fill's cursor afterwards
	const int contactBlocks = gridFor((size_t)a.nContacts);
	LAUNCH(w, k_bc_slots, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, w->bcSlot.p, nb);
	if (a.nContacts > 0)
		LAUNCH(w, k_bc_count, contactBlocks, 256, a.ids, a.flags, a.nContacts, (const int*)w->bcSlot.p, nb, countAll, countTouching);
	deviceExclusiveScan<int>(s, listed, w->qOffsets.p, w->qScanWork.p, w->qScan, w->qWords.p, n);
	int* hOff = (int*)w->qPinned;
	HIP_TRY(hipMemcpyAsync(hOff, w->qOffsets.p, offsetBytes, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(offsets, hOff, offsetBytes);
	const int total = offsets[n];
	if (total < 0) return setError(B2HIP_ERR_CAPACITY, std::string(what) + ": more than 2^31 records");
	if (total == 0) return 0;
	rc = w->qItems.ensure((size_t)total, s, false, false);
	if (rc) return rc;
	HIP_TRY(hipMemsetAsync(listed, 0, (size_t)n * sizeof(int), s));
	LAUNCH(w, k_bc_fill, contactBlocks, 256, a.ids, a.flags, a.nContacts, (const int*)w->bcSlot.p, nb, touchingOnly ? 1 : 0,
	       (const int*)w->qOffsets.p, listed, w->qItems.p);
	return bodyContactsSort(w, n, offsets, a.nContacts);
}

// n records of the device array `from` through the pinned buffer (the offsets have left it) to the caller
template <typename R>
static int bodyContactsOut(b2hip_world* w, const R* from, int n, R* out)
{
	if (n == 0) return 0;
	if (int rc = queryPinned(w, (size_t)n * sizeof(R))) return rc;
	HIP_TRY(hipMemcpyAsync(w->qPinned, from, (size_t)n * sizeof(R), hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	memcpy(out, w->qPinned, (size_t)n * sizeof(R));
	return 0;
}

} // extern "C++"

int b2hip_body_contacts(b2hip_world* w, int n, const int32_t* bodies, int touching_only, int cap, int32_t* offsets,
                        b2hip_body_contact* records)
{
	const char* what = "b2hip_body_contacts";
	if (int rc = bodyContactsArgs(what, n, bodies, cap, offsets, records)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = bodyContactsIds(w, what, n, bodies)) return rc;
	offsets[0] = 0;
	if (n == 0) return 0;
	BodyContactArrays a;
	int rc = bodyContactsLists(w, what, n, bodies, touching_only != 0, offsets, a);
	if (rc) return rc;
	const int total = offsets[n], copy = std::min(total, cap);
	if (copy > 0)
	{
		if ((rc = w->bcRecords.ensure((size_t)copy, w->stream, false, false))) return rc;
		LAUNCH(w, k_bc_records, gridFor((size_t)copy), 256, a.ids, a.man0, a.man1, a.man3, a.imp, (const float4*)w->b_xf.p,
		       (const int*)w->bcIds.p, n, (const int*)w->qOffsets.p, (const int*)w->qItems.p, copy, w->bcRecords.p);
		if ((rc = bodyContactsOut(w, (const b2hip_body_contact*)w->bcRecords.p, copy, records))) return rc;
	}
	return total;
}

int b2hip_body_contact_totals(b2hip_world* w, int n, const int32_t* bodies, b2hip_body_contact_total* out)
{
	const char* what = "b2hip_body_contact_totals";
	if (int rc = bodyContactsArgs(what, n, bodies, 0, out, nullptr)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = bodyContactsIds(w, what, n, bodies)) return rc;
	if (n == 0) return B2HIP_OK;
	BodyContactArrays a;
	std::vector<int32_t> offsets((size_t)n + 1);
	int rc = bodyContactsLists(w, what, n, bodies, true, offsets.data(), a);
	if (!rc) rc = w->bcTotals.ensure((size_t)n, w->stream, false, false);
	if (rc) return rc;
	LAUNCH(w, k_bc_totals, gridFor((size_t)n * 64, 256, 8192), 256, a.ids, a.man0, a.man1, a.man3, a.imp, (const float4*)w->b_xf.p,
	       (const int*)w->bcIds.p, n, (const int*)w->qOffsets.p, (const int*)w->qItems.p, (const int*)w->bcCounts.p, w->bcTotals.p);
	if ((rc = bodyContactsOut(w, (const b2hip_body_contact_total*)w->bcTotals.p, n, out))) return rc;
	return B2HIP_OK;
}
