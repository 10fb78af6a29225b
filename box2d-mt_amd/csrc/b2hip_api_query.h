// b2hip_api_query.h - batched AABB, point, shape-overlap, ray (closest, all hits, any hit), closest-shape-cast and distance
// queries between steps
// (include/b2hip.h; kernels: b2d_kernels_query.h).
//
// What a query sees: the edits made since the last step are uploaded first (flushEdits - what the next step's first call
// does; it uploads the host mirror, so it does the same whether it runs now or then, and the queued contact-array ops stay
// queued for the step), then the hash grid is rebuilt from every proxy's fat AABB (gridRebuildNow, force 2) - the TOI
// phase and SetTransform move boxes after the pair update built it. The rebuild leaves the pair census alone, and the one
// counter it writes (Counters::nLargeProxies) is put back afterwards: the next step finds the device state as it was.
//
// The ten entry points have two shapes, each written once. A FIXED call answers one record per query (queryFixed: the closest
// ray, any ray, the closest shape cast, the closest distance): begin, one launch, the records back. A LIST call answers a
// list per query (queryList: boxes, points, shapes, shapes within a range, every hit of a ray): a count pass, a scan, the
// offsets back, a fill pass, the sort, the way out. An entry point is its argument checks, its staging and one call of its
// skeleton, to which it hands its staging and its launches as callables (LAUNCH and HIP_TRY return the error from inside them as they do
// from a function body). Order matters throughout: the pinned buffer carries the batch in, then the offsets, then the results.

extern "C++" // (this file is included with C linkage, for its entry points; the skeletons below are templates)
{
static int queryUsable(b2hip_world* w, const char* what)
{
	if (int rcu = checkUsable(w, what, false)) return rcu;
	if (w->stepActive || !w->stepComplete) return setError(B2HIP_ERR_INVALID, std::string(what) + " inside a step");
	if (w->spatial || w->dw.shardCount > 1)
		return setError(B2HIP_ERR_UNSUPPORTED, std::string(what) + ": not on a sharded world (another rank's transforms are not current here)");
	return 0;
}

struct QueryFilter
{
	uint32_t mask;
	int sensors;
};
// a null filter: every category, sensors included
static QueryFilter queryFilterOf(const b2hip_query_filter* f)
{
	return QueryFilter{ f ? (uint32_t)f->mask : 0xffffu, f ? (f->include_sensors != 0) : 1 };
}

// edits to the device, the batch's buffers, the batch itself from the pinned buffer (nShapes < 0: n float4; else n
// QueryPose followed by the nShapes query ShapeRecs), a fresh grid. Called through queryFloat4Begin / queryShapesBegin.
static int queryBegin(b2hip_world* w, int n, bool offsets, int nShapes)
{
	int rc = flushEdits(w);
	if (rc) return rc;
	hipStream_t s = w->stream;
	rc = nShapes < 0 ? w->qIn.ensure((size_t)n, s, false, false) : w->qPoses.ensure((size_t)n, s, false, false);
	if (!rc && nShapes >= 0) rc = w->qShapes.ensure((size_t)std::max(nShapes, 1), s, false, false);
	if (!rc && offsets) rc = w->qCounts.ensure((size_t)n + 1, s, false, false);
	if (!rc && offsets) rc = w->qOffsets.ensure((size_t)n + 1, s, false, false);
	if (!rc && offsets) rc = w->qScanWork.ensure(3 * ((size_t)n / SCAN_TILE + 8), s, false, false);
	if (!rc) rc = w->qScanWords.ensure(((size_t)std::max<size_t>((size_t)n + 1, w->dw.gridMask + 1)) / SCAN_TILE + 8, s, true, true);
	if (!rc) rc = w->qWords.ensure(4, s, true, true);
	if (rc) return rc;
	w->qScan.words = w->qScanWords.p;
	w->qScan.count = w->qScanWords.cap;
	w->qScan.abortWord = w->qWords.p + 2;
	if (nShapes < 0) HIP_TRY(hipMemcpyAsync(w->qIn.p, w->qPinned, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, s));
	else
	{
		HIP_TRY(hipMemcpyAsync(w->qPoses.p, w->qPinned, (size_t)n * sizeof(QueryPose), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(w->qShapes.p, (const char*)w->qPinned + (size_t)n * sizeof(QueryPose), (size_t)nShapes * sizeof(ShapeRec),
		                       hipMemcpyHostToDevice, s));
	}
	const int words[3] = { n, 0, 0 }; // scan length, (nLargeProxies), scan abort word
	HIP_TRY(hipMemcpyAsync(w->qWords.p, words, sizeof(words), hipMemcpyHostToDevice, s));
	HIP_TRY(hipStreamSynchronize(s)); // (`words` is on this stack frame)
	if (w->dw.nProxies == 0) return 0;
	HIP_TRY(hipMemcpyAsync(w->qWords.p + 1, &w->d_state.p->c.nLargeProxies, sizeof(int), hipMemcpyDeviceToDevice, s));
	return gridRebuildNow(w, 2, w->qScan);
}

// a look-back of one of this call's scans gave up (b2d_scan.h): its output is not to be trusted
static int queryScanAborted(b2hip_world* w, const char* what)
{
	int word = 0;
	HIP_TRY(hipMemcpy(&word, w->qWords.p + 2, sizeof(int), hipMemcpyDeviceToHost));
	if (word != 0) return setError(B2HIP_ERR_HIP, std::string(what) + ": a scan of the query did not complete");
	return 0;
}

static int queryEnd(b2hip_world* w)
{
	if (w->dw.nProxies == 0) return 0;
	HIP_TRY(hipMemcpyAsync(&w->d_state.p->c.nLargeProxies, w->qWords.p + 1, sizeof(int), hipMemcpyDeviceToDevice, w->stream));
	return 0;
}

// ---- arguments ------------------------------------------------------------------------------------------------------------
// Checked before anything touches the device, in this order (b2hip_last_error names the first failure): n, [cap,] the table
// of query shapes, null pointers; then the shapes and the records' shape indices (queryShapesCheck); then queryUsable.

static int queryShapeTableArgs(const char* what, int nShapes, const b2hip_shape* shapes)
{
	if (nShapes < 0 || nShapes > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n_shapes must lie in [0, 2^24]");
	if (nShapes > 0 && !shapes) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	return 0;
}

// a fixed call's; a ray call has no table of query shapes: (0, nullptr)
static int queryFixedArgs(const char* what, int n, const void* in, const void* out, int nShapes, const b2hip_shape* shapes)
{
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (int rc = queryShapeTableArgs(what, nShapes, shapes)) return rc;
	if (!out || (n > 0 && !in)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	return 0;
}

// a list call's; one over shapes checks its table next (queryShapeTableArgs)
static int queryListArgs(const char* what, int n, const void* in, int cap, int32_t* offsets, const void* items)
{
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (cap < 0) return setError(B2HIP_ERR_INVALID, std::string(what) + ": negative cap");
	if (!offsets || (n > 0 && !in) || (cap > 0 && !items)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	return 0;
}

// The query shapes and the records of a shape batch: every shape one that b2hip_create_fixture accepts (and a polygon of at
// least one vertex), every record's shape index in [0, nShapes).
template <typename Q>
static int queryShapesCheck(const char* what, int nShapes, const b2hip_shape* shapes, int n, const Q* records, std::vector<ShapeRec>& recs)
{
	recs.resize((size_t)nShapes);
	for (int k = 0; k < nShapes; ++k)
	{
		const char* why = shapeRecordOf(&shapes[k], &recs[(size_t)k]);
		if (!why && shapes[k].type == B2HIP_SHAPE_POLYGON && shapes[k].count < 1) why = "a polygon needs at least one vertex";
		if (why) return setError(B2HIP_ERR_INVALID, std::string(what) + ": query shape " + std::to_string(k) + ": " + why);
	}
	for (int i = 0; i < n; ++i)
	{
		const int32_t k = records[i].shape;
		if (k < 0 || k >= nShapes)
			return setError(B2HIP_ERR_INVALID, std::string(what) + ": query " + std::to_string(i) + " names shape index " + std::to_string(k) +
			                ", outside [0, n_shapes)");
	}
	return 0;
}

// ---- staging and begin: the batch into the pinned buffer, which is made at least `atLeast` bytes (what comes back through
// it), then queryBegin ---------------------------------------------------------------------------------------------------------

static int queryPinned(b2hip_world* w, size_t bytes)
{
	if (bytes <= w->qPinnedBytes) return 0;
	size_t cap = w->qPinnedBytes ? w->qPinnedBytes : 4096;
	while (cap < bytes) cap *= 2;
	if (w->qPinned) HIP_TRY(hipHostFree(w->qPinned));
	w->qPinned = nullptr;
	w->qPinnedBytes = 0;
	HIP_TRY(hipHostMalloc(&w->qPinned, cap, hipHostMallocDefault));
	w->qPinnedBytes = cap;
	return 0;
}

// n float4: rays and boxes as they are (width 4), points as the boxes (x, y, x, y) (width 2)
static int queryFloat4Begin(b2hip_world* w, int n, const float* in, int width, size_t atLeast, bool offsets)
{
	if (int rc = queryPinned(w, std::max((size_t)n * sizeof(float4), atLeast))) return rc;
	float4* stage = (float4*)w->qPinned;
	if (width == 4) memcpy(stage, in, (size_t)n * sizeof(float4));
	else
		for (int i = 0; i < n; ++i) stage[i] = make_float4(in[2 * (size_t)i], in[2 * (size_t)i + 1], in[2 * (size_t)i], in[2 * (size_t)i + 1]);
	return queryBegin(w, n, offsets, -1); // (no poses, no table of query shapes)
}

// the pose's rotation by the host's sinf / cosf, as b2Rot::Set
static QueryPose queryPoseOf(float x, float y, float angle, float tx, float ty, int32_t shape)
{
	QueryPose r;
	r.x = x;
	r.y = y;
	r.s = sinf(angle);
	r.c = cosf(angle);
	r.tx = tx;
	r.ty = ty;
	r.shape = shape;
	r.pad = 0;
	return r;
}
static QueryPose queryPoseOf(const b2hip_shape_query& q) { return queryPoseOf(q.x, q.y, q.angle, 0.0f, 0.0f, q.shape); }
static QueryPose queryPoseOf(const b2hip_shape_cast& c) { return queryPoseOf(c.x, c.y, c.angle, c.tx, c.ty, c.shape); }
// (a range's max_distance travels in tx)
static QueryPose queryPoseOf(const b2hip_shape_range& r) { return queryPoseOf(r.x, r.y, r.angle, r.max_distance, 0.0f, r.shape); }

// n QueryPose records followed by the table of query shapes
template <typename Q>
static int queryShapesBegin(b2hip_world* w, int n, const std::vector<ShapeRec>& recs, const Q* records, size_t atLeast, bool offsets)
{
	const size_t bytes = (size_t)n * sizeof(QueryPose) + recs.size() * sizeof(ShapeRec);
	if (int rc = queryPinned(w, std::max(bytes, atLeast))) return rc;
	QueryPose* stage = (QueryPose*)w->qPinned;
	for (int i = 0; i < n; ++i) stage[i] = queryPoseOf(records[i]);
	if (!recs.empty()) memcpy(stage + n, recs.data(), recs.size() * sizeof(ShapeRec));
	return queryBegin(w, n, offsets, (int)recs.size());
}

// ---- the two skeletons ----------------------------------------------------------------------------------------------------
// Both run after the entry point's argument checks and are the first to look at the world: queryUsable refuses a null one,
// so an entry point names the world's arrays as members (&b2hip_world::qHits) and touches `w` only inside its callables.
// begin(atLeast, offsets) stages the batch and runs queryBegin (queryFloat4Begin / queryShapesBegin).
// A launch is handed over as a callable that takes its grid. QUERY_LAUNCH writes one: a lambda that captures by reference,
// expects the world under the name `w`, and launches 256 threads a workgroup with w->dw as the kernel's first argument, read
// at the launch (the arrays in its arguments are sized by then). LAUNCH returns the error from inside it.
#define QUERY_LAUNCH(kernel, ...) [&](int blocks) { LAUNCH(w, kernel, blocks, 256, w->dw, __VA_ARGS__); return 0; }

// A fixed call: launch writes n records into the world's array `records`, which come back through the pinned buffer. An
// empty world runs no kernel: the host answers every query with miss().
template <typename T, typename Miss, typename Begin, typename Launch>
static int queryFixed(b2hip_world* w, const char* what, int n, DevArray<T> b2hip_world::*records, Miss miss, T* out, Begin begin,
                      Launch launch)
{
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (n == 0) return B2HIP_OK;
	int rc = begin((size_t)n * sizeof(T), false);
	if (rc) return rc;
	hipStream_t s = w->stream;
	if (w->dw.nProxies == 0)
	{
		for (int i = 0; i < n; ++i) out[i] = miss();
		return B2HIP_OK;
	}
	rc = (w->*records).ensure((size_t)n, s, false, false);
	if (!rc) rc = launch(gridFor((size_t)n * 64, 256, 8192));
	if (!rc) rc = queryEnd(w);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(w->qPinned, (w->*records).p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(out, w->qPinned, (size_t)n * sizeof(T));
	return B2HIP_OK;
}

// What a list call's fill pass writes: the world's array of them, what they are called when there are too many, and the sort
// of each query's part, its long-list path included (QUERY_IDS, QUERY_KEYS below).
template <typename E>
struct QueryListKind
{
	DevArray<E> b2hip_world::*list;
	const char* noun;
	int (*sort)(b2hip_world* w, const char* what, int n, const int32_t* offsets);
};

// A list call: count fills qCounts, a scan makes qOffsets of them, and the offsets go back to the caller; fill writes each
// query's elements into kind.list at its offset, kind.sort orders each query's part, and out(copy) delivers the first
// copy = min(total, cap) of them.
template <typename E, typename Begin, typename Count, typename Fill, typename Out>
static int queryList(b2hip_world* w, const char* what, int n, int cap, int32_t* offsets, const QueryListKind<E>& kind, Begin begin,
                     Count count, Fill fill, Out out)
{
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	offsets[0] = 0;
	if (n == 0) return 0;
	const size_t offsetBytes = ((size_t)n + 1) * sizeof(int);
	int rc = begin(offsetBytes, true);
	if (rc) return rc;
	hipStream_t s = w->stream;
	const int waveBlocks = gridFor((size_t)n * 64, 256, 8192);
	if (w->dw.nProxies == 0) HIP_TRY(hipMemsetAsync(w->qOffsets.p, 0, offsetBytes, s));
	else
	{
		if ((rc = count(waveBlocks))) return rc;
		deviceExclusiveScan<int>(s, w->qCounts.p, w->qOffsets.p, w->qScanWork.p, w->qScan, w->qWords.p, n);
	}
	int* hOff = (int*)w->qPinned;
	HIP_TRY(hipMemcpyAsync(hOff, w->qOffsets.p, offsetBytes, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(offsets, hOff, offsetBytes);
	const int total = offsets[n];
	if (total < 0) return setError(B2HIP_ERR_CAPACITY, std::string(what) + ": more than 2^31 " + kind.noun);
	if (total > 0)
	{
		rc = (w->*kind.list).ensure((size_t)total, s, false, false);
		if (!rc) rc = fill(waveBlocks);
		if (!rc) rc = kind.sort(w, what, n, offsets);
		if (rc) return rc;
	}
	rc = out(std::min(total, cap));
	return rc ? rc : total;
}

// Each query's fixture ids ascending: in LDS; a list of more than QUERY_SORT_MAX by marking its ids and compacting the marks.
// (QueryListKind::sort's signature; nothing here can fail under the call's name)
static int querySortIds(b2hip_world* w, const char*, int n, const int32_t* offsets)
{
	LAUNCH(w, k_query_sort, gridFor((size_t)n, 1, 16384), QUERY_SORT_THREADS, (const int*)w->qOffsets.p, n, w->qItems.p);
	for (int i = 0; i < n; ++i)
	{
		const int len = offsets[i + 1] - offsets[i];
		if (len <= QUERY_SORT_MAX) continue;
		int rc = w->qFlags.ensure((size_t)w->dw.nProxies, w->stream, false, true); // (k_query_compact_big leaves it zero)
		if (rc) return rc;
		LAUNCH(w, k_query_mark, gridFor((size_t)len), 256, (const int*)(w->qItems.p + offsets[i]), len, w->qFlags.p);
		LAUNCH(w, k_query_compact_big, 1, 1024, w->qFlags.p, w->dw.nProxies, w->qItems.p + offsets[i]);
	}
	return 0;
}

// Each ray's (fraction bits, fixture id) keys ascending: in LDS; a ray with more than QUERY_SORT_MAX hits by one launch of
// its own over global memory.
static int querySortKeys(b2hip_world* w, const char* what, int n, const int32_t* offsets)
{
	LAUNCH(w, k_query_sort_keys, gridFor((size_t)n, 1, 16384), QUERY_SORT_THREADS, (const int*)w->qOffsets.p, n, w->qKeys.p);
	for (int i = 0; i < n; ++i)
	{
		const int len = offsets[i + 1] - offsets[i];
		if (len <= QUERY_SORT_MAX) continue;
		if (len > (1 << 30)) return setError(B2HIP_ERR_CAPACITY, std::string(what) + ": more than 2^30 hits of one ray");
		size_t size = 2 * (size_t)QUERY_SORT_MAX;
		while (size < (size_t)len) size *= 2;
		int rc = w->qKeysWork.ensure(size, w->stream, false, false);
		if (rc) return rc;
		LAUNCH(w, k_query_sort_keys_big, 1, 1024, w->qKeys.p + offsets[i], len, w->qKeysWork.p, (int)size);
	}
	return 0;
}

static const QueryListKind<int> QUERY_IDS = { &b2hip_world::qItems, "items", querySortIds };
static const QueryListKind<unsigned long long> QUERY_KEYS = { &b2hip_world::qKeys, "hits", querySortKeys };

// The way out of a list call: the world's counter put back, the first `copy` elements of `from` into the pinned buffer ...
template <typename R>
static int queryListOut(b2hip_world* w, const R* from, int copy)
{
	int rc = queryEnd(w);
	if (rc) return rc;
	if ((rc = queryPinned(w, (size_t)copy * sizeof(R)))) return rc; // (the offsets have left it)
	if (copy > 0) HIP_TRY(hipMemcpyAsync(w->qPinned, from, (size_t)copy * sizeof(R), hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	return 0;
}

// ... sorted fixture ids, made (fixture, body) on the host
static int queryItemsOut(b2hip_world* w, int copy, b2hip_query_item* items)
{
	if (int rc = queryListOut(w, (const int*)w->qItems.p, copy)) return rc;
	const int* hItems = (const int*)w->qPinned;
	for (int k = 0; k < copy; ++k)
	{
		items[k].fixture = hItems[k];
		items[k].body = w->fixtures[(size_t)hItems[k]].body;
	}
	return 0;
}

// ... sorted ids or keys that eval turns into full records on the device first, a thread per record
template <typename R, typename Eval>
static int queryRecordsOut(b2hip_world* w, int copy, DevArray<R>& records, R* hits, Eval eval)
{
	int rc = copy > 0 ? records.ensure((size_t)copy, w->stream, false, false) : 0; // (called from a skeleton: w is not null)
	if (!rc && copy > 0) rc = eval(gridFor((size_t)copy));
	if (!rc) rc = queryListOut(w, (const R*)records.p, copy);
	if (!rc && copy > 0) memcpy(hits, w->qPinned, (size_t)copy * sizeof(R));
	return rc;
}

} // extern "C++"

// ---- the entry points: argument checks, the callables, one skeleton ---------------------------------------------------------

int b2hip_ray_cast_closest(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, b2hip_ray_hit* out)
{
	const char* what = "b2hip_ray_cast_closest";
	if (int rc = queryFixedArgs(what, n, rays4n, out, 0, nullptr)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offsets) { return queryFloat4Begin(w, n, rays4n, 4, atLeast, offsets); };
	const auto launch = QUERY_LAUNCH(k_query_rays, (const float4*)w->qIn.p, n, flt.mask, flt.sensors, w->qHits.p);
	return queryFixed(w, what, n, &b2hip_world::qHits, queryRayMiss, out, begin, launch);
}

int b2hip_ray_cast_any(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, uint8_t* out)
{
	const char* what = "b2hip_ray_cast_any";
	if (int rc = queryFixedArgs(what, n, rays4n, out, 0, nullptr)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offsets) { return queryFloat4Begin(w, n, rays4n, 4, atLeast, offsets); };
	const auto launch = QUERY_LAUNCH(k_query_rays_any, (const float4*)w->qIn.p, n, flt.mask, flt.sensors, w->qAny.p);
	return queryFixed(w, what, n, &b2hip_world::qAny, [] { return (uint8_t)0; }, out, begin, launch);
}

int b2hip_shape_cast_closest(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_cast* casts,
                             const b2hip_query_filter* f, b2hip_ray_hit* out)
{
	const char* what = "b2hip_shape_cast_closest";
	if (int rc = queryFixedArgs(what, n, casts, out, n_shapes, shapes)) return rc;
	std::vector<ShapeRec> recs;
	if (int rc = queryShapesCheck(what, n_shapes, shapes, n, casts, recs)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offsets) { return queryShapesBegin(w, n, recs, casts, atLeast, offsets); };
	const auto launch = QUERY_LAUNCH(k_query_shape_casts, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p, n, flt.mask,
	                                 flt.sensors, w->qHits.p);
	return queryFixed(w, what, n, &b2hip_world::qHits, queryRayMiss, out, begin, launch);
}

int b2hip_shape_distance_closest(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_range* ranges,
                                 const b2hip_query_filter* f, b2hip_distance_hit* out)
{
	const char* what = "b2hip_shape_distance_closest";
	if (int rc = queryFixedArgs(what, n, ranges, out, n_shapes, shapes)) return rc;
	std::vector<ShapeRec> recs;
	if (int rc = queryShapesCheck(what, n_shapes, shapes, n, ranges, recs)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offsets) { return queryShapesBegin(w, n, recs, ranges, atLeast, offsets); };
	const auto launch = QUERY_LAUNCH(k_query_shape_distances, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p, n, flt.mask,
	                                 flt.sensors, w->qDistances.p);
	return queryFixed(w, what, n, &b2hip_world::qDistances, queryDistanceMiss, out, begin, launch);
}

int b2hip_query_aabbs(b2hip_world* w, int n, const float* boxes4n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                      b2hip_query_item* items)
{
	const char* what = "b2hip_query_aabbs";
	if (int rc = queryListArgs(what, n, boxes4n, cap, offsets, items)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offs) { return queryFloat4Begin(w, n, boxes4n, 4, atLeast, offs); };
	const auto count = QUERY_LAUNCH(k_query_aabbs_count, (const float4*)w->qIn.p, n, flt.mask, flt.sensors, w->qCounts.p);
	const auto fill = QUERY_LAUNCH(k_query_aabbs_fill, (const float4*)w->qIn.p, n, flt.mask, flt.sensors, (const int*)w->qOffsets.p,
	                               w->qItems.p);
	return queryList(w, what, n, cap, offsets, QUERY_IDS, begin, count, fill, [&](int copy) { return queryItemsOut(w, copy, items); });
}

int b2hip_query_points(b2hip_world* w, int n, const float* points2n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                       b2hip_query_item* items)
{
	const char* what = "b2hip_query_points";
	if (int rc = queryListArgs(what, n, points2n, cap, offsets, items)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offs) { return queryFloat4Begin(w, n, points2n, 2, atLeast, offs); };
	const auto count = QUERY_LAUNCH(k_query_points_count, (const float4*)w->qIn.p, n, flt.mask, flt.sensors, w->qCounts.p);
	const auto fill = QUERY_LAUNCH(k_query_points_fill, (const float4*)w->qIn.p, n, flt.mask, flt.sensors, (const int*)w->qOffsets.p,
	                               w->qItems.p);
	return queryList(w, what, n, cap, offsets, QUERY_IDS, begin, count, fill, [&](int copy) { return queryItemsOut(w, copy, items); });
}

int b2hip_query_shapes(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_query* queries,
                       const b2hip_query_filter* f, int cap, int32_t* offsets, b2hip_query_item* items)
{
	const char* what = "b2hip_query_shapes";
	if (int rc = queryListArgs(what, n, queries, cap, offsets, items)) return rc;
	if (int rc = queryShapeTableArgs(what, n_shapes, shapes)) return rc;
	std::vector<ShapeRec> recs;
	if (int rc = queryShapesCheck(what, n_shapes, shapes, n, queries, recs)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offs) { return queryShapesBegin(w, n, recs, queries, atLeast, offs); };
	const auto count = QUERY_LAUNCH(k_query_shapes_count, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p, n, flt.mask,
	                                flt.sensors, w->qCounts.p);
	const auto fill = QUERY_LAUNCH(k_query_shapes_fill, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p, n, flt.mask,
	                               flt.sensors, (const int*)w->qOffsets.p, w->qItems.p);
	return queryList(w, what, n, cap, offsets, QUERY_IDS, begin, count, fill, [&](int copy) { return queryItemsOut(w, copy, items); });
}

int b2hip_query_shapes_within(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_range* ranges,
                              const b2hip_query_filter* f, int cap, int32_t* offsets, b2hip_distance_hit* hits)
{
	const char* what = "b2hip_query_shapes_within";
	if (int rc = queryListArgs(what, n, ranges, cap, offsets, hits)) return rc;
	if (int rc = queryShapeTableArgs(what, n_shapes, shapes)) return rc;
	std::vector<ShapeRec> recs;
	if (int rc = queryShapesCheck(what, n_shapes, shapes, n, ranges, recs)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offs) { return queryShapesBegin(w, n, recs, ranges, atLeast, offs); };
	const auto count = QUERY_LAUNCH(k_query_ranges_count, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p, n, flt.mask,
	                                flt.sensors, w->qCounts.p);
	const auto fill = QUERY_LAUNCH(k_query_ranges_fill, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p, n, flt.mask,
	                               flt.sensors, (const int*)w->qOffsets.p, w->qItems.p);
	const auto out = [&](int copy) { // (the sorted ids become full records on the device)
		return queryRecordsOut(w, copy, w->qDistances, hits,
		                       QUERY_LAUNCH(k_query_range_eval, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p, n,
		                                    (const int*)w->qOffsets.p, (const int*)w->qItems.p, copy, w->qDistances.p));
	};
	return queryList(w, what, n, cap, offsets, QUERY_IDS, begin, count, fill, out);
}

int b2hip_ray_cast_all(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                       b2hip_ray_hit* hits)
{
	const char* what = "b2hip_ray_cast_all";
	if (int rc = queryListArgs(what, n, rays4n, cap, offsets, hits)) return rc;
	const QueryFilter flt = queryFilterOf(f);
	const auto begin = [&](size_t atLeast, bool offs) { return queryFloat4Begin(w, n, rays4n, 4, atLeast, offs); };
	const auto count = QUERY_LAUNCH(k_query_rays_all_count, (const float4*)w->qIn.p, n, flt.mask, flt.sensors, w->qCounts.p);
	const auto fill = QUERY_LAUNCH(k_query_rays_all_fill, (const float4*)w->qIn.p, n, flt.mask, flt.sensors, (const int*)w->qOffsets.p,
	                               w->qKeys.p);
	const auto out = [&](int copy) { // (the sorted keys become full records on the device)
		return queryRecordsOut(w, copy, w->qHits, hits,
		                       QUERY_LAUNCH(k_query_rays_all_eval, (const float4*)w->qIn.p, n, (const int*)w->qOffsets.p,
		                                    (const unsigned long long*)w->qKeys.p, copy, w->qHits.p));
	};
	return queryList(w, what, n, cap, offsets, QUERY_KEYS, begin, count, fill, out);
}

#undef QUERY_LAUNCH
