// b2hip_api_query.h - batched AABB, point, shape-overlap, ray (closest, all hits, any hit), closest-shape-cast and distance
// queries between steps
// (include/b2hip.h; kernels: b2d_kernels_query.h).
//
// What a query sees: the edits made since the last step are uploaded first (flushEdits - what the next step's first call
// does; it uploads the host mirror, so it does the same whether it runs now or then, and the queued contact-array ops stay
// queued for the step), then the hash grid is rebuilt from every proxy's fat AABB (gridRebuildNow, force 2) - the TOI
// phase and SetTransform move boxes after the pair update built it. The rebuild leaves the pair census alone, and the one
// counter it writes (Counters::nLargeProxies) is put back afterwards: the next step finds the device state as it was.

static int queryUsable(b2hip_world* w, const char* what)
{
	if (int rcu = checkUsable(w, what, false)) return rcu;
	if (w->stepActive || !w->stepComplete) return setError(B2HIP_ERR_INVALID, std::string(what) + " inside a step");
	if (w->spatial || w->dw.shardCount > 1)
		return setError(B2HIP_ERR_UNSUPPORTED, std::string(what) + ": not on a sharded world (another rank's transforms are not current here)");
	return 0;
}

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

// edits to the device, the batch's buffers, the batch itself from the pinned buffer (nShapes < 0: n float4; else n
// QueryPose followed by the nShapes query ShapeRecs), a fresh grid
static int queryBegin(b2hip_world* w, int n, bool offsets, int nShapes = -1)
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

// The query shapes and the records of a shape batch, checked before anything touches the device: every shape one that
// b2hip_create_fixture accepts (and a polygon of at least one vertex), every shape index in [0, nShapes).
static int queryShapesCheck(const char* what, int nShapes, const b2hip_shape* shapes, int n, const int32_t* shapeOf, size_t stride,
                            std::vector<ShapeRec>& recs)
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
		const int32_t k = *(const int32_t*)((const char*)shapeOf + (size_t)i * stride);
		if (k < 0 || k >= nShapes)
			return setError(B2HIP_ERR_INVALID, std::string(what) + ": query " + std::to_string(i) + " names shape index " + std::to_string(k) +
			                ", outside [0, n_shapes)");
	}
	return 0;
}

// n QueryPose records (the pose's rotation by the host's sinf / cosf, as b2Rot::Set) and the shape table into the pinned
// buffer, from whichever of queries / casts / ranges is given (a range's max_distance travels in tx)
static int queryShapesStage(b2hip_world* w, int n, const std::vector<ShapeRec>& recs, const b2hip_shape_query* queries,
                            const b2hip_shape_cast* casts, size_t atLeast, const b2hip_shape_range* ranges = nullptr)
{
	const size_t bytes = (size_t)n * sizeof(QueryPose) + recs.size() * sizeof(ShapeRec);
	if (int rc = queryPinned(w, std::max(bytes, atLeast))) return rc;
	QueryPose* stage = (QueryPose*)w->qPinned;
	for (int i = 0; i < n; ++i)
	{
		QueryPose& r = stage[i];
		if (ranges)
		{
			r.x = ranges[i].x;
			r.y = ranges[i].y;
			r.s = sinf(ranges[i].angle);
			r.c = cosf(ranges[i].angle);
			r.tx = ranges[i].max_distance;
			r.ty = 0.0f;
			r.shape = ranges[i].shape;
			r.pad = 0;
			continue;
		}
		const float angle = queries ? queries[i].angle : casts[i].angle;
		r.x = queries ? queries[i].x : casts[i].x;
		r.y = queries ? queries[i].y : casts[i].y;
		r.s = sinf(angle);
		r.c = cosf(angle);
		r.tx = queries ? 0.0f : casts[i].tx;
		r.ty = queries ? 0.0f : casts[i].ty;
		r.shape = queries ? queries[i].shape : casts[i].shape;
		r.pad = 0;
	}
	if (!recs.empty()) memcpy(stage + n, recs.data(), recs.size() * sizeof(ShapeRec));
	return 0;
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

// Box, point, shape and within-range queries: a count pass, a scan, a fill pass, the sort. `in` is 4n floats of boxes or 2n of
// points; a shape query passes recs (the checked query shapes) and queries instead, a within-range query recs, ranges and
// hits: its sorted ids become full records on the device (k_query_range_eval), the first min(total, cap) of them.
static int queryBoxes(b2hip_world* w, const char* what, int n, const float* in, int kind, const std::vector<ShapeRec>* recs,
                      const b2hip_shape_query* queries, const b2hip_query_filter* f, int cap, int32_t* offsets, b2hip_query_item* items,
                      const b2hip_shape_range* ranges = nullptr, b2hip_distance_hit* hits = nullptr)
{
	const bool shaped = kind == QUERY_SHAPE || kind == QUERY_RANGE;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	const uint32_t mask = f ? (uint32_t)f->mask : 0xffffu;
	const int sensors = f ? (f->include_sensors != 0) : 1;
	offsets[0] = 0;
	if (n == 0) return 0;
	const size_t offsetBytes = ((size_t)n + 1) * sizeof(int);
	int rc;
	if (shaped)
	{
		rc = queryShapesStage(w, n, *recs, queries, nullptr, offsetBytes, ranges);
		if (rc) return rc;
	}
	else
	{
		rc = queryPinned(w, std::max((size_t)n * sizeof(float4), offsetBytes));
		if (rc) return rc;
		float4* stage = (float4*)w->qPinned;
		for (int i = 0; i < n; ++i)
			stage[i] = kind == QUERY_POINT ? make_float4(in[2 * (size_t)i], in[2 * (size_t)i + 1], in[2 * (size_t)i], in[2 * (size_t)i + 1])
			                               : make_float4(in[4 * (size_t)i], in[4 * (size_t)i + 1], in[4 * (size_t)i + 2], in[4 * (size_t)i + 3]);
	}
	rc = queryBegin(w, n, true, shaped ? (int)recs->size() : -1);
	if (rc) return rc;
	hipStream_t s = w->stream;
	DW& d = w->dw;
	const float4* boxes = (const float4*)w->qIn.p;
	const QueryPose* poses = w->qPoses.p;
	const ShapeRec* qshapes = w->qShapes.p;
	const int waveBlocks = gridFor((size_t)n * 64, 256, 8192); // (one wave per query)
	if (d.nProxies == 0)
	{
		HIP_TRY(hipMemsetAsync(w->qOffsets.p, 0, ((size_t)n + 1) * sizeof(int), s));
	}
	else
	{
		if (kind == QUERY_RANGE) LAUNCH(w, k_query_ranges_count, waveBlocks, 256, d, poses, qshapes, n, mask, sensors, w->qCounts.p);
		else if (kind == QUERY_SHAPE) LAUNCH(w, k_query_shapes_count, waveBlocks, 256, d, poses, qshapes, n, mask, sensors, w->qCounts.p);
		else if (kind == QUERY_POINT) LAUNCH(w, k_query_points_count, waveBlocks, 256, d, boxes, n, mask, sensors, w->qCounts.p);
		else LAUNCH(w, k_query_aabbs_count, waveBlocks, 256, d, boxes, n, mask, sensors, w->qCounts.p);
		deviceExclusiveScan<int>(s, w->qCounts.p, w->qOffsets.p, w->qScanWork.p, w->qScan, w->qWords.p, n);
	}
	int* hOff = (int*)w->qPinned;
	HIP_TRY(hipMemcpyAsync(hOff, w->qOffsets.p, offsetBytes, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(offsets, hOff, offsetBytes);
	const int total = offsets[n];
	if (total < 0) return setError(B2HIP_ERR_CAPACITY, std::string(what) + ": more than 2^31 items");
	if (total > 0)
	{
		rc = w->qItems.ensure((size_t)total, s, false, false);
		if (rc) return rc;
		const int* offs = (const int*)w->qOffsets.p;
		if (kind == QUERY_RANGE) LAUNCH(w, k_query_ranges_fill, waveBlocks, 256, d, poses, qshapes, n, mask, sensors, offs, w->qItems.p);
		else if (kind == QUERY_SHAPE) LAUNCH(w, k_query_shapes_fill, waveBlocks, 256, d, poses, qshapes, n, mask, sensors, offs, w->qItems.p);
		else if (kind == QUERY_POINT) LAUNCH(w, k_query_points_fill, waveBlocks, 256, d, boxes, n, mask, sensors, offs, w->qItems.p);
		else LAUNCH(w, k_query_aabbs_fill, waveBlocks, 256, d, boxes, n, mask, sensors, offs, w->qItems.p);
		LAUNCH(w, k_query_sort, gridFor((size_t)n, 1, 16384), QUERY_SORT_THREADS, offs, n, w->qItems.p);
		for (int i = 0; i < n; ++i)
		{
			const int len = offsets[i + 1] - offsets[i];
			if (len <= QUERY_SORT_MAX) continue;
			rc = w->qFlags.ensure((size_t)d.nProxies, s, false, true); // (k_query_compact_big leaves it zero)
			if (rc) return rc;
			LAUNCH(w, k_query_mark, gridFor((size_t)len), 256, (const int*)(w->qItems.p + offsets[i]), len, w->qFlags.p);
			LAUNCH(w, k_query_compact_big, 1, 1024, w->qFlags.p, d.nProxies, w->qItems.p + offsets[i]);
		}
	}
	const int copy = std::min(total, cap);
	if (kind == QUERY_RANGE)
	{
		if (copy > 0)
		{
			rc = w->qDistances.ensure((size_t)copy, s, false, false);
			if (rc) return rc;
			LAUNCH(w, k_query_range_eval, gridFor((size_t)copy), 256, d, poses, qshapes, n, (const int*)w->qOffsets.p, (const int*)w->qItems.p, copy,
			       w->qDistances.p);
		}
		rc = queryEnd(w);
		if (rc) return rc;
		if ((rc = queryPinned(w, (size_t)copy * sizeof(b2hip_distance_hit)))) return rc; // (the offsets have left it)
		if (copy > 0) HIP_TRY(hipMemcpyAsync(w->qPinned, w->qDistances.p, (size_t)copy * sizeof(b2hip_distance_hit), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (copy > 0) memcpy(hits, w->qPinned, (size_t)copy * sizeof(b2hip_distance_hit));
		return total;
	}
	rc = queryEnd(w);
	if (rc) return rc;
	if ((rc = queryPinned(w, (size_t)copy * sizeof(int)))) return rc; // (the offsets have left it)
	int* hItems = (int*)w->qPinned;
	if (copy > 0) HIP_TRY(hipMemcpyAsync(hItems, w->qItems.p, (size_t)copy * sizeof(int), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	for (int k = 0; k < copy; ++k)
	{
		items[k].fixture = hItems[k];
		items[k].body = w->fixtures[(size_t)hItems[k]].body;
	}
	return total;
}

static int queryListArgs(const char* what, int n, const void* in, int cap, int32_t* offsets, const void* items)
{
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (cap < 0) return setError(B2HIP_ERR_INVALID, std::string(what) + ": negative cap");
	if (!offsets || (n > 0 && !in) || (cap > 0 && !items)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	return 0;
}

int b2hip_query_aabbs(b2hip_world* w, int n, const float* boxes4n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                      b2hip_query_item* items)
{
	const char* what = "b2hip_query_aabbs";
	if (int rc = queryListArgs(what, n, boxes4n, cap, offsets, items)) return rc;
	return queryBoxes(w, what, n, boxes4n, QUERY_BOX, nullptr, nullptr, f, cap, offsets, items);
}

int b2hip_query_points(b2hip_world* w, int n, const float* points2n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                       b2hip_query_item* items)
{
	const char* what = "b2hip_query_points";
	if (int rc = queryListArgs(what, n, points2n, cap, offsets, items)) return rc;
	return queryBoxes(w, what, n, points2n, QUERY_POINT, nullptr, nullptr, f, cap, offsets, items);
}

// the rays of a batch into the pinned buffer (at least `atLeast` bytes of it) and on to the device, a fresh grid
static int queryRaysBegin(b2hip_world* w, int n, const float* rays4n, size_t atLeast, bool offsets)
{
	if (int rc = queryPinned(w, std::max((size_t)n * sizeof(float4), atLeast))) return rc;
	memcpy(w->qPinned, rays4n, (size_t)n * sizeof(float4));
	return queryBegin(w, n, offsets);
}

int b2hip_ray_cast_closest(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, b2hip_ray_hit* out)
{
	const char* what = "b2hip_ray_cast_closest";
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (!out || (n > 0 && !rays4n)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (n == 0) return B2HIP_OK;
	const uint32_t mask = f ? (uint32_t)f->mask : 0xffffu;
	const int sensors = f ? (f->include_sensors != 0) : 1;
	int rc = queryRaysBegin(w, n, rays4n, (size_t)n * sizeof(b2hip_ray_hit), false);
	if (rc) return rc;
	hipStream_t s = w->stream;
	DW& d = w->dw;
	if (d.nProxies == 0)
	{
		for (int i = 0; i < n; ++i)
		{
			memset(&out[i], 0, sizeof(b2hip_ray_hit));
			out[i].fixture = out[i].body = -1;
			out[i].fraction = 1.0f;
		}
		return B2HIP_OK;
	}
	rc = w->qHits.ensure((size_t)n, s, false, false);
	if (rc) return rc;
	LAUNCH(w, k_query_rays, gridFor((size_t)n * 64, 256, 8192), 256, d, (const float4*)w->qIn.p, n, mask, sensors, w->qHits.p);
	rc = queryEnd(w);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(w->qPinned, w->qHits.p, (size_t)n * sizeof(b2hip_ray_hit), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(out, w->qPinned, (size_t)n * sizeof(b2hip_ray_hit));
	return B2HIP_OK;
}

// Every hit of every ray: a count pass, a scan, a fill pass of (fraction bits, fixture id) keys, the sort of each ray's keys
// (in LDS; a ray with more than QUERY_SORT_MAX hits by one launch of its own over global memory), and the records of the
// first min(total, cap) keys.
int b2hip_ray_cast_all(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, int cap, int32_t* offsets, b2hip_ray_hit* hits)
{
	const char* what = "b2hip_ray_cast_all";
	if (int rc = queryListArgs(what, n, rays4n, cap, offsets, hits)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	const uint32_t mask = f ? (uint32_t)f->mask : 0xffffu;
	const int sensors = f ? (f->include_sensors != 0) : 1;
	offsets[0] = 0;
	if (n == 0) return 0;
	const size_t offsetBytes = ((size_t)n + 1) * sizeof(int);
	int rc = queryRaysBegin(w, n, rays4n, offsetBytes, true);
	if (rc) return rc;
	hipStream_t s = w->stream;
	DW& d = w->dw;
	const float4* rays = (const float4*)w->qIn.p;
	const int waveBlocks = gridFor((size_t)n * 64, 256, 8192); // (one wave per ray)
	if (d.nProxies == 0) HIP_TRY(hipMemsetAsync(w->qOffsets.p, 0, offsetBytes, s));
	else
	{
		LAUNCH(w, k_query_rays_all_count, waveBlocks, 256, d, rays, n, mask, sensors, w->qCounts.p);
		deviceExclusiveScan<int>(s, w->qCounts.p, w->qOffsets.p, w->qScanWork.p, w->qScan, w->qWords.p, n);
	}
	int* hOff = (int*)w->qPinned;
	HIP_TRY(hipMemcpyAsync(hOff, w->qOffsets.p, offsetBytes, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(offsets, hOff, offsetBytes);
	const int total = offsets[n];
	if (total < 0) return setError(B2HIP_ERR_CAPACITY, std::string(what) + ": more than 2^31 hits");
	const int copy = std::min(total, cap);
	if (total > 0)
	{
		rc = w->qKeys.ensure((size_t)total, s, false, false);
		if (rc) return rc;
		const int* offs = (const int*)w->qOffsets.p;
		LAUNCH(w, k_query_rays_all_fill, waveBlocks, 256, d, rays, n, mask, sensors, offs, w->qKeys.p);
		LAUNCH(w, k_query_sort_keys, gridFor((size_t)n, 1, 16384), QUERY_SORT_THREADS, offs, n, w->qKeys.p);
		for (int i = 0; i < n; ++i)
		{
			const int len = offsets[i + 1] - offsets[i];
			if (len <= QUERY_SORT_MAX) continue;
			if (len > (1 << 30)) return setError(B2HIP_ERR_CAPACITY, std::string(what) + ": more than 2^30 hits of one ray");
			size_t size = 2 * (size_t)QUERY_SORT_MAX;
			while (size < (size_t)len) size *= 2;
			rc = w->qKeysWork.ensure(size, s, false, false);
			if (rc) return rc;
			LAUNCH(w, k_query_sort_keys_big, 1, 1024, w->qKeys.p + offsets[i], len, w->qKeysWork.p, (int)size);
		}
		if (copy > 0)
		{
			rc = w->qHits.ensure((size_t)copy, s, false, false);
			if (rc) return rc;
			LAUNCH(w, k_query_rays_all_eval, gridFor((size_t)copy), 256, d, rays, n, offs, (const unsigned long long*)w->qKeys.p, copy, w->qHits.p);
		}
	}
	rc = queryEnd(w);
	if (rc) return rc;
	if ((rc = queryPinned(w, (size_t)copy * sizeof(b2hip_ray_hit)))) return rc; // (the offsets have left it)
	if (copy > 0) HIP_TRY(hipMemcpyAsync(w->qPinned, w->qHits.p, (size_t)copy * sizeof(b2hip_ray_hit), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (copy > 0) memcpy(hits, w->qPinned, (size_t)copy * sizeof(b2hip_ray_hit));
	return total;
}

int b2hip_ray_cast_any(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, uint8_t* out)
{
	const char* what = "b2hip_ray_cast_any";
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (!out || (n > 0 && !rays4n)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (n == 0) return B2HIP_OK;
	const uint32_t mask = f ? (uint32_t)f->mask : 0xffffu;
	const int sensors = f ? (f->include_sensors != 0) : 1;
	int rc = queryRaysBegin(w, n, rays4n, 0, false);
	if (rc) return rc;
	hipStream_t s = w->stream;
	DW& d = w->dw;
	if (d.nProxies == 0)
	{
		memset(out, 0, (size_t)n);
		return B2HIP_OK;
	}
	rc = w->qAny.ensure((size_t)n, s, false, false);
	if (rc) return rc;
	LAUNCH(w, k_query_rays_any, gridFor((size_t)n * 64, 256, 8192), 256, d, (const float4*)w->qIn.p, n, mask, sensors, w->qAny.p);
	rc = queryEnd(w);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(w->qPinned, w->qAny.p, (size_t)n, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(out, w->qPinned, (size_t)n);
	return B2HIP_OK;
}

int b2hip_query_shapes(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_query* queries,
                       const b2hip_query_filter* f, int cap, int32_t* offsets, b2hip_query_item* items)
{
	const char* what = "b2hip_query_shapes";
	if (int rc = queryListArgs(what, n, queries, cap, offsets, items)) return rc;
	if (n_shapes < 0 || n_shapes > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n_shapes must lie in [0, 2^24]");
	if (n_shapes > 0 && !shapes) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	std::vector<ShapeRec> recs;
	if (int rc = queryShapesCheck(what, n_shapes, shapes, n, n > 0 ? &queries[0].shape : nullptr, sizeof(b2hip_shape_query), recs)) return rc;
	return queryBoxes(w, what, n, nullptr, QUERY_SHAPE, &recs, queries, f, cap, offsets, items);
}

int b2hip_shape_cast_closest(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_cast* casts,
                             const b2hip_query_filter* f, b2hip_ray_hit* out)
{
	const char* what = "b2hip_shape_cast_closest";
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (n_shapes < 0 || n_shapes > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n_shapes must lie in [0, 2^24]");
	if (!out || (n > 0 && !casts) || (n_shapes > 0 && !shapes)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	std::vector<ShapeRec> recs;
	if (int rc = queryShapesCheck(what, n_shapes, shapes, n, n > 0 ? &casts[0].shape : nullptr, sizeof(b2hip_shape_cast), recs)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (n == 0) return B2HIP_OK;
	const uint32_t mask = f ? (uint32_t)f->mask : 0xffffu;
	const int sensors = f ? (f->include_sensors != 0) : 1;
	int rc = queryShapesStage(w, n, recs, nullptr, casts, (size_t)n * sizeof(b2hip_ray_hit));
	if (rc) return rc;
	rc = queryBegin(w, n, false, n_shapes);
	if (rc) return rc;
	hipStream_t s = w->stream;
	DW& d = w->dw;
	if (d.nProxies == 0)
	{
		for (int i = 0; i < n; ++i)
		{
			memset(&out[i], 0, sizeof(b2hip_ray_hit));
			out[i].fixture = out[i].body = -1;
			out[i].fraction = 1.0f;
		}
		return B2HIP_OK;
	}
	rc = w->qHits.ensure((size_t)n, s, false, false);
	if (rc) return rc;
	LAUNCH(w, k_query_shape_casts, gridFor((size_t)n * 64, 256, 8192), 256, d, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p, n,
	       mask, sensors, w->qHits.p);
	rc = queryEnd(w);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(w->qPinned, w->qHits.p, (size_t)n * sizeof(b2hip_ray_hit), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(out, w->qPinned, (size_t)n * sizeof(b2hip_ray_hit));
	return B2HIP_OK;
}

// the misses of a closest-distance batch (an empty world answers every record with one)
static void queryDistanceMisses(int n, b2hip_distance_hit* out)
{
	for (int i = 0; i < n; ++i)
	{
		memset(&out[i], 0, sizeof(b2hip_distance_hit));
		out[i].fixture = out[i].body = -1;
		out[i].distance = INFINITY;
	}
}

int b2hip_shape_distance_closest(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_range* ranges,
                                 const b2hip_query_filter* f, b2hip_distance_hit* out)
{
	const char* what = "b2hip_shape_distance_closest";
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (n_shapes < 0 || n_shapes > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n_shapes must lie in [0, 2^24]");
	if (!out || (n > 0 && !ranges) || (n_shapes > 0 && !shapes)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	std::vector<ShapeRec> recs;
	if (int rc = queryShapesCheck(what, n_shapes, shapes, n, n > 0 ? &ranges[0].shape : nullptr, sizeof(b2hip_shape_range), recs)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (n == 0) return B2HIP_OK;
	const uint32_t mask = f ? (uint32_t)f->mask : 0xffffu;
	const int sensors = f ? (f->include_sensors != 0) : 1;
	int rc = queryShapesStage(w, n, recs, nullptr, nullptr, (size_t)n * sizeof(b2hip_distance_hit), ranges);
	if (rc) return rc;
	rc = queryBegin(w, n, false, n_shapes);
	if (rc) return rc;
	hipStream_t s = w->stream;
	DW& d = w->dw;
	if (d.nProxies == 0)
	{
		queryDistanceMisses(n, out);
		return B2HIP_OK;
	}
	rc = w->qDistances.ensure((size_t)n, s, false, false);
	if (rc) return rc;
	LAUNCH(w, k_query_shape_distances, gridFor((size_t)n * 64, 256, 8192), 256, d, (const QueryPose*)w->qPoses.p, (const ShapeRec*)w->qShapes.p,
	       n, mask, sensors, w->qDistances.p);
	rc = queryEnd(w);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(w->qPinned, w->qDistances.p, (size_t)n * sizeof(b2hip_distance_hit), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(out, w->qPinned, (size_t)n * sizeof(b2hip_distance_hit));
	return B2HIP_OK;
}

int b2hip_query_shapes_within(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_range* ranges,
                              const b2hip_query_filter* f, int cap, int32_t* offsets, b2hip_distance_hit* hits)
{
	const char* what = "b2hip_query_shapes_within";
	if (int rc = queryListArgs(what, n, ranges, cap, offsets, hits)) return rc;
	if (n_shapes < 0 || n_shapes > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n_shapes must lie in [0, 2^24]");
	if (n_shapes > 0 && !shapes) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	std::vector<ShapeRec> recs;
	if (int rc = queryShapesCheck(what, n_shapes, shapes, n, n > 0 ? &ranges[0].shape : nullptr, sizeof(b2hip_shape_range), recs)) return rc;
	return queryBoxes(w, what, n, nullptr, QUERY_RANGE, &recs, nullptr, f, cap, offsets, nullptr, ranges, hits);
}
