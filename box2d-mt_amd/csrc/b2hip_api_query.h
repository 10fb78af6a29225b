// b2hip_api_query.h - batched AABB, point and closest-ray queries between steps (include/b2hip.h; kernels:
// b2d_kernels_query.h).
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

// edits to the device, the batch's buffers, the batch itself (n float4 from the pinned buffer), a fresh grid
static int queryBegin(b2hip_world* w, int n, bool offsets)
{
	int rc = flushEdits(w);
	if (rc) return rc;
	hipStream_t s = w->stream;
	rc = w->qIn.ensure((size_t)n, s, false, false);
	if (!rc && offsets) rc = w->qCounts.ensure((size_t)n + 1, s, false, false);
	if (!rc && offsets) rc = w->qOffsets.ensure((size_t)n + 1, s, false, false);
	if (!rc && offsets) rc = w->qScanWork.ensure(3 * ((size_t)n / SCAN_TILE + 8), s, false, false);
	if (!rc) rc = w->qScanWords.ensure(((size_t)std::max<size_t>((size_t)n + 1, w->dw.gridMask + 1)) / SCAN_TILE + 8, s, true, true);
	if (!rc) rc = w->qWords.ensure(4, s, true, true);
	if (rc) return rc;
	w->qScan.words = w->qScanWords.p;
	w->qScan.count = w->qScanWords.cap;
	w->qScan.abortWord = w->qWords.p + 2;
	HIP_TRY(hipMemcpyAsync(w->qIn.p, w->qPinned, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, s));
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

static int queryBoxes(b2hip_world* w, const char* what, int n, const float* in, bool points, const b2hip_query_filter* f, int cap,
                      int32_t* offsets, b2hip_query_item* items)
{
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (cap < 0) return setError(B2HIP_ERR_INVALID, std::string(what) + ": negative cap");
	if (!offsets || (n > 0 && !in) || (cap > 0 && !items)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	const uint32_t mask = f ? (uint32_t)f->mask : 0xffffu;
	const int sensors = f ? (f->include_sensors != 0) : 1;
	offsets[0] = 0;
	if (n == 0) return 0;
	int rc = queryPinned(w, std::max((size_t)n * sizeof(float4), ((size_t)n + 1) * sizeof(int)));
	if (rc) return rc;
	float4* stage = (float4*)w->qPinned;
	for (int i = 0; i < n; ++i)
		stage[i] = points ? make_float4(in[2 * (size_t)i], in[2 * (size_t)i + 1], in[2 * (size_t)i], in[2 * (size_t)i + 1])
		                  : make_float4(in[4 * (size_t)i], in[4 * (size_t)i + 1], in[4 * (size_t)i + 2], in[4 * (size_t)i + 3]);
	rc = queryBegin(w, n, true);
	if (rc) return rc;
	hipStream_t s = w->stream;
	DW& d = w->dw;
	const int waveBlocks = gridFor((size_t)n * 64, 256, 8192); // (one wave per query)
	if (d.nProxies == 0)
	{
		HIP_TRY(hipMemsetAsync(w->qOffsets.p, 0, ((size_t)n + 1) * sizeof(int), s));
	}
	else
	{
		if (points) LAUNCH(w, k_query_points_count, waveBlocks, 256, d, (const float4*)w->qIn.p, n, mask, sensors, w->qCounts.p);
		else LAUNCH(w, k_query_aabbs_count, waveBlocks, 256, d, (const float4*)w->qIn.p, n, mask, sensors, w->qCounts.p);
		deviceExclusiveScan<int>(s, w->qCounts.p, w->qOffsets.p, w->qScanWork.p, w->qScan, w->qWords.p, n);
	}
	int* hOff = (int*)w->qPinned;
	HIP_TRY(hipMemcpyAsync(hOff, w->qOffsets.p, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((rc = queryScanAborted(w, what))) return rc;
	memcpy(offsets, hOff, ((size_t)n + 1) * sizeof(int));
	const int total = offsets[n];
	if (total < 0) return setError(B2HIP_ERR_CAPACITY, std::string(what) + ": more than 2^31 items");
	if (total > 0)
	{
		rc = w->qItems.ensure((size_t)total, s, false, false);
		if (rc) return rc;
		if (points) LAUNCH(w, k_query_points_fill, waveBlocks, 256, d, (const float4*)w->qIn.p, n, mask, sensors, (const int*)w->qOffsets.p, w->qItems.p);
		else LAUNCH(w, k_query_aabbs_fill, waveBlocks, 256, d, (const float4*)w->qIn.p, n, mask, sensors, (const int*)w->qOffsets.p, w->qItems.p);
		LAUNCH(w, k_query_sort, gridFor((size_t)n, 1, 16384), QUERY_SORT_THREADS, (const int*)w->qOffsets.p, n, w->qItems.p);
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
	rc = queryEnd(w);
	if (rc) return rc;
	const int copy = std::min(total, cap);
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

int b2hip_query_aabbs(b2hip_world* w, int n, const float* boxes4n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                      b2hip_query_item* items)
{
	return queryBoxes(w, "b2hip_query_aabbs", n, boxes4n, false, f, cap, offsets, items);
}

int b2hip_query_points(b2hip_world* w, int n, const float* points2n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                       b2hip_query_item* items)
{
	return queryBoxes(w, "b2hip_query_points", n, points2n, true, f, cap, offsets, items);
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
	int rc = queryPinned(w, (size_t)n * std::max(sizeof(float4), sizeof(b2hip_ray_hit)));
	if (rc) return rc;
	memcpy(w->qPinned, rays4n, (size_t)n * sizeof(float4));
	rc = queryBegin(w, n, false);
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
