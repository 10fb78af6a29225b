// b2d_kernels_query.h - batched world queries between steps (b2hip_query_aabbs / b2hip_query_points / b2hip_ray_cast_closest /
// b2hip_query_shapes / b2hip_shape_cast_closest / b2hip_shape_distance_closest / b2hip_query_shapes_within /
// b2hip_ray_cast_all / b2hip_ray_cast_any).
//
// Everything is read from the world's device state: the fat AABBs, the proxies' filters and shapes, the bodies' transforms,
// and the hashed grid of b2d_kernels_broadphase.h, rebuilt from every proxy's box just before (gridRebuildNow). One WAVE per
// query. A proxy is binned in the cell of its centre and is at most gridLimit wide, so every proxy whose box overlaps the
// query box has its centre in the query box grown by half the limit: the cells of gridWindow. Cells of a window that hash to
// the same bucket would show a proxy twice; a candidate counts only in the cell its own centre lies in (the bucket dedup).
// Proxies wider than the limit (DW::largeProxies) are tested by every query.
//
// Determinism: the grid's order inside a bucket depends on arrival, so nothing here depends on it. Box, point and shape
// queries sort each query's items by fixture id (k_query_sort, k_query_compact_big); rays and shape casts keep the smallest
// (fraction bits, fixture) key, a total order; the closest distance keeps the smallest (distance bits, fixture) key; the
// all-hit rays sort each ray's (fraction bits, fixture) keys (k_query_sort_keys, k_query_sort_keys_big).
//
// What has one definition here, because its copies would have to agree to the bit: the ray walk's arithmetic (QueryRay: set-up,
// candidate cull, pieces - shared by the closest, all-hit and any-hit kernels; queryPieceCount / queryPieceSpan also by the
// shape cast), the keys (queryKey / queryKeyValue / queryKeyFixture), the owner of a flat item (queryOwner), the GJK call of
// every overlap and distance (queryDistance), and the miss records (queryRayMiss / queryDistanceMiss, host and device).
#ifndef B2D_KERNELS_QUERY_H
#define B2D_KERNELS_QUERY_H

#include "b2d_kernels_broadphase.h"
#include "b2d_kernels_collide.h"
#include "b2d_shapecast.h"
#include "b2d_shape_geom.h"

#define QUERY_WINDOW_MAX 4096     // cells a window may have; a wider one scans every proxy
#define QUERY_COORD_MAX 1.0e8f    // coordinates beyond this (in magnitude) scan every proxy too (no cell index overflows)
#define QUERY_SORT_MAX 4096       // items of one query sorted in LDS by k_query_sort; more: k_query_mark + k_query_compact_big
#define QUERY_SORT_THREADS 256

// b2hip_query_filter on the proxy's filter words (DW::p_filter0 low half = categoryBits, p_filter1 PF_SENSOR)
__device__ __forceinline__ bool queryFilterPasses(const DW& W, int q, uint32_t mask, int sensors)
{
	return (W.p_filter0[q] & mask & 0xffffu) != 0u && (sensors || (W.p_filter1[q] & PF_SENSOR) == 0);
}

__device__ __forceinline__ bool queryBoxSane(float4 b)
{
	return fabsf(b.x) <= QUERY_COORD_MAX && fabsf(b.y) <= QUERY_COORD_MAX && fabsf(b.z) <= QUERY_COORD_MAX && fabsf(b.w) <= QUERY_COORD_MAX;
}

// The (value bits, fixture id) key the closest and the all-hit walks order by: the bits of a float >= +0 order like the
// values, and ties go to the lower id. One definition: what is packed here is what every reader takes apart.
__device__ __forceinline__ unsigned long long queryKey(uint32_t valueBits, int q)
{
	return ((unsigned long long)valueBits << 32) | (uint32_t)q;
}
__device__ __forceinline__ float queryKeyValue(unsigned long long key) { return __uint_as_float((uint32_t)(key >> 32)); }
__device__ __forceinline__ int queryKeyFixture(unsigned long long key) { return (int)(uint32_t)key; }

// item k of a list call's flat output belongs to the last query i with offsets[i] <= k (a search over offsets[0 .. n]; empty
// queries share an offset with the next one)
__device__ __forceinline__ int queryOwner(const int* offsets, int n, int k)
{
	int lo = 0, hi = n; // (offsets[lo] <= k < offsets[hi])
	while (hi - lo > 1)
	{
		const int mid = (lo + hi) >> 1;
		if (offsets[mid] <= k) lo = mid; else hi = mid;
	}
	return lo;
}

// The records of a query that found nothing, every field set (pad included): what the kernels write for a miss and what
// the host writes for every query of an empty world, where no kernel runs - the same bytes.
__host__ __device__ inline b2hip_ray_hit queryRayMiss()
{
	b2hip_ray_hit o;
	o.fixture = o.body = -1;
	o.point_x = o.point_y = o.normal_x = o.normal_y = 0.0f;
	o.fraction = 1.0f;
	o.pad = 0;
	return o;
}
__host__ __device__ inline b2hip_distance_hit queryDistanceMiss()
{
	b2hip_distance_hit o;
	o.fixture = o.body = -1;
	o.point_ax = o.point_ay = o.point_bx = o.point_by = 0.0f;
	o.distance = INFINITY;
	o.iterations = 0;
	return o;
}

// Calls visit(valid, proxy, fatAabb) for every grid-sized proxy binned in a cell of box's window, 64 candidates per call,
// whole wave (the lanes' candidates: valid = false on lanes without one). The cells are taken 64 at a time, lane c owning
// cell c; their counts are flattened into one index space by a prefix sum over the lanes, and candidate idx finds its cell
// by a binary search over those sums (as k_find_pairs_window does). false: the window is too wide / degenerate - the caller
// scans every proxy instead (queryVisitAll).
template <typename F>
__device__ __forceinline__ bool queryVisitGrid(const DW& W, int lane, float4 box, F& visit)
{
	int ix0, iy0, nx, ny;
	if (!queryBoxSane(box) || !gridWindow(W, box, &ix0, &iy0, &nx, &ny)) return false;
	const int nCells = nx * ny;
	if (nCells > QUERY_WINDOW_MAX) return false;
	for (int c0 = 0; c0 < nCells; c0 += 64)
	{
		const int c = c0 + lane;
		int cx = 0, cy = 0, cnt = 0, start = 0;
		if (c < nCells)
		{
			cx = ix0 + c % nx;
			cy = iy0 + c / nx;
			const uint32_t h = cellHash(cx, cy, W.gridMask);
			cnt = W.gridCount[h];
			start = W.gridStart[h];
		}
		int incl = cnt;
		for (int off = 1; off < 64; off <<= 1)
		{
			const int v = __shfl_up(incl, off);
			if (lane >= off) incl += v;
		}
		const int excl = incl - cnt;
		const int total = __shfl(incl, 63);
		for (int base = 0; base < total; base += 64)
		{
			const int idx = base + lane;
			int lo = 0, hi = 63;
#pragma unroll
			for (int step = 0; step < 6; ++step)
			{
				const int mid = (lo + hi) >> 1;
				if (__shfl(incl, mid) > idx) hi = mid; else lo = mid + 1;
			}
			const int cl = lo < 63 ? lo : 63;
			const int t = __shfl(start, cl) + (idx - __shfl(excl, cl));
			const int cellX = __shfl(cx, cl), cellY = __shfl(cy, cl);
			bool valid = idx < total;
			int q = -1;
			float4 fat = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			if (valid)
			{
				q = W.gridItems[t];
				fat = W.gridFat[t];
				int px, py;
				proxyCell(W, fat, &px, &py);
				valid = px == cellX && py == cellY; // (the bucket dedup)
			}
			visit(valid, q, fat);
		}
	}
	return true;
}

template <typename F>
__device__ __forceinline__ void queryVisitLarge(const DW& W, int lane, F& visit)
{
	const int nLarge = W.st->c.nLargeProxies;
	for (int base = 0; base < nLarge; base += 64)
	{
		const int k = base + lane;
		const int q = k < nLarge ? W.largeProxies[k] : -1;
		visit(q >= 0, q, q >= 0 ? W.p_fat[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
	}
}

// every live proxy (grid-sized and large)
template <typename F>
__device__ __forceinline__ void queryVisitAll(const DW& W, int lane, F& visit)
{
	for (int base = 0; base < W.nProxies; base += 64)
	{
		const int q = base + lane;
		const bool live = q < W.nProxies && W.p_body[q] >= 0;
		visit(live, q, live ? W.p_fat[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
	}
}

// The record of one shape query or shape cast (b2hip_query_shapes / b2hip_shape_cast_closest): the pose as a transform the
// host built (sinf / cosf there, as b2Rot::Set), the index of the query shape in the call's table, the cast's translation.
// A distance query (b2hip_shape_distance_closest / b2hip_query_shapes_within) carries its max_distance in tx.
struct QueryPose
{
	float x, y, c, s;
	float tx, ty;
	int32_t shape, pad;
};

#define QUERY_BOX 0
#define QUERY_POINT 1
#define QUERY_SHAPE 2
#define QUERY_RANGE 3

__device__ __forceinline__ Xf queryPoseXf(const QueryPose& qp)
{
	Xf xf;
	xf.p = v2(qp.x, qp.y);
	xf.q.s = qp.s;
	xf.q.c = qp.c;
	return xf;
}

// a distance record is answered: a finite pose and a finite max_distance (QueryPose::tx) >= 0
__device__ __forceinline__ bool queryRangeValid(const QueryPose& qp)
{
	return isfinite(qp.x) && isfinite(qp.y) && isfinite(qp.c) && isfinite(qp.s) && isfinite(qp.tx) && qp.tx >= 0.0f;
}

// b2Distance between the query shape at its pose (proxy A) and proxy q's shape at its body's transform (proxy B), with the
// radii and from a zeroed cache: the value of the distance queries
__device__ __forceinline__ GjkOutput queryDistance(const DW& W, int q, const GjkProxy& pQ, Xf xfQ)
{
	GjkCache cache;
	cache.count = 0;
	cache.metric = 0.0f;
	for (int k = 0; k < 3; ++k) cache.indexA[k] = cache.indexB[k] = 0;
	GjkOutput dist;
	b2dDistance(dist, cache, pQ, xfQ, b2dProxy(W.shapes + W.p_shape[q]), loadXf(W.b_xf, W.p_body[q]), true);
	return dist;
}

__device__ __forceinline__ b2hip_distance_hit queryDistanceRecord(const DW& W, int q, const GjkProxy& pQ, Xf xfQ)
{
	const GjkOutput dist = queryDistance(W, q, pQ, xfQ);
	b2hip_distance_hit o;
	o.fixture = q;
	o.body = W.p_body[q];
	o.point_ax = dist.pointA.x;
	o.point_ay = dist.pointA.y;
	o.point_bx = dist.pointB.x;
	o.point_by = dist.pointB.y;
	o.distance = dist.distance;
	o.iterations = dist.iterations;
	return o;
}

// Box, point and shape queries. pass 0: counts[i] = items of query i; pass 1: query i's items (fixture ids, unsorted) at
// items[offsets[i] ...]. QUERY_POINT: boxes[i] = (x, y, x, y) and the shape must contain the point (b2dShapeTestPoint).
// QUERY_SHAPE: the box is the query shape's AABB at its pose (b2Shape::ComputeAABB), computed by every lane from the
// table, and a candidate must overlap the shape (b2TestOverlap: queryDistance below 10 epsilon; the query shape is proxy A,
// as in b2TestOverlap(query, 0, fixture, child, xfQ, xfBody)). Both proxies point into global memory (W.shapes, the query
// table), so b2dSupport's run-time indexing stays out of scratch.
// QUERY_RANGE (b2hip_query_shapes_within): the same box grown by the record's max_distance (QueryPose::tx) on every side, one
// float operation per coordinate, and a candidate counts when that GJK distance is <= max_distance (queryDistance, the
// value k_query_range_eval reports afterwards). A pose that is not finite, or a range that is NaN, negative or infinite:
// nothing.
template <int PASS, int KIND>
__device__ __forceinline__ void queryBoxesWave(DW W, const float4* boxes, const QueryPose* poses, const ShapeRec* qshapes, int n,
                                               uint32_t mask, int sensors, int* counts, const int* offsets, int* items)
{
	const int lane = (int)(threadIdx.x & 63u);
	const int nWaves = (int)((gridDim.x * blockDim.x) >> 6);
	for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nWaves)
	{
		float4 b;
		Xf xfQ;
		GjkProxy pQ;
		bool nan = false;
		float range = 0.0f;
		if (KIND == QUERY_SHAPE || KIND == QUERY_RANGE)
		{
			const QueryPose qp = poses[i];
			nan = isnan(qp.x) || isnan(qp.y) || isnan(qp.c) || isnan(qp.s);
			if (KIND == QUERY_RANGE)
			{
				range = qp.tx;
				nan = !queryRangeValid(qp);
			}
			xfQ = queryPoseXf(qp);
			const ShapeRec* rec = qshapes + qp.shape;
			pQ = b2dProxy(rec);
			const AABB qa = b2dShapeAABB(rec, xfQ);
			b = make_float4(qa.lo.x, qa.lo.y, qa.hi.x, qa.hi.y);
			if (KIND == QUERY_RANGE) b = make_float4(qa.lo.x - range, qa.lo.y - range, qa.hi.x + range, qa.hi.y + range);
		}
		else b = boxes[i];
		if (nan || !(b.x <= b.z && b.y <= b.w)) // (lower > upper, or a NaN: nothing)
		{
			if (PASS == 0 && lane == 0) counts[i] = 0;
			continue;
		}
		AABB a;
		a.lo = v2(b.x, b.y);
		a.hi = v2(b.z, b.w);
		int found = 0;
		const int at = PASS == 1 ? offsets[i] : 0, end = PASS == 1 ? offsets[i + 1] : 0;
		auto visit = [&](bool valid, int q, float4 fat)
		{
			bool hit = false;
			if (valid)
			{
				AABB f;
				f.lo = v2(fat.x, fat.y);
				f.hi = v2(fat.z, fat.w);
				hit = b2dAabbOverlap(a, f) && queryFilterPasses(W, q, mask, sensors);
				if (KIND == QUERY_POINT && hit) hit = b2dShapeTestPoint(W.shapes + W.p_shape[q], loadXf(W.b_xf, W.p_body[q]), a.lo);
				if (KIND == QUERY_SHAPE && hit) hit = queryDistance(W, q, pQ, xfQ).distance < 10.0f * B2D_EPSILON;
				if (KIND == QUERY_RANGE && hit) hit = queryDistance(W, q, pQ, xfQ).distance <= range;
			}
			const unsigned long long m = __ballot(hit);
			if (PASS == 1 && hit)
			{
				const int k = at + found + (int)__popcll(m & ((1ull << lane) - 1ull));
				if (k < end) items[k] = q;
			}
			found += (int)__popcll(m);
		};
		if (queryVisitGrid(W, lane, b, visit)) queryVisitLarge(W, lane, visit);
		else queryVisitAll(W, lane, visit);
		if (PASS == 0 && lane == 0) counts[i] = found;
	}
}

__global__ __launch_bounds__(256) void k_query_aabbs_count(DW W, const float4* boxes, int n, uint32_t mask, int sensors, int* counts)
{
	queryBoxesWave<0, QUERY_BOX>(W, boxes, nullptr, nullptr, n, mask, sensors, counts, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void k_query_aabbs_fill(DW W, const float4* boxes, int n, uint32_t mask, int sensors, const int* offsets, int* items)
{
	queryBoxesWave<1, QUERY_BOX>(W, boxes, nullptr, nullptr, n, mask, sensors, nullptr, offsets, items);
}
__global__ __launch_bounds__(256) void k_query_points_count(DW W, const float4* boxes, int n, uint32_t mask, int sensors, int* counts)
{
	queryBoxesWave<0, QUERY_POINT>(W, boxes, nullptr, nullptr, n, mask, sensors, counts, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void k_query_points_fill(DW W, const float4* boxes, int n, uint32_t mask, int sensors, const int* offsets, int* items)
{
	queryBoxesWave<1, QUERY_POINT>(W, boxes, nullptr, nullptr, n, mask, sensors, nullptr, offsets, items);
}
__global__ __launch_bounds__(256) void k_query_shapes_count(DW W, const QueryPose* poses, const ShapeRec* qshapes, int n, uint32_t mask,
                                                            int sensors, int* counts)
{
	queryBoxesWave<0, QUERY_SHAPE>(W, nullptr, poses, qshapes, n, mask, sensors, counts, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void k_query_shapes_fill(DW W, const QueryPose* poses, const ShapeRec* qshapes, int n, uint32_t mask,
                                                           int sensors, const int* offsets, int* items)
{
	queryBoxesWave<1, QUERY_SHAPE>(W, nullptr, poses, qshapes, n, mask, sensors, nullptr, offsets, items);
}
__global__ __launch_bounds__(256) void k_query_ranges_count(DW W, const QueryPose* poses, const ShapeRec* qshapes, int n, uint32_t mask,
                                                            int sensors, int* counts)
{
	queryBoxesWave<0, QUERY_RANGE>(W, nullptr, poses, qshapes, n, mask, sensors, counts, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void k_query_ranges_fill(DW W, const QueryPose* poses, const ShapeRec* qshapes, int n, uint32_t mask,
                                                           int sensors, const int* offsets, int* items)
{
	queryBoxesWave<1, QUERY_RANGE>(W, nullptr, poses, qshapes, n, mask, sensors, nullptr, offsets, items);
}

// One workgroup per query: its items sorted ascending in LDS (bitonic network over the next power of two, padded with
// `pad`, the largest value). Lists longer than QUERY_SORT_MAX are left to k_query_mark / k_query_compact_big (fixture ids)
// or k_query_sort_keys_big (ray keys).
template <typename T>
__device__ __forceinline__ void querySortLists(const int* offsets, int n, T* items, T pad, T* s)
{
	for (int i = blockIdx.x; i < n; i += gridDim.x)
	{
		const int at = offsets[i], len = offsets[i + 1] - at;
		if (len <= 1 || len > QUERY_SORT_MAX) continue;
		int size = 2;
		while (size < len) size <<= 1;
		for (int k = threadIdx.x; k < size; k += blockDim.x) s[k] = k < len ? items[at + k] : pad;
		__syncthreads();
		for (int span = 2; span <= size; span <<= 1)
		{
			for (int j = span >> 1; j > 0; j >>= 1)
			{
				for (int k = threadIdx.x; k < size; k += blockDim.x)
				{
					const int other = k ^ j;
					if (other > k)
					{
						const T x = s[k], y = s[other];
						const bool up = (k & span) == 0;
						if (up ? x > y : x < y)
						{
							s[k] = y;
							s[other] = x;
						}
					}
				}
				__syncthreads();
			}
		}
		for (int k = threadIdx.x; k < len; k += blockDim.x) items[at + k] = s[k];
		__syncthreads();
	}
}
__global__ __launch_bounds__(QUERY_SORT_THREADS) void k_query_sort(const int* offsets, int n, int* items)
{
	__shared__ int s[QUERY_SORT_MAX];
	querySortLists<int>(offsets, n, items, 0x7fffffff, s);
}
// the (fraction bits, fixture id) keys of b2hip_ray_cast_all: 32 KB of LDS
__global__ __launch_bounds__(QUERY_SORT_THREADS) void k_query_sort_keys(const int* offsets, int n, unsigned long long* keys)
{
	__shared__ unsigned long long s[QUERY_SORT_MAX];
	querySortLists<unsigned long long>(offsets, n, keys, ~0ull, s);
}

// A ray with more than QUERY_SORT_MAX hits: the same network over global memory from ONE workgroup (its barrier orders the
// rounds), in `work` (size = the next power of two >= len, padded with ~0), and back. One launch per such ray, one after
// the other from the host: correct, and the slow case of b2hip_ray_cast_all (len = 8192: 91 rounds of 4 exchanges a thread).
__global__ __launch_bounds__(1024) void k_query_sort_keys_big(unsigned long long* keys, int len, unsigned long long* work, int size)
{
	for (int k = threadIdx.x; k < size; k += blockDim.x) work[k] = k < len ? keys[k] : ~0ull;
	__syncthreads();
	for (int span = 2; span <= size; span <<= 1)
	{
		for (int j = span >> 1; j > 0; j >>= 1)
		{
			for (int k = threadIdx.x; k < size; k += blockDim.x)
			{
				const int other = k ^ j;
				if (other > k)
				{
					const unsigned long long x = work[k], y = work[other];
					const bool up = (k & span) == 0;
					if (up ? x > y : x < y)
					{
						work[k] = y;
						work[other] = x;
					}
				}
			}
			__syncthreads();
		}
	}
	for (int k = threadIdx.x; k < len; k += blockDim.x) keys[k] = work[k];
}

// A query with more than QUERY_SORT_MAX items (a box over much of the world): its fixture ids - distinct - are marked in a
// flag per proxy, and k_query_compact_big writes the marked ids back in proxy order, clearing the flags behind it. Cost: two
// launches per such query, one after the other from the host, and ONE workgroup walking all nProxies flags - a batch of k
// wide boxes on a world of N proxies costs k x N flag reads on one CU (10^6 proxies: 1 000 rounds of 1 024 flags per query).
__global__ __launch_bounds__(256) void k_query_mark(const int* items, int len, int* flags)
{
	for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < len; k += gridDim.x * blockDim.x) flags[items[k]] = 1;
}
__global__ __launch_bounds__(1024) void k_query_compact_big(int* flags, int nProxies, int* out)
{
	__shared__ int s_wave[16];
	__shared__ int s_run;
	const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
	if (tid == 0) s_run = 0;
	__syncthreads();
	for (int base = 0; base < nProxies; base += 1024)
	{
		const int p = base + tid;
		const bool on = p < nProxies && flags[p] != 0;
		const unsigned long long m = __ballot(on);
		if (lane == 0) s_wave[wv] = (int)__popcll(m);
		__syncthreads();
		int before = s_run;
		for (int q = 0; q < wv; ++q) before += s_wave[q];
		if (on)
		{
			out[before + (int)__popcll(m & ((1ull << lane) - 1ull))] = p;
			flags[p] = 0;
		}
		__syncthreads();
		if (tid == 0)
		{
			int add = 0;
			for (int q = 0; q < 16; ++q) add += s_wave[q];
			s_run += add;
		}
		__syncthreads();
	}
}

__device__ __forceinline__ unsigned long long waveMinU64(unsigned long long v)
{
	for (int off = 32; off > 0; off >>= 1)
	{
		const unsigned long long o = __shfl_xor(v, off);
		v = o < v ? o : v;
	}
	return v;
}

// the record of a hit of fixture q by the ray p1 -> p2: the shape's cast once more (fraction, -0.0 included, and normal)
__device__ __forceinline__ b2hip_ray_hit queryRayRecord(const DW& W, int q, V2 p1, V2 p2)
{
	const int body = W.p_body[q];
	RayHit hit;
	(void)b2dShapeRayCast(W.shapes + W.p_shape[q], loadXf(W.b_xf, body), p1, p2, 1.0f, &hit);
	const float f = hit.fraction;
	b2hip_ray_hit o;
	o.fixture = q;
	o.body = body;
	o.point_x = (1.0f - f) * p1.x + f * p2.x;
	o.point_y = (1.0f - f) * p1.y + f * p2.y;
	o.normal_x = hit.normal.x;
	o.normal_y = hit.normal.y;
	o.fraction = f;
	o.pad = 0;
	return o;
}

// A walk in pieces about a cell long (rays, and the translation of a shape cast): how many pieces a length takes - 0: more
// than QUERY_WINDOW_MAX, the caller scans every proxy instead - and the fractions [t0, t1] of piece k. The last piece ends at
// 1 exactly, and a piece's t1 is the next piece's t0 to the bit: the same division of the same integers.
__device__ __forceinline__ int queryPieceCount(const DW& W, float len)
{
	const float pieces = ceilf(len / gridCell(W));
	if (!(pieces <= (float)QUERY_WINDOW_MAX)) return 0;
	return pieces < 1.0f ? 1 : (int)pieces;
}
__device__ __forceinline__ void queryPieceSpan(int k, int np, float* t0, float* t1)
{
	*t0 = (float)k / (float)np;
	*t1 = k + 1 == np ? 1.0f : (float)(k + 1) / (float)np;
}

// One ray of a batch, set up once from its float4, and the ONLY text of the ray walk's arithmetic: k_query_rays (closest)
// and queryRayHitsWave (all hits, any hit) both cull their candidates by cull() and cut the ray by pieceCount() / piece(), and
// keep no expression of their own. That is what makes their answers agree to the bit - b2hip_ray_cast_all's first record of
// a ray IS b2hip_ray_cast_closest's, any == (closest hits something) - also for a ray that grazes a fat box at a piece
// boundary: both walks see the same boxes, the same margins and the same t0 / t1. The build contracts nothing
// (-ffp-contract=off), so an expression rounds the same wherever it is inlined; an edit here moves both walks together.
// Only `valid` means anything for a ray that is not valid (a zero length leaves NaN in perp): test it before any other use.
struct QueryRay
{
	V2 p1, p2, d;
	bool valid;     // finite and not of zero length: anything else hits nothing
	float mag, eps; // the largest coordinate; the margin that covers rounding, growing with it
	float len;
	V2 perp, aperp; // the unit normal of the ray, and its absolute value
	V2 slo, shi;    // the ray's own box, grown by eps

	__device__ __forceinline__ explicit QueryRay(float4 r)
	{
		p1 = v2(r.x, r.y);
		p2 = v2(r.z, r.w);
		d = p2 - p1;
		valid = isfinite(r.x) && isfinite(r.y) && isfinite(r.z) && isfinite(r.w) && (d.x != 0.0f || d.y != 0.0f);
		mag = fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fmaxf(fabsf(r.z), fabsf(r.w)));
		eps = 1.0e-3f + 1.0e-5f * mag;
		len = sqrtf(d.x * d.x + d.y * d.y);
		const V2 u = v2(d.x / len, d.y / len);
		perp = v2(-u.y, u.x);
		aperp = v2(fabsf(perp.x), fabsf(perp.y));
		slo = v2(fminf(p1.x, p2.x) - eps, fminf(p1.y, p2.y) - eps);
		shi = v2(fmaxf(p1.x, p2.x) + eps, fmaxf(p1.y, p2.y) + eps);
	}

	// true: the segment cannot meet the fat box - the boxes apart, then the ray's normal as a separating axis (k_query_rays)
	__device__ __forceinline__ bool cull(float4 fat) const
	{
		if (fat.x > shi.x || fat.y > shi.y || slo.x > fat.z || slo.y > fat.w) return true;
		const V2 c = v2(0.5f * (fat.x + fat.z), 0.5f * (fat.y + fat.w));
		const V2 h = v2(0.5f * (fat.z - fat.x) + eps, 0.5f * (fat.w - fat.y) + eps);
		const V2 rel = p1 - c;
		return !(fabsf(perp.x * rel.x + perp.y * rel.y) - (aperp.x * h.x + aperp.y * h.y) <= 0.0f);
	}

	// how many pieces the walk takes; 0: too many, or a coordinate beyond QUERY_COORD_MAX - every proxy is scanned instead
	__device__ __forceinline__ int pieceCount(const DW& W) const
	{
		const int np = queryPieceCount(W, len);
		return mag <= QUERY_COORD_MAX ? np : 0;
	}

	// piece k of np: its fractions and its box, grown by eps; the last piece ends at p2 itself
	__device__ __forceinline__ float4 piece(int k, int np, float* t0, float* t1) const
	{
		queryPieceSpan(k, np, t0, t1);
		const V2 a = p1 + *t0 * d, b = k + 1 == np ? p2 : p1 + *t1 * d;
		return make_float4(fminf(a.x, b.x) - eps, fminf(a.y, b.y) - eps, fmaxf(a.x, b.x) + eps, fmaxf(a.y, b.y) + eps);
	}
};

// Closest ray hit, one WAVE per ray. The ray is cut into pieces about a cell long; the cells of a piece's box (grown by
// half the grid limit, gridWindow) hold every grid-sized proxy whose box the piece can meet, so after piece k every hit at
// a fraction up to its end t1 has been seen: the walk stops once the best fraction is below t1. Large proxies are tested
// by every ray. A candidate is culled by the segment against its fat AABB (b2DynamicTree::RayCast's two tests, the box
// grown by a margin that covers rounding: only boxes the reference culls as well), then cast against its shape at the
// body's transform with maxFraction 1 (the fraction and normal of a hit do not depend on maxFraction). Best = the smallest
// (fraction bits, fixture id): fractions are >= 0 (a -0.0 enters as +0.0), so their bits order like the values, and ties
// go to the lower id. A ray of more than QUERY_WINDOW_MAX pieces (or with a coordinate beyond QUERY_COORD_MAX) tests every
// proxy of the world from its one wave instead: 10^6 candidates on a 10^6-body world - a scan is still cheaper than
// thousands of pieces, but it is the slow case of this kernel.
__global__ __launch_bounds__(256) void k_query_rays(DW W, const float4* rays, int n, uint32_t mask, int sensors, b2hip_ray_hit* out)
{
	const int lane = (int)(threadIdx.x & 63u);
	const int nWaves = (int)((gridDim.x * blockDim.x) >> 6);
	for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nWaves)
	{
		const QueryRay ray(rays[i]);
		unsigned long long best = ~0ull;
		if (ray.valid)
		{
			auto visit = [&](bool valid, int q, float4 fat)
			{
				if (valid && !ray.cull(fat) && queryFilterPasses(W, q, mask, sensors))
				{
					RayHit hit;
					if (b2dShapeRayCast(W.shapes + W.p_shape[q], loadXf(W.b_xf, W.p_body[q]), ray.p1, ray.p2, 1.0f, &hit))
					{
						// (+ 0.0f: a ray that starts on an edge or a circle is hit at -0.0, whose bits would sort after
						// every positive fraction; the kept hit's own fraction, -0.0 included, is reported below)
						const unsigned long long key = queryKey(__float_as_uint(hit.fraction + 0.0f), q);
						best = key < best ? key : best;
					}
				}
			};
			queryVisitLarge(W, lane, visit);
			const int np = ray.pieceCount(W);
			bool all = np == 0;
			for (int k = 0; k < np; ++k)
			{
				float t0, t1;
				if (!queryVisitGrid(W, lane, ray.piece(k, np, &t0, &t1), visit))
				{
					all = true;
					break;
				}
				best = waveMinU64(best);
				if (best != ~0ull && queryKeyValue(best) < t1) break;
			}
			if (all) queryVisitAll(W, lane, visit);
			best = waveMinU64(best);
		}
		// (the kept hit again: its normal)
		if (lane == 0) out[i] = best != ~0ull ? queryRayRecord(W, queryKeyFixture(best), ray.p1, ray.p2) : queryRayMiss();
	}
}

// Every hit of a ray (b2hip_ray_cast_all) and whether there is one (b2hip_ray_cast_any), one WAVE per ray, walked and culled
// by the QueryRay that k_query_rays walks (one text: a piece's t1 is the next piece's t0 to the bit). MODE QUERY_RAY_COUNT:
// counts[i] = hits of ray i; QUERY_RAY_FILL: their keys (bits of fraction + 0.0f) << 32 | fixture id, unsorted, at
// keys[offsets[i] ...]; QUERY_RAY_ANY: any[i] = 1 when something is hit.
// Once only: the windows of successive pieces overlap (gridWindow grows a piece's box by half the grid limit), so a grid-sized
// proxy is met in several pieces. Piece k accepts a hit only when t0 <= fraction + 0.0f < t1, the last piece up to and
// including 1: fractions lie in [0, 1] and the pieces' [t0, t1) tile it, so exactly one piece accepts; and that piece meets
// the proxy - the hit point lies in the piece's box and in the proxy's fat box, so the proxy's centre is in the piece's
// window (k_query_rays' invariant: after piece k every hit up to t1 has been seen). The rule looks at the fraction alone,
// never at the order inside a bucket. Large proxies are visited once and accept every hit. A walk the grid refuses (more than
// QUERY_WINDOW_MAX pieces, a coordinate beyond QUERY_COORD_MAX, a piece's box grown past it) starts over as a scan of every
// proxy, which also meets each once. The count and the fill pass take the same decisions from the same inputs.
// Any hit: the same walk with no key kept; once a ballot holds a hit the remaining candidates of that visit are skipped and
// the walk leaves. It equals `the closest hit exists`: both walks only stop early on a hit.
#define QUERY_RAY_COUNT 0
#define QUERY_RAY_FILL 1
#define QUERY_RAY_ANY 2

template <int MODE>
__device__ __forceinline__ void queryRayHitsWave(DW W, const float4* rays, int n, uint32_t mask, int sensors, int* counts, const int* offsets,
                                                 unsigned long long* keys, uint8_t* any)
{
	const int lane = (int)(threadIdx.x & 63u);
	const int nWaves = (int)((gridDim.x * blockDim.x) >> 6);
	for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nWaves)
	{
		const QueryRay ray(rays[i]);
		int found = 0;
		if (ray.valid)
		{
			const int at = MODE == QUERY_RAY_FILL ? offsets[i] : 0, end = MODE == QUERY_RAY_FILL ? offsets[i + 1] : 0;
			float t0 = 0.0f, t1 = 1.0f; // a hit counts when t0 <= fraction + 0.0f < t1 - or <= t1 when `closed`
			bool closed = true;
			auto visit = [&](bool valid, int q, float4 fat)
			{
				bool hit = false;
				float f = 0.0f;
				if (valid && !(MODE == QUERY_RAY_ANY && found > 0) && !ray.cull(fat) && queryFilterPasses(W, q, mask, sensors))
				{
					RayHit rh;
					if (b2dShapeRayCast(W.shapes + W.p_shape[q], loadXf(W.b_xf, W.p_body[q]), ray.p1, ray.p2, 1.0f, &rh))
					{
						f = rh.fraction + 0.0f; // (a -0.0 enters as +0.0, as in k_query_rays)
						hit = MODE == QUERY_RAY_ANY || (f >= t0 && (f < t1 || closed));
					}
				}
				const unsigned long long m = __ballot(hit);
				if (MODE == QUERY_RAY_FILL && hit)
				{
					const int k = at + found + (int)__popcll(m & ((1ull << lane) - 1ull));
					if (k < end) keys[k] = queryKey(__float_as_uint(f), q);
				}
				found += (int)__popcll(m);
			};
			const int np = ray.pieceCount(W);
			bool all = np == 0;
			if (!all) queryVisitLarge(W, lane, visit);
			for (int k = 0; k < np && !(MODE == QUERY_RAY_ANY && found > 0); ++k)
			{
				closed = k + 1 == np;
				if (!queryVisitGrid(W, lane, ray.piece(k, np, &t0, &t1), visit))
				{
					all = true;
					break;
				}
			}
			if (all)
			{
				if (MODE != QUERY_RAY_ANY) found = 0; // (the scan meets every proxy once: what the walk gathered is gathered again)
				t0 = 0.0f;
				t1 = 1.0f;
				closed = true;
				queryVisitAll(W, lane, visit);
			}
		}
		if (lane == 0)
		{
			if (MODE == QUERY_RAY_COUNT) counts[i] = found;
			if (MODE == QUERY_RAY_ANY) any[i] = found > 0 ? 1 : 0;
		}
	}
}

__global__ __launch_bounds__(256) void k_query_rays_all_count(DW W, const float4* rays, int n, uint32_t mask, int sensors, int* counts)
{
	queryRayHitsWave<QUERY_RAY_COUNT>(W, rays, n, mask, sensors, counts, nullptr, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void k_query_rays_all_fill(DW W, const float4* rays, int n, uint32_t mask, int sensors, const int* offsets,
                                                             unsigned long long* keys)
{
	queryRayHitsWave<QUERY_RAY_FILL>(W, rays, n, mask, sensors, nullptr, offsets, keys, nullptr);
}
__global__ __launch_bounds__(256) void k_query_rays_any(DW W, const float4* rays, int n, uint32_t mask, int sensors, uint8_t* any)
{
	queryRayHitsWave<QUERY_RAY_ANY>(W, rays, n, mask, sensors, nullptr, nullptr, nullptr, any);
}

// The records of b2hip_ray_cast_all, after the sort: one thread per key. Key k belongs to ray queryOwner(k); its fixture is
// cast again and the record written out whole.
__global__ __launch_bounds__(256) void k_query_rays_all_eval(DW W, const float4* rays, int n, const int* offsets, const unsigned long long* keys,
                                                             int nItems, b2hip_ray_hit* out)
{
	for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < nItems; k += (int)(gridDim.x * blockDim.x))
	{
		const float4 r = rays[queryOwner(offsets, n, k)];
		out[k] = queryRayRecord(W, queryKeyFixture(keys[k]), v2(r.x, r.y), v2(r.z, r.w));
	}
}

// Closest shape cast, one WAVE per cast (b2hip_shape_cast_closest), walked as k_query_rays walks a ray. The sweep box is the
// union of the query shape's AABB at the pose and at the pose moved by the translation; a candidate is a live proxy passing
// the filter whose fat AABB overlaps the WHOLE sweep box, whichever cells it was found in, so the answer does not depend on
// the walk. Its hit is b2ShapeCast with the fixture's child at its body's transform as proxy A, the query shape at the
// pose as proxy B and the translation as B's (the Testbed's ShapeCast.h); best = the smallest (lambda bits, fixture id).
// The walk: large proxies first; then the sweep box's window once when it has at most QUERY_WINDOW_MAX cells; else the
// translation in cell-long pieces, piece k's box being the shape's box swept over [t0, t1] grown by `margin`, stopping once
// the best lambda is below t1; else (too many pieces, or a coordinate beyond QUERY_COORD_MAX) every proxy of the world.
// The margin: b2ShapeCast reports a hit once the cores are within sigma + tolerance, sigma = the two skins less
// b2_polygonRadius, a skin being the shape's radius or b2_polygonRadius if that is larger. The query box holds the query
// shape's radius and a fixture's fat box its own (none for a chain link) plus b2_aabbExtension, so the cores' reach beyond
// the tight boxes is at most 2 b2_polygonRadius + tolerance - both skins at b2_polygonRadius over a zero radius - taken
// here on top of a rounding term that grows with the coordinates' magnitude.
__global__ __launch_bounds__(256) void k_query_shape_casts(DW W, const QueryPose* casts, const ShapeRec* qshapes, int n, uint32_t mask,
                                                           int sensors, b2hip_ray_hit* out)
{
	const int lane = (int)(threadIdx.x & 63u);
	const int nWaves = (int)((gridDim.x * blockDim.x) >> 6);
	for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nWaves)
	{
		const QueryPose qp = casts[i];
		const ShapeRec* rec = qshapes + qp.shape;
		const GjkProxy pB = b2dProxy(rec);
		const Xf xfB = queryPoseXf(qp);
		const V2 t = v2(qp.tx, qp.ty);
		unsigned long long best = ~0ull;
		const bool finite = isfinite(qp.x) && isfinite(qp.y) && isfinite(qp.c) && isfinite(qp.s) && isfinite(qp.tx) && isfinite(qp.ty);
		if (finite)
		{
			Xf xfEnd = xfB;
			xfEnd.p = xfB.p + t;
			const AABB box0 = b2dShapeAABB(rec, xfB);
			const AABB sweep = b2dAabbCombine(box0, b2dShapeAABB(rec, xfEnd));
			const float mag = fmaxf(fmaxf(fabsf(sweep.lo.x), fabsf(sweep.lo.y)), fmaxf(fabsf(sweep.hi.x), fabsf(sweep.hi.y)));
			const float margin = 1.0e-3f + 1.0e-5f * mag + 2.0f * B2D_POLYGON_RADIUS + 0.5f * B2D_LINEAR_SLOP;
			auto visit = [&](bool valid, int q, float4 fat)
			{
				bool cand = valid && !(fat.x > sweep.hi.x || fat.y > sweep.hi.y || sweep.lo.x > fat.z || sweep.lo.y > fat.w);
				if (cand) cand = queryFilterPasses(W, q, mask, sensors);
				if (cand)
				{
					ShapeCastResult r;
					if (b2dShapeCast(&r, b2dProxy(W.shapes + W.p_shape[q]), loadXf(W.b_xf, W.p_body[q]), pB, xfB, t))
					{
						const unsigned long long key = queryKey(__float_as_uint(r.lambda + 0.0f), q);
						best = key < best ? key : best;
					}
				}
			};
			queryVisitLarge(W, lane, visit);
			bool all = !(mag <= QUERY_COORD_MAX);
			const float4 whole = make_float4(sweep.lo.x, sweep.lo.y, sweep.hi.x, sweep.hi.y);
			if (!all && !queryVisitGrid(W, lane, whole, visit))
			{
				const float len = sqrtf(t.x * t.x + t.y * t.y);
				const int np = queryPieceCount(W, len);
				all = np == 0;
				if (!all)
				{
					for (int k = 0; k < np; ++k)
					{
						float t0, t1;
						queryPieceSpan(k, np, &t0, &t1);
						const V2 a = t0 * t, b = t1 * t;
						const float4 box = make_float4(box0.lo.x + fminf(a.x, b.x) - margin, box0.lo.y + fminf(a.y, b.y) - margin,
						                               box0.hi.x + fmaxf(a.x, b.x) + margin, box0.hi.y + fmaxf(a.y, b.y) + margin);
						if (!queryVisitGrid(W, lane, box, visit))
						{
							all = true;
							break;
						}
						best = waveMinU64(best);
						if (best != ~0ull && queryKeyValue(best) < t1) break;
					}
				}
			}
			if (all) queryVisitAll(W, lane, visit);
			best = waveMinU64(best);
		}
		if (lane == 0)
		{
			b2hip_ray_hit o = queryRayMiss();
			if (best != ~0ull)
			{
				const int q = queryKeyFixture(best);
				const int body = W.p_body[q];
				ShapeCastResult r;
				(void)b2dShapeCast(&r, b2dProxy(W.shapes + W.p_shape[q]), loadXf(W.b_xf, body), pB, xfB, t); // (the kept hit again)
				o.fixture = q;
				o.body = body;
				o.point_x = r.point.x;
				o.point_y = r.point.y;
				o.normal_x = r.normal.x;
				o.normal_y = r.normal.y;
				o.fraction = r.lambda;
			}
			out[i] = o;
		}
	}
}

// The records of b2hip_query_shapes_within, after the sort (it moves bare fixture ids): one thread per item. Item k belongs
// to query queryOwner(k); its distance is computed again, as the fill pass computed it, and written out whole.
__global__ __launch_bounds__(256) void k_query_range_eval(DW W, const QueryPose* poses, const ShapeRec* qshapes, int n, const int* offsets,
                                                          const int* items, int nItems, b2hip_distance_hit* out)
{
	for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < nItems; k += (int)(gridDim.x * blockDim.x))
	{
		const QueryPose qp = poses[queryOwner(offsets, n, k)];
		out[k] = queryDistanceRecord(W, items[k], b2dProxy(qshapes + qp.shape), queryPoseXf(qp));
	}
}

// Closest fixture within a range, one WAVE per query (b2hip_shape_distance_closest). The query box is the query shape's AABB
// at the pose grown by max_distance; a candidate is a live proxy passing the filter whose fat AABB overlaps the WHOLE query
// box, whichever cells it was found in, and whose distance (queryDistance) is <= max_distance; best = the smallest
// (distance bits, fixture id) - distances are >= +0, so their bits order like the values. The walk does not pay for the
// whole range when something is near: large proxies first, then the grid windows of the shape's box grown by r = one cell,
// then 2, 4, ... cells, the last ring being the whole query box; it stops once the best distance is below r - margin. Why
// that is sound: queryVisitGrid shows every grid-sized proxy whose fat box overlaps the ring's box, so one not yet seen has
// a fat box clear of the shape's box by more than r on some axis. The shape's box holds the query shape with its skin and a
// fat box the fixture's with its skin - except for a chain link, whose box leaves its b2_polygonRadius out - so the
// unseen proxy is farther than r - 2 b2_polygonRadius: margin = those plus the rounding term the rays and casts use. A
// proxy whose fat box overlaps the previous ring's box was evaluated there and is skipped (the minimum would not change).
// A ring of more than QUERY_WINDOW_MAX cells, or a coordinate beyond QUERY_COORD_MAX, scans every proxy of the world.
__global__ __launch_bounds__(256) void k_query_shape_distances(DW W, const QueryPose* poses, const ShapeRec* qshapes, int n, uint32_t mask,
                                                               int sensors, b2hip_distance_hit* out)
{
	const int lane = (int)(threadIdx.x & 63u);
	const int nWaves = (int)((gridDim.x * blockDim.x) >> 6);
	for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nWaves)
	{
		const QueryPose qp = poses[i];
		const ShapeRec* rec = qshapes + qp.shape;
		const GjkProxy pQ = b2dProxy(rec);
		const Xf xfQ = queryPoseXf(qp);
		const float range = qp.tx;
		unsigned long long best = ~0ull;
		if (queryRangeValid(qp))
		{
			const AABB box0 = b2dShapeAABB(rec, xfQ);
			const float4 whole = make_float4(box0.lo.x - range, box0.lo.y - range, box0.hi.x + range, box0.hi.y + range);
			const float mag = fmaxf(fmaxf(fabsf(whole.x), fabsf(whole.y)), fmaxf(fabsf(whole.z), fabsf(whole.w)));
			const float margin = 1.0e-3f + 1.0e-5f * mag + 2.0f * B2D_POLYGON_RADIUS;
			const float inf = __uint_as_float(0x7f800000u);
			float4 done = make_float4(inf, inf, -inf, -inf); // the ring already evaluated (none yet: lower = +inf overlaps no box)
			auto visit = [&](bool valid, int q, float4 fat)
			{
				bool cand = valid && !(fat.x > whole.z || fat.y > whole.w || whole.x > fat.z || whole.y > fat.w);
				if (cand) cand = fat.x > done.z || fat.y > done.w || done.x > fat.z || done.y > fat.w;
				if (cand) cand = queryFilterPasses(W, q, mask, sensors);
				if (cand)
				{
					const float dist = queryDistance(W, q, pQ, xfQ).distance;
					if (dist <= range)
					{
						const unsigned long long key = queryKey(__float_as_uint(dist), q);
						best = key < best ? key : best;
					}
				}
			};
			queryVisitLarge(W, lane, visit);
			bool all = !(mag <= QUERY_COORD_MAX);
			if (!all)
			{
				for (float r = fmaxf(gridCell(W), B2D_LINEAR_SLOP);; r *= 2.0f) // (never 0: the rings must grow)
				{
					const bool last = !(r < range);
					const float4 box = last ? whole : make_float4(box0.lo.x - r, box0.lo.y - r, box0.hi.x + r, box0.hi.y + r);
					if (!queryVisitGrid(W, lane, box, visit))
					{
						all = true;
						break;
					}
					best = waveMinU64(best);
					if (last || (best != ~0ull && queryKeyValue(best) < r - margin)) break;
					done = box;
				}
			}
			if (all) queryVisitAll(W, lane, visit);
			best = waveMinU64(best);
		}
		if (lane == 0)
		{
			// (the kept candidate again)
			out[i] = best != ~0ull ? queryDistanceRecord(W, queryKeyFixture(best), pQ, xfQ) : queryDistanceMiss();
		}
	}
}

#endif
