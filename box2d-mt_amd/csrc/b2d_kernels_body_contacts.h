// b2d_kernels_body_contacts.h - per-body contact lists and contact totals (include/b2hip.h: b2hip_body_contacts,
// b2hip_body_contact_totals; host side: b2hip_api_body_contacts.h).
//
// A batch names n bodies. `slot` maps a body id to its place in the batch (-1: not asked for). Two passes walk the world's
// CURRENT contact array, a thread per contact, reading ids (16 B) and flags (4 B): k_bc_count adds to the two counters of
// every asked-for body the contact names (all contacts, touching ones), k_bc_fill hands out places in the body's part of the
// list and writes the contact's index there. The parts are then sorted ascending (k_query_sort; a part of more than
// QUERY_SORT_MAX by k_query_mark / k_query_compact_big over a flag per contact), and k_bc_records (a thread per record) or
// k_bc_totals (a wave per body) read the manifolds, the impulses and the two bodies' transforms.
// Nothing the step reads is written, and there is no float atomic: a body's totals are summed by one wave over its sorted
// list - lane l takes the entries l, l + 64, ... in list order, one fixed butterfly combines the lanes - so the same list
// gives the same bytes.
// Same-address adds: a static ground asked for in the batch receives one add per contact it has on ONE word; the count goes
// through blockHotAddInt (a workgroup's sum for its first key stays in LDS), the fill through waveRunAlloc (one atomic per
// run of neighbouring lanes with the same body: contacts are created in key order, those of one fixture sit side by side).
#ifndef B2D_KERNELS_BODY_CONTACTS_H
#define B2D_KERNELS_BODY_CONTACTS_H

#include "b2d_kernels_query.h"
#include "b2d_wave.h"

__global__ __launch_bounds__(256) void k_bc_slots(const int* bodies, int n, int* slot, int nBodies)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int b = bodies[i];
		if ((unsigned)b < (unsigned)nBodies) slot[b] = i; // (the host has checked the ids: in range, each once)
	}
}

// the batch slots of contact k's two bodies (-1: not asked for, or no contact k) and whether it touches
__device__ __forceinline__ void bcContactSlots(const int4* ids, const uint32_t* flags, int nContacts, const int* slot, int nBodies, int k,
                                               int& slotA, int& slotB, bool& touching)
{
	slotA = -1;
	slotB = -1;
	touching = false;
	if (k >= nContacts) return;
	const int4 id = ids[k];
	if ((unsigned)id.z < (unsigned)nBodies) slotA = slot[id.z];
	if ((unsigned)id.w < (unsigned)nBodies) slotB = slot[id.w];
	touching = (flags[k] & CF_TOUCHING) != 0u;
}

// countAll[s] / countTouching[s] += the contacts that name the body of slot s. Every thread of a workgroup goes through the
// same rounds (the helpers of b2d_wave.h want wave-uniform control flow, blockHotFlush a barrier).
__global__ __launch_bounds__(256) void k_bc_count(const int4* ids, const uint32_t* flags, int nContacts, const int* slot, int nBodies,
                                                  int* countAll, int* countTouching)
{
	__shared__ BlockHot hotAll, hotTouching;
	blockHotInit(&hotAll);
	blockHotInit(&hotTouching);
	const int stride = (int)(gridDim.x * blockDim.x);
	for (int base = (int)(blockIdx.x * blockDim.x); base < nContacts; base += stride)
	{
		int slotA, slotB;
		bool touching;
		bcContactSlots(ids, flags, nContacts, slot, nBodies, base + (int)threadIdx.x, slotA, slotB, touching);
		blockHotAddInt(&hotAll, countAll, slotA, 1, slotA >= 0);
		blockHotAddInt(&hotAll, countAll, slotB, 1, slotB >= 0);
		blockHotAddInt(&hotTouching, countTouching, slotA, 1, touching && slotA >= 0);
		blockHotAddInt(&hotTouching, countTouching, slotB, 1, touching && slotB >= 0);
	}
	blockHotFlush(&hotAll, countAll);
	blockHotFlush(&hotTouching, countTouching);
}

// items[offsets[s] + place] = k for every listed contact k of slot s's body (unsorted: places go in arrival order);
// cursor: zero at the launch, one word per slot.
__global__ __launch_bounds__(256) void k_bc_fill(const int4* ids, const uint32_t* flags, int nContacts, const int* slot, int nBodies,
                                                 int touchingOnly, const int* offsets, int* cursor, int* items)
{
	const int stride = (int)(gridDim.x * blockDim.x);
	for (int base = (int)(blockIdx.x * blockDim.x); base < nContacts; base += stride)
	{
		const int k = base + (int)threadIdx.x;
		int slotA, slotB;
		bool touching;
		bcContactSlots(ids, flags, nContacts, slot, nBodies, k, slotA, slotB, touching);
		const bool listed = touching || !touchingOnly;
		const bool a = listed && slotA >= 0, b = listed && slotB >= 0;
		const int placeA = waveRunAlloc(cursor, slotA, a);
		if (a) items[offsets[slotA] + placeA] = k;
		const int placeB = waveRunAlloc(cursor, slotB, b);
		if (b) items[offsets[slotB] + placeB] = k;
	}
}

// Contact c as `body` sees it. The normal is b2WorldManifold::Initialize's (b2d_solver.h: the same operations on the same
// transforms, DW::b_xf = (p.x, p.y, q.s, q.c)) without the points, turned to point from the other body towards this one.
__device__ __forceinline__ b2hip_body_contact bcRecord(int c, int body, const int4* ids, const float4* man0, const float4* man1,
                                                       const int4* man3, const float4* imp, const float4* b_xf, int& pointCount)
{
	const int4 id = ids[c];
	const int4 m3 = man3[c];
	const bool isB = id.w == body;
	b2hip_body_contact r;
	r.contact_index = c;
	r.other_body = isB ? id.z : id.w;
	r.fixture = isB ? id.y : id.x;
	r.other_fixture = isB ? id.x : id.y;
	V2 normal = v2(0.0f, 0.0f);
	float jn = 0.0f, jt = 0.0f;
	pointCount = m3.w;
	if (pointCount > 0)
	{
		const float4 m0 = man0[c];
		const float4 xa = b_xf[id.z], xb = b_xf[id.w];
		Xf xfA, xfB;
		xfA.p = v2(xa.x, xa.y); xfA.q.s = xa.z; xfA.q.c = xa.w;
		xfB.p = v2(xb.x, xb.y); xfB.q.s = xb.z; xfB.q.c = xb.w;
		if (m3.z == B2D_MANIFOLD_CIRCLES)
		{
			const float4 m1 = man1[c];
			normal = v2(1.0f, 0.0f);
			const V2 pointA = b2dMulXV(xfA, v2(m0.z, m0.w));
			const V2 pointB = b2dMulXV(xfB, v2(m1.x, m1.y));
			if (b2dDistanceSquared(pointA, pointB) > B2D_EPSILON * B2D_EPSILON)
			{
				normal = pointB - pointA;
				b2dNormalize(normal);
			}
		}
		else if (m3.z == B2D_MANIFOLD_FACE_A) normal = b2dMulRV(xfA.q, v2(m0.x, m0.y));
		else normal = -b2dMulRV(xfB.q, v2(m0.x, m0.y));
		if (!isB) normal = -normal;
		const float4 j = imp[c];
		jn = j.x;
		jt = j.y;
		if (pointCount > 1)
		{
			jn = jn + j.z;
			jt = jt + j.w;
		}
	}
	r.normal[0] = normal.x;
	r.normal[1] = normal.y;
	r.normal_impulse = jn;
	r.tangent_impulse = jt;
	return r;
}

// 32-byte records leave as two 16-byte stores
template <typename R>
__device__ __forceinline__ void bcStore32(R* out, const R& r)
{
	static_assert(sizeof(R) == 32, "two 16-byte stores");
	union { R r; int4 q[2]; } u;
	u.r = r;
	int4* o = (int4*)out;
	o[0] = u.q[0];
	o[1] = u.q[1];
}

// The first nItems records of the batch, a thread per record: item k belongs to the body of slot queryOwner(k).
__global__ __launch_bounds__(256) void k_bc_records(const int4* ids, const float4* man0, const float4* man1, const int4* man3,
                                                    const float4* imp, const float4* b_xf, const int* bodies, int n, const int* offsets,
                                                    const int* items, int nItems, b2hip_body_contact* out)
{
	for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < nItems; k += (int)(gridDim.x * blockDim.x))
	{
		int pointCount;
		bcStore32(out + k, bcRecord(items[k], bodies[queryOwner(offsets, n, k)], ids, man0, man1, man3, imp, b_xf, pointCount));
	}
}

__device__ __forceinline__ float bcWaveSum(float v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off); // (a + b == b + a: every lane ends with the same bits)
	return v;
}

// One wave per body over its sorted list of TOUCHING contacts (offsets / items); countAll: every contact that names it.
__global__ __launch_bounds__(256) void k_bc_totals(const int4* ids, const float4* man0, const float4* man1, const int4* man3,
                                                   const float4* imp, const float4* b_xf, const int* bodies, int n, const int* offsets,
                                                   const int* items, const int* countAll, b2hip_body_contact_total* out)
{
	const int lane = (int)(threadIdx.x & 63u);
	const int nWaves = (int)((gridDim.x * blockDim.x) >> 6);
	for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nWaves)
	{
		const int at = offsets[i], len = offsets[i + 1] - at, body = bodies[i];
		float sx = 0.0f, sy = 0.0f, sn = 0.0f, mx = -B2D_MAXFLOAT;
		int points = 0;
		for (int k = lane; k < len; k += 64)
		{
			int pointCount;
			const b2hip_body_contact r = bcRecord(items[at + k], body, ids, man0, man1, man3, imp, b_xf, pointCount);
			// the impulse on this body: jn n + jt (n.y, -n.x)
			sx = sx + (r.normal_impulse * r.normal[0] + r.tangent_impulse * r.normal[1]);
			sy = sy + (r.normal_impulse * r.normal[1] - r.tangent_impulse * r.normal[0]);
			sn = sn + r.normal_impulse;
			mx = fmaxf(mx, r.normal_impulse);
			points += pointCount;
		}
		sx = bcWaveSum(sx);
		sy = bcWaveSum(sy);
		sn = bcWaveSum(sn);
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
		points = waveSumInt(points);
		if (lane == 0)
		{
			b2hip_body_contact_total t;
			t.contacts = countAll[i];
			t.touching = len;
			t.impulse[0] = sx;
			t.impulse[1] = sy;
			t.normal_impulse = sn;
			t.max_normal_impulse = len > 0 ? mx : 0.0f;
			t.points = points;
			t.pad = 0;
			bcStore32(out + i, t);
		}
	}
}

#endif
