// b2d_kernels_body_lifecycle.h - batched body destruction and activation sets (include/b2hip.h, block I: b2hip_destroy_bodies,
// b2hip_set_actives; host side: b2hip_api_body_lifecycle.h).
//
// The single calls go through the host's mirror - eight rows per body and five small copies per fixture uploaded by the next
// flushEdits - and queue one EDIT_DESTROY_BODY op each, which k_apply_edits (b2d_kernels_edit.h) works off with ONE workgroup
// that scans the whole contact array once per op. A batch is a second route to the same state:
//   k_lifecycle_rows           one lane per named body writes what that upload would leave in the body's rows, and the body's
//                              place in the batch (+ 1) into `named`, a word per body of the world that is 0 between calls
//   k_lifecycle_proxies        one lane per fixture record: owner and proxy id, and for an activated proxy the fat AABB at the
//                              body's transform and a place in the move buffer (the expressions of k_set_transforms)
//   k_destroy_contacts_of_set  grid-wide over the contact array: every live contact with a named body is destroyed as the op of
//                              its FIRST named body would destroy it (a contact between two named bodies belongs to the earlier
//                              entry: the later op finds it gone)
//   k_lifecycle_toi_*          the slots of the TOI partition are given back by one lane in the order the loop of ops would
//                              have taken: by entry, and within an entry newest contact first (RemoveFromContactArray's
//                              swap-back depends on it). The contact pass lists (entry, index) of the contacts that hold a slot;
//                              the list is sorted in LDS, or by the pair update's radix sort when it is longer than that
//   k_lifecycle_unname         puts the words of `named` back to 0, entry by entry (a batch names few of a world's bodies:
//                              n words written, against a memset of one word per body of the world per call)
// k_edit_keepflags, the scan, k_compact_contacts and k_edit_finish follow as behind k_apply_edits.
#ifndef B2D_KERNELS_BODY_LIFECYCLE_H
#define B2D_KERNELS_BODY_LIFECYCLE_H

#include "b2d_kernels_body_writes.h"

#define LIFECYCLE_NONE 0       // the entry has the requested state already: it takes no part
#define LIFECYCLE_DESTROY 1
#define LIFECYCLE_DEACTIVATE 2
#define LIFECYCLE_ACTIVATE 3
#define LIFECYCLE_SORT_MAX 4096 // list entries the one-workgroup sort holds in LDS (32 KB)

// A fixture of a named body: x fixture id, y the proxy id it has from now on, z what to do (LIFECYCLE_*), w its body.
typedef int4 LifecycleProxy;

// The flags word: uploadDirtyBodies writes it whole from the host's copy, of which pullBody refreshes the low seven bits and
// which never holds a higher one - so the looped route ends with the device's low seven bits, edited, and nothing above them.
// destroy: type static, not active, not awake, no bullet; velocity and force rows zero; invMass and invI zero, the local
// centre kept (b2hip_destroy_body). deactivate / activate: the active bit.
__global__ __launch_bounds__(256) void k_lifecycle_rows(const int* bodies, const int* ops, int n, int nBodies, uint32_t* b_flags, float4* b_vel,
                                                        float4* b_force, float4* b_mass, int* named)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int body = bodies[i], op = ops[i];
		if ((unsigned)body >= (unsigned)nBodies || op == LIFECYCLE_NONE) continue; // (the host has checked the ids: in range, each once)
		const uint32_t flags = b_flags[body] & 0x7fu;
		if (op == LIFECYCLE_ACTIVATE)
		{
			b_flags[body] = flags | BF_ACTIVE;
			continue;
		}
		named[body] = i + 1;
		if (op == LIFECYCLE_DEACTIVATE)
		{
			b_flags[body] = flags & ~BF_ACTIVE;
			continue;
		}
		b_flags[body] = flags & ~(BF_TYPE_MASK | BF_ACTIVE | BF_AWAKE | BF_BULLET);
		b_vel[body] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		b_force[body] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		const float4 m = b_mass[body];
		b_mass[body] = make_float4(0.0f, 0.0f, m.z, m.w);
	}
}

__global__ __launch_bounds__(256) void k_lifecycle_unname(const int* bodies, int n, int nBodies, int* named)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int body = bodies[i];
		if ((unsigned)body < (unsigned)nBodies) named[body] = 0;
	}
}

// destroy / deactivate: the proxy has no owner any more (proxyWords, b2hip_host_upload.h); the filter and material words stay.
// activate: b2Fixture::CreateProxies - owner, a fresh proxy id, the shape's AABB at the body's transform grown by
// B2D_AABB_EXTENSION, one buffered move. A lane makes at most one move, so a workgroup's moves fit its list of 256 and take
// their places with ONE atomic on the counter; the host has checked that they fit the buffer, the guard is kept all the same.
__global__ __launch_bounds__(256) void k_lifecycle_proxies(DW W, const LifecycleProxy* recs, int n)
{
	DState* S = W.st;
	const int tid = (int)threadIdx.x;
	__shared__ int s_list[256];
	__shared__ int s_cnt, s_base;
	for (int base = (int)(blockIdx.x * 256); base < n; base += (int)(gridDim.x * 256))
	{
		if (tid == 0) s_cnt = 0;
		__syncthreads();
		const int i = base + tid;
		if (i < n)
		{
			const LifecycleProxy r = recs[i];
			const int q = r.x;
			if ((unsigned)q < (unsigned)W.nProxies && (unsigned)r.w < (unsigned)W.nBodies)
			{
				W.p_key[q] = r.y;
				if (r.z == LIFECYCLE_ACTIVATE)
				{
					W.p_body[q] = r.w;
					const float4 t = W.b_xf[r.w];
					Xf xf;
					xf.p = v2(t.x, t.y);
					xf.q.s = t.z;
					xf.q.c = t.w;
					const AABB aabb = b2dShapeAABB(W.shapes + W.p_shape[q], xf);
					W.p_fat[q] = make_float4(aabb.lo.x - B2D_AABB_EXTENSION, aabb.lo.y - B2D_AABB_EXTENSION, aabb.hi.x + B2D_AABB_EXTENSION,
					                         aabb.hi.y + B2D_AABB_EXTENSION);
					s_list[atomicAdd(&s_cnt, 1)] = q;
				}
				else W.p_body[q] = -1;
			}
		}
		__syncthreads();
		const int cnt = s_cnt;
		if (tid == 0 && cnt > 0)
		{
			s_base = atomicAdd(&S->c.nMoves, cnt);
			S->c.gridFresh = 0; // (boxes appeared: whatever grid there is is stale until the next pair update)
		}
		__syncthreads();
		if (tid < cnt)
		{
			if (s_base + tid < W.capMoves) W.moveBuf[s_base + tid] = s_list[tid];
			else atomicOr(&S->c.overflow, 8);
		}
		__syncthreads();
	}
}

// The hot path: one pass over the contact array for the whole batch, 256 lanes, full waves. For a live contact the entry it
// belongs to is r = the lower of its two bodies' places in the batch; with one it gets the order-independent part of
// k_apply_edits' destroy branch, word for word - the end event of a reported contact, the wake of both bodies when the manifold
// has points and the contact is no sensor (b2Contact::Destroy), CF_DESTROY. The census of destroyed contacts costs one atomic
// per workgroup (a returning atomic per contact on one word serialises the grid on it). A contact that holds a slot of the TOI
// partition is listed as (r << 32) | (nContacts - 1 - i): ascending keys are the order the loop of ops removes them in.
// toiCap 0: a world without TOI candidates has no list.
__global__ __launch_bounds__(256) void k_destroy_contacts_of_set(DW W, const int* named, unsigned long long* toiKeys, int toiCap, int* toiCount)
{
	DState* S = W.st;
	const ContactArrays& C = W.ca[S->cur];
	const int n = S->c.nContacts;
	__shared__ int s_destroyed;
	if (threadIdx.x == 0) s_destroyed = 0;
	__syncthreads();
	int mine = 0;
	for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n; i += (int)(gridDim.x * 256))
	{
		const uint32_t flags = C.flags[i];
		if (flags & CF_DESTROY) continue;
		const int4 ids = C.ids[i];
		if ((unsigned)ids.z >= (unsigned)W.nBodies || (unsigned)ids.w >= (unsigned)W.nBodies) continue;
		const unsigned ra = (unsigned)named[ids.z] - 1u, rb = (unsigned)named[ids.w] - 1u; // (not named: 0xffffffff)
		const unsigned r = ra < rb ? ra : rb;
		if (r == 0xffffffffu) continue;
		if (W.eventsOn && (flags & CF_REPORTED))
		{
			// b2ContactManager::Destroy (:104-107): a touching contact ends when it is destroyed
			const int e = atomicAdd(&S->c.nEvents, 1);
			if (e < W.capContacts)
			{
				W.evKey[e] = C.key[i];
				W.evInfo[e] = make_int4(ids.x, ids.y, 1, -1);
			}
		}
		// b2Contact::Destroy (b2Contact.cpp:100-113): wake both bodies if the manifold had points
		if (C.man3[i].w > 0 && (flags & CF_SENSOR) == 0)
		{
			atomicOr(&W.b_flags[ids.z], BF_AWAKE);
			atomicOr(&W.b_flags[ids.w], BF_AWAKE);
			W.b_pos[ids.z].w = 0.0f;
			W.b_pos[ids.w].w = 0.0f;
		}
		C.flags[i] = flags | CF_DESTROY;
		mine += 1;
		if (toiCap > 0 && C.mgr[i] >= 0)
		{
			const int at = atomicAdd(toiCount, 1);
			if (at < toiCap) toiKeys[at] = ((unsigned long long)r << 32) | (unsigned)(n - 1 - i);
		}
	}
	for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
	if ((threadIdx.x & 63) == 0 && mine > 0) atomicAdd(&s_destroyed, mine);
	__syncthreads();
	if (threadIdx.x == 0 && s_destroyed > 0) atomicAdd(&S->c.nDestroy, s_destroyed);
}

// b2ContactManager::RemoveFromContactArray (:688-714) for the listed contacts in the order of their keys, by one lane: what
// lines 126 to 143 of b2d_kernels_edit.h do op after op.
__device__ inline void lifecycleToiReplay(const DW& W, const unsigned long long* keys, int count)
{
	DState* S = W.st;
	const ContactArrays& C = W.ca[S->cur];
	const int n = S->c.nContacts;
	int nToi = S->c.nToiOrder;
	for (int k = 0; k < count; ++k)
	{
		const int i = n - 1 - (int)(unsigned)(keys[k] & 0xffffffffull);
		if ((unsigned)i >= (unsigned)n) continue;
		const int slot = C.mgr[i];
		if (slot < 0 || nToi <= 0) continue;
		const int last = nToi - 1;
		const int moved = W.toiPos2c[last];
		if (slot > last || (unsigned)moved >= (unsigned)n) continue; // (a sound partition meets neither: nothing is indexed past the arrays)
		W.toiPos2c[slot] = moved;
		C.mgr[moved] = slot;
		C.mgr[i] = -1;
		nToi = last;
	}
	S->c.nToiOrder = nToi;
}

// `count` keys (0 < count <= LIFECYCLE_SORT_MAX, uniform) into s_keys, ascending: a bitonic sort by one workgroup of 1024.
// (The batched fixture sets, b2d_kernels_fixture_batch.h, sort their list with it too.)
__device__ inline void lifecycleSortInLds(unsigned long long* s_keys, const unsigned long long* keys, int count)
{
	const int t = (int)threadIdx.x;
	int room = 64;
	while (room < count) room <<= 1;
	for (int k = t; k < room; k += 1024) s_keys[k] = k < count ? keys[k] : ~0ull;
	__syncthreads();
	for (int size = 2; size <= room; size <<= 1)
	{
		for (int stride = size >> 1; stride > 0; stride >>= 1)
		{
			for (int k = t; k < room; k += 1024)
			{
				const int other = k ^ stride;
				if (other > k)
				{
					const unsigned long long a = s_keys[k], b = s_keys[other];
					const bool up = (k & size) == 0;
					if ((a > b) == up) { s_keys[k] = b; s_keys[other] = a; }
				}
			}
			__syncthreads();
		}
	}
}

// The list while it fits LDS: sorted by one workgroup, then the replay. (A longer list: the host sorts it with the pair
// update's radix sort and launches k_lifecycle_toi_replay.)
__global__ __launch_bounds__(1024) void k_lifecycle_toi_sort_replay(DW W, unsigned long long* keys, const int* toiCount)
{
	__shared__ unsigned long long s_keys[LIFECYCLE_SORT_MAX];
	const int count = *toiCount;
	if (count <= 0 || count > LIFECYCLE_SORT_MAX) return; // (uniform)
	lifecycleSortInLds(s_keys, keys, count);
	if (threadIdx.x == 0) lifecycleToiReplay(W, s_keys, count);
}

__global__ void k_lifecycle_toi_replay(DW W, const unsigned long long* sortedKeys, const int* toiCount, int toiCap)
{
	const int count = *toiCount;
	if (threadIdx.x == 0 && blockIdx.x == 0) lifecycleToiReplay(W, sortedKeys, count < toiCap ? count : toiCap);
}

#endif
