// b2d_kernels_fixture_batch.h - batched fixture filter, sensor, thick-shape and material sets (include/b2hip.h, block J:
// b2hip_fixture_set_filters, b2hip_fixture_set_sensors, b2hip_fixture_set_thicks, b2hip_fixture_set_materials; host side:
// b2hip_api_fixture_batch.h).
//
// The single calls push the fixture onto the host's list of edited proxies - five small blocking copies per fixture at the next
// flushEdits - and queue one or two ops for k_apply_edits (b2d_kernels_edit.h), each of which is a walk of ONE workgroup over
// the whole contact array; b2hip_fixture_set_sensor also wakes the body through the host's mirror, eight rows uploaded per body.
// A batch is a second route to the same state:
//   k_fixture_words      one lane per entry writes the proxy's filter or material words as proxyWords (b2hip_host_upload.h)
//                        composes them, the entry's place in the batch (+ 1) into `named`, a word per fixture of the world that
//                        is 0 between calls; a filter entry of an active body takes its place in the move buffer
//                        (b2Fixture::Refilter's TouchProxy), a sensor entry that changes wakes its body (b2Body::SetAwake(true))
//   k_fixture_contacts   grid-wide over the contact array, once per call, behind the final words: CF_FILTER on every live
//                        contact of a named fixture (filters); CF_SENSOR recomputed from the two proxies (sensors); and for
//                        sensors and thick shapes the contacts whose TOI candidacy no longer is what CF_TOI_CANDIDATE says are
//                        COUNTED and, as far as the room goes, listed
//   k_fixture_toi_*      b2ContactManager::RecalculateToiCandidacy for the listed contacts by one lane in the order the loop of
//                        ops would have taken: by entry, and within an entry newest contact first (slots are appended and
//                        given back by swap-back: the partition depends on it). Sorted in LDS, or by the pair update's radix
//                        sort when the list is longer than that
//   k_fixture_unname     puts the words of `named` back to 0, entry by entry
// Nothing is destroyed: no compaction, no event, no read-back.
#ifndef B2D_KERNELS_FIXTURE_BATCH_H
#define B2D_KERNELS_FIXTURE_BATCH_H

#include "b2d_kernels_collide.h"
#include "b2d_kernels_body_lifecycle.h"

enum
{
	FIXTURE_SET_FILTERS = 0,
	FIXTURE_SET_SENSORS = 1,
	FIXTURE_SET_THICKS = 2,
	FIXTURE_SET_MATERIALS = 3
};

// One entry of a batch, as the host stages it:
//   filters    x categoryBits | maskBits << 16, y the group index (low 16 bits), z its place among the batch's moves (-1: the
//              body is inactive, no move)
//   sensors /  x bit 0 the requested value, bit 1 set when it differs from the value the fixture has (else the entry is a
//   thicks     no-op); w the fixture's body
//   materials  x, y the bits of friction and restitution
typedef uint4 FixtureSetRec;

// moveBase: the moves the device has buffered (the host has just read the counter and checked that moveBase + moveTotal fits
// the buffer); the batch's moves go behind them in entry order - the order the loop's pending moves are appended in, which a
// snapshot taken before the step carries - and one lane moves the counter. No box moves, so the hash grid stays as fresh as it
// was (the loop leaves Counters::gridFresh alone too).
template <int KIND>
__global__ __launch_bounds__(256) void k_fixture_words(DW W, const int* fixtures, const FixtureSetRec* recs, int n, int moveBase, int moveTotal, int* named)
{
	DState* S = W.st;
	if (KIND == FIXTURE_SET_FILTERS && blockIdx.x == 0 && threadIdx.x == 0 && moveTotal > 0) S->c.nMoves = moveBase + moveTotal;
	for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n; i += (int)(gridDim.x * 256))
	{
		const int q = fixtures[i];
		if ((unsigned)q >= (unsigned)W.nProxies) continue; // (the host has checked the ids: in range, alive, each once)
		const FixtureSetRec r = recs[i];
		if (KIND == FIXTURE_SET_MATERIALS)
		{
			W.p_mat[q] = make_float2(__uint_as_float(r.x), __uint_as_float(r.y));
			continue;
		}
		if (KIND == FIXTURE_SET_FILTERS)
		{
			W.p_filter0[q] = r.x;
			W.p_filter1[q] = (W.p_filter1[q] & ~0xffff) | (int)(r.y & 0xffffu);
			named[q] = i + 1;
			const int at = (int)r.z;
			if (at < 0) continue;
			if (at < moveTotal && moveBase + at < W.capMoves) W.moveBuf[moveBase + at] = q;
			else atomicOr(&S->c.overflow, 8);
			continue;
		}
		if ((r.x & 2u) == 0u) continue;
		const int bit = KIND == FIXTURE_SET_SENSORS ? PF_SENSOR : PF_THICK;
		const int f1 = W.p_filter1[q];
		W.p_filter1[q] = (r.x & 1u) ? (f1 | bit) : (f1 & ~bit);
		named[q] = i + 1;
		if (KIND != FIXTURE_SET_SENSORS) continue;
		// b2Fixture::SetSensor wakes the body (b2Fixture.cpp:249): what the upload of the host's row leaves - the low seven
		// bits of the flags word with the awake bit set, the sleep time zero; setAwake's early return for a static body that
		// is awake kept. (Two entries of one body write the same words.)
		const int body = (int)r.w;
		if ((unsigned)body >= (unsigned)W.nBodies) continue;
		const uint32_t flags = W.b_flags[body];
		if ((flags & BF_TYPE_MASK) == BT_STATIC && (flags & BF_AWAKE) != 0u) continue;
		W.b_flags[body] = (flags & 0x7fu) | BF_AWAKE;
		W.b_pos[body].w = 0.0f;
	}
}

__global__ __launch_bounds__(256) void k_fixture_unname(const int* fixtures, int n, int nProxies, int* named)
{
	for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n; i += (int)(gridDim.x * 256))
	{
		const int q = fixtures[i];
		if ((unsigned)q < (unsigned)nProxies) named[q] = 0;
	}
}

// The hot path: one pass over the contact array for the whole batch, 256 lanes, full waves. A live contact belongs to the entry
// r = the lower of its two proxies' places in the batch (in the loop the later op finds nothing left to change). It reads the
// flags (4 B), the ids (16 B) and two words of `named`; for a contact of a named fixture also the two filter words and the two
// bodies' flags.
//   filters   b2Fixture::Refilter (b2Fixture.cpp:187-210): CF_FILTER.
//   sensors   EDIT_SENSOR_FIXTURE: CF_SENSOR from the two proxies' PF_SENSOR; then as thick shapes.
//   thicks    EDIT_RECALC_FIXTURE: every op of the loop sees the FINAL proxy words (flushEdits precedes applyEditOps), so the
//             candidacy is a function of what this pass reads and not of the order. A contact whose candidacy differs from
//             CF_TOI_CANDIDATE is counted, and listed as (r << 32) | (nContacts - 1 - i) while the list has room: ascending keys
//             are the order the loop recalculates them in. The pass changes nothing the listing reads - CF_SENSOR is written
//             from the proxies alone - so it can run again with more room when the count says the list was short.
template <int KIND>
__global__ __launch_bounds__(256) void k_fixture_contacts(DW W, const int* named, unsigned long long* toiKeys, int toiRoom, int* toiCount)
{
	DState* S = W.st;
	const ContactArrays& C = W.ca[S->cur];
	const int n = S->c.nContacts;
	for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n; i += (int)(gridDim.x * 256))
	{
		uint32_t flags = C.flags[i];
		if (flags & CF_DESTROY) continue;
		const int4 ids = C.ids[i];
		if ((unsigned)ids.x >= (unsigned)W.nProxies || (unsigned)ids.y >= (unsigned)W.nProxies) continue;
		const unsigned ra = (unsigned)named[ids.x] - 1u, rb = (unsigned)named[ids.y] - 1u; // (not named: 0xffffffff)
		const unsigned r = ra < rb ? ra : rb;
		if (r == 0xffffffffu) continue;
		if (KIND == FIXTURE_SET_FILTERS)
		{
			C.flags[i] = flags | CF_FILTER;
			continue;
		}
		if ((unsigned)ids.z >= (unsigned)W.nBodies || (unsigned)ids.w >= (unsigned)W.nBodies) continue;
		if (KIND == FIXTURE_SET_SENSORS)
		{
			const bool sensor = ((W.p_filter1[ids.x] | W.p_filter1[ids.y]) & PF_SENSOR) != 0;
			const uint32_t now = (flags & ~CF_SENSOR) | (sensor ? CF_SENSOR : 0u);
			if (now != flags) C.flags[i] = now;
			flags = now;
		}
		const bool cand = isToiCandidate(W, ids.x, ids.y, ids.z, ids.w);
		if (cand == ((flags & CF_TOI_CANDIDATE) != 0u)) continue;
		const int at = atomicAdd(toiCount, 1);
		if (at < toiRoom) toiKeys[at] = ((unsigned long long)r << 32) | (unsigned)(n - 1 - i);
	}
}

// b2ContactManager::RecalculateToiCandidacy (:590-640) for the listed contacts in the order of their keys, by one lane: what
// lines 147 to 181 of b2d_kernels_edit.h do op after op - the flag toggled, the TOI state cleared, the cached time of impact
// reset, a slot appended or given back by swap-back; adds and removals interleave in list order. (A sound partition meets none
// of the guards: nothing is indexed past the arrays - toiPos2c holds capContacts slots.)
__device__ inline void fixtureToiReplay(const DW& W, const unsigned long long* keys, int count)
{
	DState* S = W.st;
	const ContactArrays& C = W.ca[S->cur];
	const int n = S->c.nContacts;
	int nToi = S->c.nToiOrder;
	for (int k = 0; k < count; ++k)
	{
		const int i = n - 1 - (int)(unsigned)(keys[k] & 0xffffffffull);
		if ((unsigned)i >= (unsigned)n) continue;
		const int4 ids = C.ids[i];
		const uint32_t flags = C.flags[i];
		const bool cand = isToiCandidate(W, ids.x, ids.y, ids.z, ids.w);
		if (cand == ((flags & CF_TOI_CANDIDATE) != 0u)) continue;
		if (cand)
		{
			if (nToi < 0 || nToi >= W.capContacts) continue;
			C.mgr[i] = nToi;
			W.toiPos2c[nToi] = i;
			++nToi;
		}
		else
		{
			const int slot = C.mgr[i];
			if (slot < 0 || nToi <= 0) continue;
			const int last = nToi - 1;
			const int moved = W.toiPos2c[last];
			if (slot > last || (unsigned)moved >= (unsigned)n) continue;
			W.toiPos2c[slot] = moved;
			C.mgr[moved] = slot;
			C.mgr[i] = -1;
			nToi = last;
		}
		C.flags[i] = (flags ^ CF_TOI_CANDIDATE) & ~CF_TOI_STATE_MASK;
		float4 mat = C.mat[i];
		mat.w = 1.0f;
		C.mat[i] = mat;
	}
	S->c.nToiOrder = nToi;
}

// The list while it fits LDS: sorted by one workgroup, then the replay. (A longer list: the host sorts it with the pair
// update's radix sort and launches k_fixture_toi_replay.)
__global__ __launch_bounds__(1024) void k_fixture_toi_sort_replay(DW W, const unsigned long long* keys, const int* toiCount)
{
	__shared__ unsigned long long s_keys[LIFECYCLE_SORT_MAX];
	const int count = *toiCount;
	if (count <= 0 || count > LIFECYCLE_SORT_MAX) return; // (uniform)
	lifecycleSortInLds(s_keys, keys, count);
	if (threadIdx.x == 0) fixtureToiReplay(W, s_keys, count);
}

__global__ void k_fixture_toi_replay(DW W, const unsigned long long* sortedKeys, const int* toiCount, int toiRoom)
{
	const int count = *toiCount;
	if (threadIdx.x == 0 && blockIdx.x == 0) fixtureToiReplay(W, sortedKeys, count < toiRoom ? count : toiRoom);
}

#endif
