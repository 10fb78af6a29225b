// b2d_kernels_body_props.h - batched body property sets (include/b2hip.h, block K: b2hip_set_types, b2hip_set_bullets,
// b2hip_set_fixed_rotations, b2hip_set_sleeping_alloweds, b2hip_set_body_dampings, b2hip_set_mass_datas,
// b2hip_reset_mass_datas; host side: b2hip_api_body_props.h).
//
// The single calls go through the host's mirror - eight rows per body uploaded by the next flushEdits - and b2hip_set_type /
// b2hip_set_bullet queue one op each for k_apply_edits (b2d_kernels_edit.h), a walk of ONE workgroup over the whole contact
// array per body. A batch is a second route to the same state:
//   k_body_dampings        one lane per entry writes the masked components of the body's damping row
//   k_body_flag_sets       one lane per entry edits BF_AUTOSLEEP (and wakes a body that may no longer sleep) or BF_BULLET (and
//                          writes the entry's place in the batch (+ 1) into `named`, the word per body of block I)
//   k_body_bullet_contacts grid-wide over the contact array, once per call, behind the final flags: what k_fixture_contacts does
//                          for thick shapes, for bodies - the contacts whose TOI candidacy no longer is what CF_TOI_CANDIDATE
//                          says are COUNTED and, as far as the room goes, listed; block J's sort and replay follow
//   k_body_mass_rows       one lane per entry does the device's half of b2Body::ResetMassData / SetMassData / SetFixedRotation /
//                          SetType: the host has computed the mass data (the fixtures and densities are its own), the lane moves
//                          the centre, corrects the velocity, rewrites the mass row and the sweep origin, edits the flags
//   k_body_refit_count     b2hip_set_types: how many proxies of the bodies that turn static have left their fat AABB (the host
//                          expects none, and runs the single calls if there is one)
//   k_body_prop_moves      b2hip_set_types: the proxies of the changing bodies into the move buffer, at the places the host gave
// A lane owns the rows of its body (the host has checked the ids: in range, alive, each once): plain loads and stores. The
// flags word is written as uploadDirtyBodies writes it - the low seven bits, edited, and nothing above them (k_lifecycle_rows).
#ifndef B2D_KERNELS_BODY_PROPS_H
#define B2D_KERNELS_BODY_PROPS_H

#include "b2d_kernels_fixture_batch.h"
#include "b2d_wave.h"

#define BODY_PROP_SLEEPING 0
#define BODY_PROP_BULLETS 1

// What k_body_mass_rows does for an entry (BodyMassRec::op).
#define BODY_MASS_PART 0x1u      // the entry takes part (else it has the requested state already)
#define BODY_MASS_UPLOADS 0x2u   // the single call uploads the body's rows even though it changes nothing: the flags word loses
                                 // what lies above its low seven bits
#define BODY_MASS_ZERO_SPIN 0x4u // b2Body::SetFixedRotation: the angular velocity is zeroed first
#define BODY_MASS_FIXED_ON 0x8u
#define BODY_MASS_FIXED_OFF 0x10u
#define BODY_MASS_ORIGIN 0x20u   // ResetMassData of a static or kinematic body: the centre is the origin, the velocity stays
#define BODY_MASS_TYPE 0x40u     // b2Body::SetType: the type of bits 8 and 9, awake, sleep time and force row zero, named
#define BODY_MASS_STATIC 0x80u   // ... to static: the velocity row zero
#define BODY_MASS_TYPE_SHIFT 8

// One entry as the host stages it: the mass row (invMass, invI, the local centre) and what to do.
struct BodyMassRec
{
	float invMass, invI, lcx, lcy;
	uint32_t op, pad0, pad1, pad2;
};

// b2hip_set_body_damping with the components outside `mask` (B2HIP_DAMPING_*) kept: the row as the upload writes it.
__global__ __launch_bounds__(256) void k_body_dampings(const int* bodies, int n, const float4* recs, int mask, int nBodies, float4* b_damp, uint32_t* b_flags)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int body = bodies[i];
		if ((unsigned)body >= (unsigned)nBodies) continue; // (the host has checked the ids: in range, each once)
		const float4 r = recs[i], old = b_damp[body];
		b_damp[body] = make_float4((mask & 1) ? r.x : old.x, (mask & 2) ? r.y : old.y, (mask & 4) ? r.z : old.z, 0.0f);
		const uint32_t flags = b_flags[body];
		if (flags & ~0x7fu) b_flags[body] = flags & 0x7fu;
	}
}

// value[i]: bit 0 the requested flag; bullets: bit 1 set when it differs from the flag the body has (else the entry takes no
// part in the contact pass).
//   sleeping  b2Body::SetSleepingAllowed (b2Body.h:674-688): false also wakes the body - the awake bit set and the sleep time
//             zeroed whether or not it slept.
//   bullets   b2Body::SetBullet: the bit, and the name for k_body_bullet_contacts.
template <int KIND>
__global__ __launch_bounds__(256) void k_body_flag_sets(const int* bodies, int n, const uint8_t* value, int nBodies, uint32_t* b_flags, float4* b_pos, int* named)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int body = bodies[i];
		if ((unsigned)body >= (unsigned)nBodies) continue; // (the host has checked the ids: in range, each once)
		const uint32_t v = value[i];
		uint32_t flags = b_flags[body] & 0x7fu;
		if (KIND == BODY_PROP_SLEEPING)
		{
			if (v & 1u) flags |= BF_AUTOSLEEP;
			else
			{
				flags = (flags & ~BF_AUTOSLEEP) | BF_AWAKE;
				b_pos[body].w = 0.0f;
			}
		}
		else
		{
			flags = (v & 1u) ? (flags | BF_BULLET) : (flags & ~BF_BULLET);
			if (v & 2u) named[body] = i + 1;
		}
		b_flags[body] = flags;
	}
}

// The hot path of b2hip_set_bullets: one pass over the contact array for the whole batch, 256 lanes, full waves. A live contact
// of a named body belongs to the entry r = the lower of its two bodies' places in the batch (in the loop the later op finds
// nothing left to change). It reads the flags (4 B), the ids (16 B) and two words of `named`; for a contact of a named body also
// the two proxies' words and the two bodies' flags (isToiCandidate). Every op of the loop sees the FINAL flags of all bodies
// (flushEdits precedes applyEditOps), so the candidacy is a function of what this pass reads and not of the order. A contact
// whose candidacy differs from CF_TOI_CANDIDATE is counted, and listed as (r << 32) | (nContacts - 1 - i) while the list has
// room: ascending keys are the order the loop recalculates them in. The pass changes nothing, so it can run again with more room
// when the count says the list was short. Places in the list are taken once per workgroup and trip (blockAlloc): a bullet batch
// over 10^4 bodies lists 10^5 contacts, and a returning atomic per contact on one word serialises the grid on it; where an entry
// lands does not matter - the list is sorted by key afterwards.
__global__ __launch_bounds__(256) void k_body_bullet_contacts(DW W, const int* named, unsigned long long* toiKeys, int toiRoom, int* toiCount)
{
	DState* S = W.st;
	const ContactArrays& C = W.ca[S->cur];
	const int n = S->c.nContacts;
	for (int base = (int)(blockIdx.x * 256); base < n; base += (int)(gridDim.x * 256)) // (uniform per workgroup: blockAlloc has barriers)
	{
		const int i = base + (int)threadIdx.x;
		bool list = false;
		unsigned r = 0xffffffffu;
		if (i < n)
		{
			const uint32_t flags = C.flags[i];
			const int4 ids = C.ids[i];
			if ((flags & CF_DESTROY) == 0u && (unsigned)ids.x < (unsigned)W.nProxies && (unsigned)ids.y < (unsigned)W.nProxies &&
			    (unsigned)ids.z < (unsigned)W.nBodies && (unsigned)ids.w < (unsigned)W.nBodies)
			{
				const unsigned ra = (unsigned)named[ids.z] - 1u, rb = (unsigned)named[ids.w] - 1u; // (not named: 0xffffffff)
				r = ra < rb ? ra : rb;
				if (r != 0xffffffffu) list = isToiCandidate(W, ids.x, ids.y, ids.z, ids.w) != ((flags & CF_TOI_CANDIDATE) != 0u);
			}
		}
		const int at = blockAlloc(toiCount, list);
		if (list && at < toiRoom) toiKeys[at] = ((unsigned long long)r << 32) | (unsigned)(n - 1 - i);
	}
}

// The device's half of b2Body::ResetMassData (b2Body.cpp:310-385), SetMassData (:387-424), SetFixedRotation (:546-565) and
// SetType (:116-175), with the expressions of k_set_transforms - bit-equal to the host's b2dMulXV (both sides are built with
// -ffp-contract=off, and b2dRot of the angle is the host's sinf / cosf):
//   oldC = c; c = xf * localCentre; v += cross(w, c - oldC)     (a static or kinematic body: c = the origin, v untouched)
// The mass row is rewritten, and the sweep origin as the single route leaves it: pullBody sets a0 = a, c0 = c, the call moves c0
// with c, and the upload writes (c0, a0) because the call asked for it (HostBody::resetSweep).
__global__ __launch_bounds__(256) void k_body_mass_rows(DW W, const int* bodies, const BodyMassRec* recs, int n, int* named)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int body = bodies[i];
		if ((unsigned)body >= (unsigned)W.nBodies) continue; // (the host has checked the ids: in range, each once)
		const float4 m = ((const float4*)recs)[2 * (size_t)i];
		const uint32_t op = ((const uint4*)recs)[2 * (size_t)i + 1].x;
		if ((op & (BODY_MASS_PART | BODY_MASS_UPLOADS)) == 0u) continue;
		uint32_t flags = W.b_flags[body] & 0x7fu;
		if ((op & BODY_MASS_PART) == 0u)
		{
			W.b_flags[body] = flags;
			continue;
		}
		const float4 t = W.b_xf[body], pos = W.b_pos[body];
		float4 v = W.b_vel[body];
		if (op & BODY_MASS_ZERO_SPIN) v.z = 0.0f;
		if (op & BODY_MASS_FIXED_ON) flags |= BF_FIXEDROT;
		if (op & BODY_MASS_FIXED_OFF) flags &= ~BF_FIXEDROT;
		V2 c = v2(t.x, t.y);
		if ((op & BODY_MASS_ORIGIN) == 0u)
		{
			Xf xf;
			xf.p = v2(t.x, t.y);
			xf.q = b2dRot(pos.z);
			c = b2dMulXV(xf, v2(m.z, m.w));
			const V2 dv = b2dCrossSV(v.z, c - v2(pos.x, pos.y));
			v.x += dv.x;
			v.y += dv.y;
		}
		float sleepTime = pos.w;
		if (op & BODY_MASS_TYPE)
		{
			flags = (flags & ~BF_TYPE_MASK) | ((op >> BODY_MASS_TYPE_SHIFT) & BF_TYPE_MASK) | BF_AWAKE;
			sleepTime = 0.0f;
			W.b_force[body] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			named[body] = i + 1;
		}
		if (op & BODY_MASS_STATIC) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		W.b_mass[body] = make_float4(m.x, m.y, m.z, m.w);
		W.b_pos[body] = make_float4(c.x, c.y, pos.z, sleepTime);
		W.b_pos0[body] = make_float4(c.x, c.y, pos.z, 0.0f);
		W.b_vel[body] = make_float4(v.x, v.y, v.z, 0.0f);
		W.b_flags[body] = flags;
	}
}

// b2Body::SynchronizeFixtures with xf1 == xf for a body that turns static: b2DynamicTree::MoveProxy with zero displacement moves
// a proxy only if its fat AABB no longer holds the shape's (refitProxy, b2hip_api_bodies.h). Counts those, one atomic per wave
// that has any.
__global__ __launch_bounds__(256) void k_body_refit_count(DW W, const int* proxies, int n, int* count)
{
	for (int base = (int)(blockIdx.x * 256); base < n; base += (int)(gridDim.x * 256))
	{
		const int i = base + (int)threadIdx.x;
		bool left = false;
		if (i < n)
		{
			const int q = proxies[i];
			const int body = (unsigned)q < (unsigned)W.nProxies ? W.p_body[q] : -1;
			if ((unsigned)body < (unsigned)W.nBodies)
			{
				const float4 t = W.b_xf[body];
				Xf xf;
				xf.p = v2(t.x, t.y);
				xf.q = b2dRot(W.b_pos[body].z);
				left = !b2dAabbContains(loadAabb(W.p_fat, q), b2dShapeAABB(W.shapes + W.p_shape[q], xf));
			}
		}
		const unsigned long long mask = __ballot(left);
		if (mask != 0ull && waveLane() == 0) atomicAdd(count, __popcll(mask));
	}
}

// b2BroadPhase::TouchProxy for every proxy of a body whose type changes: recs[k] = (proxy, its place among the batch's moves).
// moveBase: the moves the device has buffered (the host has just read the counter and checked that moveBase + moveTotal fits the
// buffer); the batch's go behind them in the order the loop's pending moves are appended in, and one lane moves the counter. No
// box moves, so the hash grid stays as fresh as it was (k_fixture_words).
__global__ __launch_bounds__(256) void k_body_prop_moves(DW W, const int2* recs, int n, int moveBase, int moveTotal)
{
	DState* S = W.st;
	if (blockIdx.x == 0 && threadIdx.x == 0 && moveTotal > 0) S->c.nMoves = moveBase + moveTotal;
	for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n; i += (int)(gridDim.x * 256))
	{
		const int2 r = recs[i];
		if ((unsigned)r.x >= (unsigned)W.nProxies) continue;
		if (r.y >= 0 && r.y < moveTotal && moveBase + r.y < W.capMoves) W.moveBuf[moveBase + r.y] = r.x;
		else atomicOr(&S->c.overflow, 8);
	}
}

#endif
