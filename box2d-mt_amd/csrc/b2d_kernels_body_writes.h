// b2d_kernels_body_writes.h - batched body writes and the gather of body-state rows (include/b2hip.h: b2hip_apply_forces,
// b2hip_apply_impulses, b2hip_set_velocities, b2hip_get_body_states_of; host side: b2hip_api_body_writes.h).
//
// A batch names n bodies, each at most once in a write call (the host has checked the ids), so a lane owns the rows of its
// body: plain loads and stores, no atomics, the same bytes run after run. A lane does for its entry what the single-body
// call of include/b2hip.h does on the host's mirror - the same float32 expressions in the same order, and both sides are
// built with -ffp-contract=off - and writes what that call's upload would write: b_force or b_vel (the fourth word is 0 in
// either), and on a wake-up b_flags and the sleep time in b_pos[].w (as k_apply_edits wakes a body, b2d_kernels_edit.h).
// These are gather / scatter kernels over 16-byte rows; the grid-stride loop covers a batch of 2^24 with gridFor's 2 048
// workgroups. b2hip_set_awakes and b2hip_set_transforms (block H) follow the same rules; the latter also walks the proxies
// of its body and owns their fat AABBs for the same reason.
#ifndef B2D_KERNELS_BODY_WRITES_H
#define B2D_KERNELS_BODY_WRITES_H

#include "b2d_world.h"
#include "b2d_kernels_broadphase.h"

#define BODY_WRITE_FORCES 0
#define BODY_WRITE_IMPULSES 1
#define BODY_WRITE_VELOCITIES 2

// One b2hip_body_push as two 16-byte loads.
struct BodyPush
{
	float4 a; // x, y, angular, at_point (an int32)
	float4 b; // px, py, pad, pad
};

// FAMILY forces / impulses: `in` is n BodyPush, `arg` the call's wake; velocities: `in` is n x (vx, vy, omega), `arg` the mask.
template <int FAMILY>
__global__ __launch_bounds__(256) void k_body_write(const int* bodies, int n, const void* in, int arg, int nBodies, uint32_t* b_flags,
                                                    float4* b_pos, const float4* b_mass, float4* b_vel, float4* b_force)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int body = bodies[i];
		if ((unsigned)body >= (unsigned)nBodies) continue; // (the host has checked the ids: in range, each once)
		uint32_t flags = b_flags[body];
		const uint32_t type = flags & BF_TYPE_MASK;
		if (FAMILY == BODY_WRITE_VELOCITIES)
		{
			// b2hip_set_velocity: not on a static body; a non-zero velocity wakes (and restarts the sleep timer of) the body
			if (type == BT_STATIC) continue;
			const float* v3 = (const float*)in + 3 * (size_t)i;
			const float4 old = b_vel[body];
			const float vx = (arg & 1) ? v3[0] : old.x, vy = (arg & 1) ? v3[1] : old.y, omega = (arg & 2) ? v3[2] : old.z;
			if (vx * vx + vy * vy > 0.0f || omega * omega > 0.0f)
			{
				if ((flags & BF_AWAKE) == 0u) b_flags[body] = flags | BF_AWAKE;
				b_pos[body].w = 0.0f;
			}
			b_vel[body] = make_float4(vx, vy, omega, 0.0f);
			continue;
		}
		// b2hip_apply_force / b2hip_apply_*_impulse: dynamic bodies only; a sleeping body is woken or left alone
		if (type != BT_DYNAMIC) continue;
		if ((flags & BF_AWAKE) == 0u)
		{
			if (!arg) continue;
			flags |= BF_AWAKE;
			b_flags[body] = flags;
			b_pos[body].w = 0.0f;
		}
		const BodyPush p = ((const BodyPush*)in)[i];
		const float x = p.a.x, y = p.a.y, angular = p.a.z;
		const bool atPoint = __float_as_int(p.a.w) != 0;
		const float4 c = b_pos[body];
		if (FAMILY == BODY_WRITE_FORCES)
		{
			const float torque = atPoint ? angular + ((p.b.x - c.x) * y - (p.b.y - c.y) * x) : angular;
			const float4 f = b_force[body];
			b_force[body] = make_float4(f.x + x, f.y + y, f.z + torque, 0.0f);
		}
		else
		{
			const float4 m = b_mass[body]; // invMass, invI
			float4 v = b_vel[body];
			const float sx = m.x * x, sy = m.x * y;
			v.x += sx;
			v.y += sy;
			if (atPoint) v.z += m.y * ((p.b.x - c.x) * y - (p.b.y - c.y) * x);
			v.z += m.y * angular; // (b2hip_apply_angular_impulse, always made: a zero still does its +=)
			b_vel[body] = make_float4(v.x, v.y, v.z, 0.0f);
		}
	}
}

// b2hip_set_awakes: awake[i] == 0 is b2hip_set_awake(w, body, 0) - the flag cleared, the sleep time, the velocity row and the
// force row zeroed, on any body type; anything else is b2Body::SetAwake(true) - the flag set and the sleep time zeroed, a
// static body that is awake already left untouched (setAwake, b2hip_host_world.h).
__global__ __launch_bounds__(256) void k_set_awakes(const int* bodies, int n, const uint8_t* awake, int nBodies, uint32_t* b_flags, float4* b_pos,
                                                    float4* b_vel, float4* b_force)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int body = bodies[i];
		if ((unsigned)body >= (unsigned)nBodies) continue; // (the host has checked the ids: in range, each once)
		const uint32_t flags = b_flags[body];
		if (awake[i] != 0)
		{
			if ((flags & BF_TYPE_MASK) == BT_STATIC && (flags & BF_AWAKE) != 0u) continue;
			if ((flags & BF_AWAKE) == 0u) b_flags[body] = flags | BF_AWAKE;
			b_pos[body].w = 0.0f;
			continue;
		}
		if ((flags & BF_AWAKE) != 0u) b_flags[body] = flags & ~BF_AWAKE;
		b_pos[body].w = 0.0f;
		b_vel[body] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		b_force[body] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	}
}

// b2hip_set_transforms: one lane per entry does what b2hip_set_transform does on the host's mirror and what the next upload
// would write - b_xf, b_pos (the sleep time kept), b_pos0 (the sweep origin moves with the body, b2Body.cpp:463-467) - and then
// b2Fixture::Synchronize(xf, xf) for every proxy of the body, newest first (b_proxyHead / p_next): b2DynamicTree::MoveProxy
// with zero displacement. A proxy whose fat AABB still contains its box is left alone; one that left it gets the box grown by
// B2D_AABB_EXTENSION and a place in the move buffer. The moved proxies of a workgroup are collected in LDS and take their
// places with ONE atomic on the counter, as in k_sync_fixtures (the order of the move buffer has no meaning: the pairs are
// sorted); a body with more proxies than the list has room for - a container, a chain of edges - walks them all on its one lane
// and takes the places past the list's end one by one. The host has checked that every proxy of the batch fits in the move
// buffer; the guard of k_sync_fixtures is kept all the same. pose3: n x (x, y, angle); mask bit 0: position, bit 1: angle.
#define XF_MOVES_TILE 1024
__global__ __launch_bounds__(256) void k_set_transforms(DW W, const int* bodies, int n, const float* pose3, int mask)
{
	DState* S = W.st;
	const int tid = (int)threadIdx.x;
	__shared__ int s_list[XF_MOVES_TILE];
	__shared__ int s_cnt, s_base;
	for (int base = (int)(blockIdx.x * 256); base < n; base += (int)(gridDim.x * 256))
	{
		if (tid == 0) s_cnt = 0;
		__syncthreads();
		const int i = base + tid;
		const int body = i < n ? bodies[i] : -1;
		if ((unsigned)body < (unsigned)W.nBodies) // (the host has checked the ids: in range, each once)
		{
			const float4 t = W.b_xf[body], pos = W.b_pos[body], m = W.b_mass[body];
			const float* p = pose3 + 3 * (size_t)i;
			const float x = (mask & 1) ? p[0] : t.x, y = (mask & 1) ? p[1] : t.y, a = (mask & 2) ? p[2] : pos.z;
			Xf xf;
			xf.p = v2(x, y);
			xf.q = b2dRot(a);
			const V2 c = b2dMulXV(xf, v2(m.z, m.w));
			W.b_xf[body] = make_float4(x, y, xf.q.s, xf.q.c);
			W.b_pos[body] = make_float4(c.x, c.y, a, pos.w);
			W.b_pos0[body] = make_float4(c.x, c.y, a, 0.0f);
			// (the walks of b2d_kernels_spatial.h and b2d_kernels_toi.h trust the list and only read; this one writes p_fat and
			// moveBuf behind it, so a broken link ends the walk rather than index past the proxy tables. A sound list meets
			// neither bound.)
			int walked = 0;
			for (int q = W.b_proxyHead[body]; q >= 0 && q < W.nProxies && walked < W.nProxies; q = W.p_next[q], ++walked)
			{
				const AABB aabb = b2dShapeAABB(W.shapes + W.p_shape[q], xf);
				if (b2dAabbContains(loadAabb(W.p_fat, q), aabb)) continue;
				W.p_fat[q] = make_float4(aabb.lo.x - B2D_AABB_EXTENSION, aabb.lo.y - B2D_AABB_EXTENSION, aabb.hi.x + B2D_AABB_EXTENSION,
				                         aabb.hi.y + B2D_AABB_EXTENSION);
				const int k = atomicAdd(&s_cnt, 1);
				if (k < XF_MOVES_TILE) { s_list[k] = q; continue; }
				const int at = atomicAdd(&S->c.nMoves, 1);
				if (at < W.capMoves) W.moveBuf[at] = q;
				else atomicOr(&S->c.overflow, 8);
			}
		}
		__syncthreads();
		const int cnt = s_cnt < XF_MOVES_TILE ? s_cnt : XF_MOVES_TILE;
		if (tid == 0 && cnt > 0)
		{
			s_base = atomicAdd(&S->c.nMoves, cnt);
			S->c.gridFresh = 0; // (boxes moved: whatever grid there is is stale until the next pair update)
		}
		__syncthreads();
		if (cnt > 0)
		{
			const int at = s_base;
			for (int k = tid; k < cnt; k += 256)
			{
				if (at + k < W.capMoves) W.moveBuf[at + k] = s_list[k];
				else atomicOr(&S->c.overflow, 8);
			}
		}
		__syncthreads();
	}
}

// rows[i] = the b2hip_body_state of bodies[i], the ten words as k_end_step lays them out (b2d_kernels_broadphase.h). A read:
// an id may occur more than once.
__global__ __launch_bounds__(256) void k_body_rows(const int* bodies, int n, int nBodies, const uint32_t* b_flags, const float4* b_pos,
                                                   const float4* b_vel, const float4* b_xf, float2* rows)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int body = bodies[i];
		float2* o = rows + 5 * (size_t)i; // (40 bytes a row: 8-byte aligned)
		if ((unsigned)body >= (unsigned)nBodies)
		{
			for (int c = 0; c < 5; ++c) o[c] = make_float2(0.0f, 0.0f);
			continue;
		}
		const float4 xf = b_xf[body], p = b_pos[body], v = b_vel[body];
		const uint32_t f = b_flags[body];
		o[0] = make_float2(xf.x, xf.y);
		o[1] = make_float2(p.z, v.x);
		o[2] = make_float2(v.y, v.z);
		o[3] = make_float2(p.x, p.y);
		o[4] = make_float2(__uint_as_float(f & 0x7fu), p.w);
	}
}

#endif
