// b2d_kernels_body_writes.h - batched body writes and the gather of body-state rows (include/b2hip.h: b2hip_apply_forces,
// b2hip_apply_impulses, b2hip_set_velocities, b2hip_get_body_states_of; host side: b2hip_api_body_writes.h).
//
// A batch names n bodies, each at most once in a write call (the host has checked the ids), so a lane owns the rows of its
// body: plain loads and stores, no atomics, the same bytes run after run. A lane does for its entry what the single-body
// call of include/b2hip.h does on the host's mirror - the same float32 expressions in the same order, and both sides are
// built with -ffp-contract=off - and writes what that call's upload would write: b_force or b_vel (the fourth word is 0 in
// either), and on a wake-up b_flags and the sleep time in b_pos[].w (as k_apply_edits wakes a body, b2d_kernels_edit.h).
// These are gather / scatter kernels over 16-byte rows; the grid-stride loop covers a batch of 2^24 with gridFor's 2 048
// workgroups.
#ifndef B2D_KERNELS_BODY_WRITES_H
#define B2D_KERNELS_BODY_WRITES_H

#include "b2d_world.h"

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
