// b2d_kernels_joint_batch.h - batched joint motor targets and the gather of joint states (include/b2hip.h, block G:
// b2hip_joint_set_motors, b2hip_get_joint_states; host side: b2hip_api_joint_batch.h).
//
// k_joint_set_motors: the host sends the entries that CHANGE their joint, each joint at most once, so a lane owns the three
// motor members of its record. The bodies it wakes it may share with other lanes (a chain, a chassis with two wheels): every
// lane that wakes a body stores the same two values - the flags it read with the awake bit set, a zero sleep time - and no
// other bit of either row changes in this kernel, so the result does not depend on which lane comes first.
// k_joint_states: a lane reads its JointRec through the pointer (the record is 196 bytes and 4-byte aligned: dword loads,
// and only of the members its type uses - nothing is copied to registers whole) and the four rows of its two bodies
// (16-byte loads), and stores one 48-byte record as three 16-byte stores. The float32 expressions are those of the drop-in
// classes' getters (host/src/b2_world.cpp) in their order; both sides are built with -ffp-contract=off.
// Both are grid-stride gather / scatter kernels: gridFor's 2 048 workgroups cover a batch of 2^24.
#ifndef B2D_KERNELS_JOINT_BATCH_H
#define B2D_KERNELS_JOINT_BATCH_H

#include "b2d_world.h"
#include "b2d_joint.h"

#define JOINT_MOTOR_ENABLE 1
#define JOINT_MOTOR_SPEED 2
#define JOINT_MOTOR_MAX 4

// b2Body::SetAwake(true) as setAwake makes it on the host (b2hip_host_world.h): not on a static body that is awake already
__device__ __forceinline__ void jointBatchWake(int body, int nBodies, uint32_t* b_flags, float4* b_pos)
{
	if ((unsigned)body >= (unsigned)nBodies) return;
	const uint32_t flags = b_flags[body];
	if ((flags & BF_TYPE_MASK) == BT_STATIC && (flags & BF_AWAKE) != 0u) return;
	if ((flags & BF_AWAKE) == 0u) b_flags[body] = flags | BF_AWAKE;
	b_pos[body].w = 0.0f;
}

// edits[i] = (joint, enableMotor as 0 / 1, motorSpeed, maxMotorTorque): the changed entries of the call
__global__ __launch_bounds__(256) void k_joint_set_motors(const int4* edits, int n, JointRec* joints, int nJoints, int nBodies,
                                                          uint32_t* b_flags, float4* b_pos)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int4 e = edits[i];
		if ((unsigned)e.x >= (unsigned)nJoints) continue; // (the host has checked the ids: in range, alive, each once)
		JointRec* j = joints + e.x;
		j->enableMotor = e.y;
		j->motorSpeed = __int_as_float(e.z);
		j->maxMotorTorque = __int_as_float(e.w);
		jointBatchWake(j->bodyA, nBodies, b_flags, b_pos);
		jointBatchWake(j->bodyB, nBodies, b_flags, b_pos);
	}
}

// The four rows of a body a joint getter reads.
struct JointBody
{
	V2 p; Rot q;    // b_xf: the origin's transform
	V2 c; float a;  // b_pos: world centre, angle
	V2 v; float w;  // b_vel
	V2 lc;          // b_mass: local centre
};

__device__ __forceinline__ JointBody jointBatchBody(int body, int nBodies, const float4* b_xf, const float4* b_pos, const float4* b_vel,
                                                    const float4* b_mass)
{
	JointBody r;
	memset(&r, 0, sizeof(r));
	if ((unsigned)body >= (unsigned)nBodies) return r;
	const float4 xf = b_xf[body], p = b_pos[body], v = b_vel[body], m = b_mass[body];
	r.p = v2(xf.x, xf.y); r.q.s = xf.z; r.q.c = xf.w;
	r.c = v2(p.x, p.y); r.a = p.z;
	r.v = v2(v.x, v.y); r.w = v.z;
	r.lc = v2(m.z, m.w);
	return r;
}

// b2Body::GetWorldPoint: b2Mul(xf, local)
__device__ __forceinline__ V2 jointBatchWorldPoint(const JointBody& b, V2 local)
{
	return v2((b.q.c * local.x - b.q.s * local.y) + b.p.x, (b.q.s * local.x + b.q.c * local.y) + b.p.y);
}

// b2PrismaticJoint::GetJointTranslation / b2WheelJoint::GetJointTranslation
__device__ __forceinline__ float jointBatchTranslation(const JointBody& A, const JointBody& B, V2 anchorA, V2 anchorB, V2 localAxisA)
{
	const V2 d = jointBatchWorldPoint(B, anchorB) - jointBatchWorldPoint(A, anchorA);
	return b2dDot(d, b2dMulRV(A.q, localAxisA));
}

// b2PrismaticJoint::GetJointSpeed / b2WheelJoint::GetJointLinearSpeed
__device__ __forceinline__ float jointBatchLinearSpeed(const JointBody& A, const JointBody& B, V2 anchorA, V2 anchorB, V2 localAxisA)
{
	const V2 rA = b2dMulRV(A.q, anchorA - A.lc);
	const V2 rB = b2dMulRV(B.q, anchorB - B.lc);
	const V2 d = (B.c + rB) - (A.c + rA);
	const V2 axis = b2dMulRV(A.q, localAxisA);
	return b2dDot(d, b2dCrossSV(A.w, axis)) + b2dDot(axis, B.v + b2dCrossSV(B.w, rB) - A.v - b2dCrossSV(A.w, rA));
}

// out[3 * i ..] = the b2hip_joint_state of ids[i]: (type, limit_state, coordinate, speed) (coordinate2, speed2, force.x,
// force.y) (torque, motor, 0, 0). A read: an id may occur more than once.
__global__ __launch_bounds__(256) void k_joint_states(const int* ids, int n, float inv_dt, const JointRec* joints, int nJoints,
                                                      const GearRec* gears, int nGears, int nBodies, const float4* b_xf, const float4* b_pos,
                                                      const float4* b_vel, const float4* b_mass, float4* out)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int id = ids[i];
		float4* o = out + 3 * (size_t)i;
		const JointRec* j = joints + id;
		const int type = (unsigned)id < (unsigned)nJoints ? j->type : B2D_JOINT_DEAD; // (the host has checked the ids)
		if (type == B2D_JOINT_DEAD)
		{
			o[0] = make_float4(__int_as_float(B2D_JOINT_DEAD), 0.0f, 0.0f, 0.0f);
			o[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			o[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			continue;
		}
		const GearRec* gear = nullptr;
		if (type == B2D_JOINT_GEAR && (unsigned)j->enableLimit < (unsigned)nGears) gear = gears + j->enableLimit;
		const JointReaction r = b2dJointReaction(j, gear, inv_dt);
		float coordinate = 0.0f, speed = 0.0f, coordinate2 = 0.0f, speed2 = 0.0f;
		if (type == B2D_JOINT_REVOLUTE || type == B2D_JOINT_PRISMATIC || type == B2D_JOINT_WHEEL || type == B2D_JOINT_PULLEY)
		{
			const JointBody A = jointBatchBody(j->bodyA, nBodies, b_xf, b_pos, b_vel, b_mass);
			const JointBody B = jointBatchBody(j->bodyB, nBodies, b_xf, b_pos, b_vel, b_mass);
			if (type == B2D_JOINT_REVOLUTE)
			{
				coordinate = B.a - A.a - j->referenceAngle;
				speed = B.w - A.w;
			}
			else if (type == B2D_JOINT_PULLEY)
			{
				// (the ground anchors: A in localAxisA, B in s1, s2)
				coordinate = b2dLength(jointBatchWorldPoint(A, j->localAnchorA) - j->groundAnchorA);
				coordinate2 = b2dLength(jointBatchWorldPoint(B, j->localAnchorB) - v2(j->s1, j->s2));
			}
			else
			{
				coordinate = jointBatchTranslation(A, B, j->localAnchorA, j->localAnchorB, j->localAxisA);
				speed = jointBatchLinearSpeed(A, B, j->localAnchorA, j->localAnchorB, j->localAxisA);
				if (type == B2D_JOINT_WHEEL)
				{
					coordinate2 = B.a - A.a;
					speed2 = B.w - A.w;
				}
			}
		}
		o[0] = make_float4(__int_as_float(type), __int_as_float(j->limitState), coordinate, speed);
		o[1] = make_float4(coordinate2, speed2, r.force.x, r.force.y);
		o[2] = make_float4(r.torque, r.motor, 0.0f, 0.0f);
	}
}

#endif
