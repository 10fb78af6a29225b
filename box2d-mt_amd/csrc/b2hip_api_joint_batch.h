// b2hip_api_joint_batch.h - batched joint motor targets between steps, and the states of a batch of joints
// (include/b2hip.h, block G; kernels: b2d_kernels_joint_batch.h).
//
// b2hip_joint_set_motors has the effect of b2hip_joint_set_motor made for its entries in order. It goes round that call's cost -
// one upload per edited joint at the next flushEdits, and setAwake -> markDirty -> pullBody on both bodies, whose eight rows
// each are uploaded too - by storing the motor members and waking the bodies in one launch. The host keeps two things right:
//   w->joints[id]     the three motor members follow the batch: they are what "the current value" is judged against, here and
//                     in b2hip_joint_set_motor, and b2hip_joint_set_limits uploads them again with its own members.
//   the woken bodies  are newer on the device than in h_state and the HostBody rows: bodyWritesMirror marks them not pulled
//                     and the rows pending, as behind a batched body write (b2hip_api_body_writes.h). Nothing is fetched.
// An entry that changes nothing is dropped on the host: only the entries that change travel, and a call without one launches
// nothing. b2hip_get_joint_states reads: pending edits are uploaded first (a joint created since the last step included), the
// records come back through the pinned buffer.

extern "C++"
{
// the ids of a joint batch, on the host: each in [0, joint count); a write call also refuses a destroyed joint, one without a
// motor and an id that occurs again. The first offender is named.
static int jointBatchIds(b2hip_world* w, const char* what, int n, const int32_t* joints, bool write)
{
	const size_t nj = w->joints.size();
	if (write)
	{
		if (w->jbSeen.size() < nj) w->jbSeen.resize(nj, 0u);
		if (++w->jbEpoch == 0u)
		{
			std::fill(w->jbSeen.begin(), w->jbSeen.end(), 0u);
			w->jbEpoch = 1u;
		}
	}
	for (int i = 0; i < n; ++i)
	{
		const int32_t j = joints[i];
		const char* why = nullptr;
		if (j < 0 || (size_t)j >= nj) why = ", outside [0, b2hip_joint_count)";
		else if (write)
		{
			const int type = w->joints[(size_t)j].type;
			if (type == B2D_JOINT_DEAD) why = ", which is destroyed";
			else if (!jointHasMotor(type)) why = ", whose type has no motor";
			else if (w->jbSeen[(size_t)j] == w->jbEpoch) why = " a second time";
			else w->jbSeen[(size_t)j] = w->jbEpoch;
		}
		if (why) return setError(B2HIP_ERR_INVALID, std::string(what) + ": entry " + std::to_string(i) + " names joint " + std::to_string(j) + why);
	}
	return 0;
}
} // extern "C++"

int b2hip_joint_count(const b2hip_world* w)
{
	return w ? (int)w->joints.size() : 0;
}

int b2hip_joint_is_destroyed(const b2hip_world* w, int joint)
{
	return w && joint >= 0 && joint < (int)w->joints.size() && w->joints[joint].type == B2D_JOINT_DEAD ? 1 : 0;
}

int b2hip_joint_set_motors(b2hip_world* w, int n, const int32_t* joints, const b2hip_joint_motor* motors, int mask)
{
	const char* what = "b2hip_joint_set_motors";
	if (int rc = bodyWritesArgs(what, n, joints, motors, what)) return rc; // (a write call has no output: any non-null pointer)
	if (mask < 1 || mask > 7) return setError(B2HIP_ERR_INVALID, std::string(what) + ": mask must lie in 1..7");
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = jointBatchIds(w, what, n, joints, true)) return rc;
	// the entries that change their joint (b2hip_joint_set_motor's comparison), and the bodies they wake
	std::vector<int4> edits;
	std::vector<int32_t> woken;
	for (int i = 0; i < n; ++i)
	{
		const JointRec& j = w->joints[(size_t)joints[i]];
		const int enable = (mask & JOINT_MOTOR_ENABLE) ? (motors[i].enable_motor != 0) : (j.enableMotor != 0);
		const float speed = (mask & JOINT_MOTOR_SPEED) ? motors[i].motor_speed : j.motorSpeed;
		const float maxMotor = (mask & JOINT_MOTOR_MAX) ? motors[i].max_motor : j.maxMotorTorque;
		if (enable == (j.enableMotor != 0) && speed == j.motorSpeed && maxMotor == j.maxMotorTorque) continue;
		int4 e;
		e.x = joints[i];
		e.y = enable;
		memcpy(&e.z, &speed, sizeof(float));
		memcpy(&e.w, &maxMotor, sizeof(float));
		edits.push_back(e);
		woken.push_back(j.bodyA);
		woken.push_back(j.bodyB);
	}
	if (edits.empty()) return B2HIP_OK;
	const int m = (int)edits.size();
	if (int rc = bodyWritesBegin(w, 0, nullptr, edits.data(), (size_t)m * sizeof(int4), 0)) return rc;
	LAUNCH(w, k_joint_set_motors, gridFor((size_t)m), 256, (const int4*)w->bwIn.p, m, w->d_joints.p, (int)w->upJoints, w->dw.nBodies, w->b_flags.p,
	       w->b_pos.p);
	for (int k = 0; k < m; ++k)
	{
		JointRec& j = w->joints[(size_t)edits[(size_t)k].x];
		j.enableMotor = edits[(size_t)k].y;
		memcpy(&j.motorSpeed, &edits[(size_t)k].z, sizeof(float));
		memcpy(&j.maxMotorTorque, &edits[(size_t)k].w, sizeof(float));
	}
	return bodyWritesMirror(w, (int)woken.size(), woken.data(), BODY_FORCES_NONE);
}

int b2hip_get_joint_states(b2hip_world* w, int n, const int32_t* joints, float inv_dt, b2hip_joint_state* out)
{
	const char* what = "b2hip_get_joint_states";
	if (int rc = bodyWritesArgs(what, n, joints, joints, out)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = jointBatchIds(w, what, n, joints, false)) return rc;
	if (n == 0) return B2HIP_OK;
	int rc = bodyWritesBegin(w, n, joints, nullptr, 0, (size_t)n * sizeof(b2hip_joint_state));
	if (!rc) rc = w->jbOut.ensure(3 * (size_t)n, w->stream, false, false);
	if (rc) return rc;
	LAUNCH(w, k_joint_states, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, inv_dt, (const JointRec*)w->d_joints.p, (int)w->upJoints,
	       (const GearRec*)w->d_gears.p, (int)w->upGears, w->dw.nBodies, (const float4*)w->b_xf.p, (const float4*)w->b_pos.p,
	       (const float4*)w->b_vel.p, (const float4*)w->b_mass.p, w->jbOut.p);
	return bodyContactsOut(w, (const b2hip_joint_state*)w->jbOut.p, n, out);
}
