// b2hip_api_joints.h - part of the ONE translation unit b2hip.hip, inside its extern "C" block: the joints of the C ABI of
// include/b2hip.h - the eleven creators, b2hip_destroy_joint, every single-joint setter and getter (the batched ones:
// b2hip_api_joint_batch.h).
// (No include guard on purpose: b2hip.hip includes it exactly once, in order - the fragments share one scope.)

static int addJoint(b2hip_world* w, const JointRec& j)
{
	if (int rcu = checkUsable(w, "b2hip_create_joint", true)) return rcu;
	w->joints.push_back(j);
	if (w->spatial) w->spOwnersDirty = true; // (a joint may join bodies of different owners: resolved at the next step)
	// b2World::CreateJoint (b2World.cpp:716-732): contacts between the two bodies are re-filtered
	if (j.collideConnected == 0) w->pendingFilter.push_back(std::make_pair(j.bodyA, j.bodyB));
	return (int)w->joints.size() - 1;
}

extern "C++"
{
// What every creator of a joint between two bodies starts with: the arguments are there, the body ids are in range (the
// world's state is addJoint's to check, behind them), and the record is zero but for its type, bodies and collideConnected.
template <typename Def>
static int jointFromDef(b2hip_world* w, const Def* def, int type, JointRec* j)
{
	if (!w || !def) return setError(B2HIP_ERR_INVALID, "null argument");
	const int nb = (int)w->bodies.size();
	if (def->body_a < 0 || def->body_a >= nb || def->body_b < 0 || def->body_b >= nb) return setError(B2HIP_ERR_INVALID, "bad body id");
	memset(j, 0, sizeof(*j));
	j->type = type;
	j->bodyA = def->body_a;
	j->bodyB = def->body_b;
	j->collideConnected = def->collide_connected;
	return 0;
}

// ... and the two local anchors of the types that have both
template <typename Def>
static void anchorsFromDef(const Def* def, JointRec* j)
{
	j->localAnchorA = v2(def->local_anchor_a[0], def->local_anchor_a[1]);
	j->localAnchorB = v2(def->local_anchor_b[0], def->local_anchor_b[1]);
}
} // extern "C++"

int b2hip_create_revolute_joint(b2hip_world* w, const b2hip_revolute_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_REVOLUTE, &j)) return rc;
	anchorsFromDef(def, &j);
	j.referenceAngle = def->reference_angle;
	j.enableLimit = def->enable_limit;
	j.lowerAngle = def->lower_angle;
	j.upperAngle = def->upper_angle;
	j.enableMotor = def->enable_motor;
	j.motorSpeed = def->motor_speed;
	j.maxMotorTorque = def->max_motor_torque;
	return addJoint(w, j);
}

int b2hip_create_distance_joint(b2hip_world* w, const b2hip_distance_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_DISTANCE, &j)) return rc;
	anchorsFromDef(def, &j);
	j.length = def->length;
	j.frequencyHz = def->frequency_hz;
	j.dampingRatio = def->damping_ratio;
	return addJoint(w, j);
}

int b2hip_create_prismatic_joint(b2hip_world* w, const b2hip_prismatic_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_PRISMATIC, &j)) return rc;
	anchorsFromDef(def, &j);
	j.localAxisA = v2(def->local_axis_a[0], def->local_axis_a[1]);
	b2dNormalize(j.localAxisA); // b2PrismaticJoint.cpp:104
	j.referenceAngle = def->reference_angle;
	j.enableLimit = def->enable_limit;
	j.lowerTranslation = def->lower_translation;
	j.upperTranslation = def->upper_translation;
	j.enableMotor = def->enable_motor;
	j.motorSpeed = def->motor_speed;
	j.maxMotorForce = def->max_motor_force;
	return addJoint(w, j);
}

int b2hip_create_weld_joint(b2hip_world* w, const b2hip_weld_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_WELD, &j)) return rc;
	anchorsFromDef(def, &j);
	j.referenceAngle = def->reference_angle;
	j.frequencyHz = def->frequency_hz;
	j.dampingRatio = def->damping_ratio;
	return addJoint(w, j);
}

int b2hip_create_wheel_joint(b2hip_world* w, const b2hip_wheel_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_WHEEL, &j)) return rc;
	anchorsFromDef(def, &j);
	j.localAxisA = v2(def->local_axis_a[0], def->local_axis_a[1]);
	j.frequencyHz = def->frequency_hz;
	j.dampingRatio = def->damping_ratio;
	j.enableMotor = def->enable_motor;
	j.motorSpeed = def->motor_speed;
	j.maxMotorTorque = def->max_motor_torque;
	return addJoint(w, j);
}

int b2hip_create_rope_joint(b2hip_world* w, const b2hip_rope_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_ROPE, &j)) return rc;
	anchorsFromDef(def, &j);
	j.maxLength = def->max_length;
	return addJoint(w, j);
}

int b2hip_create_friction_joint(b2hip_world* w, const b2hip_friction_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_FRICTION, &j)) return rc;
	anchorsFromDef(def, &j);
	j.maxForce = def->max_force;
	j.maxTorque = def->max_torque;
	return addJoint(w, j);
}

int b2hip_create_motor_joint(b2hip_world* w, const b2hip_motor_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_MOTOR, &j)) return rc;
	j.linearOffset = v2(def->linear_offset[0], def->linear_offset[1]);
	j.angularOffset = def->angular_offset;
	j.maxForce = def->max_force;
	j.maxTorque = def->max_torque;
	j.correctionFactor = def->correction_factor;
	return addJoint(w, j);
}

int b2hip_create_pulley_joint(b2hip_world* w, const b2hip_pulley_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_PULLEY, &j)) return rc;
	if (def->ratio == 0.0f) return setError(B2HIP_ERR_INVALID, "pulley ratio must not be zero");
	anchorsFromDef(def, &j);
	j.groundAnchorA = v2(def->ground_anchor_a[0], def->ground_anchor_a[1]);
	j.s1 = def->ground_anchor_b[0];
	j.s2 = def->ground_anchor_b[1];
	j.ratio = def->ratio;
	j.constant = def->length_a + def->ratio * def->length_b; // b2PulleyJoint.cpp:75
	return addJoint(w, j);
}

int b2hip_create_mouse_joint(b2hip_world* w, const b2hip_mouse_joint_def* def)
{
	JointRec j;
	if (int rc = jointFromDef(w, def, B2D_JOINT_MOUSE, &j)) return rc;
	HostBody& bB = w->bodies[def->body_b];
	if (!bB.dirty) pullBody(w, def->body_b); // current transform of bodyB
	j.targetA = v2(def->target[0], def->target[1]);
	// m_localAnchorB = b2MulT(bodyB transform, target) (b2MouseJoint.cpp:45)
	const float px = def->target[0] - bB.px, py = def->target[1] - bB.py;
	j.localAnchorB = v2(bB.qc * px + bB.qs * py, -bB.qs * px + bB.qc * py);
	j.bodyMass = bB.mass;
	j.maxForce = def->max_force;
	j.frequencyHz = def->frequency_hz;
	j.dampingRatio = def->damping_ratio;
	w->nMouseJoints += 1;
	return addJoint(w, j);
}

// b2GearJoint::b2GearJoint (b2GearJoint.cpp:50-129): everything is derived from the two joints and the bodies' current poses
static float gearCoordinate(b2hip_world* w, const JointRec& jt, int moving, int fixed)
{
	const HostBody& bm = w->bodies[moving];
	const HostBody& bf = w->bodies[fixed];
	if (jt.type == B2D_JOINT_REVOLUTE) return bm.a - bf.a - jt.referenceAngle;
	// pA = b2MulT(xfC.q, b2Mul(xfA.q, m_localAnchorA) + (xfA.p - xfC.p)); coordinate = b2Dot(pA - pC, m_localAxisC)
	const V2 la = jt.localAnchorB, lc = jt.localAnchorA;
	const V2 wa = v2(bm.qc * la.x - bm.qs * la.y, bm.qs * la.x + bm.qc * la.y) + v2(bm.px - bf.px, bm.py - bf.py);
	const V2 pa = v2(bf.qc * wa.x + bf.qs * wa.y, -bf.qs * wa.x + bf.qc * wa.y);
	return b2dDot(pa - lc, jt.localAxisA);
}

// (a gear couples two joints, not two bodies of its definition: its checks are its own)
int b2hip_create_gear_joint(b2hip_world* w, const b2hip_gear_joint_def* def)
{
	if (!w || !def) return setError(B2HIP_ERR_INVALID, "null argument");
	const int nj = (int)w->joints.size();
	if (def->joint1 < 0 || def->joint1 >= nj || def->joint2 < 0 || def->joint2 >= nj) return setError(B2HIP_ERR_INVALID, "bad joint id");
	const JointRec j1 = w->joints[def->joint1], j2 = w->joints[def->joint2];
	if ((j1.type != B2D_JOINT_REVOLUTE && j1.type != B2D_JOINT_PRISMATIC) || (j2.type != B2D_JOINT_REVOLUTE && j2.type != B2D_JOINT_PRISMATIC))
		return setError(B2HIP_ERR_INVALID, "a gear joint connects revolute and / or prismatic joints");
	const int ids[4] = { j1.bodyB, j2.bodyB, j1.bodyA, j2.bodyA }; // A, B, C, D
	for (int k = 0; k < 4; ++k)
		if (!w->bodies[ids[k]].dirty) pullBody(w, ids[k]);
	GearRec g;
	memset(&g, 0, sizeof(g));
	g.bodyC = ids[2];
	g.bodyD = ids[3];
	g.typeA = j1.type;
	g.typeB = j2.type;
	g.localAnchorC = j1.localAnchorA; g.localAnchorA = j1.localAnchorB; g.referenceAngleA = j1.referenceAngle;
	g.localAxisC = j1.type == B2D_JOINT_PRISMATIC ? j1.localAxisA : v2(0.0f, 0.0f);
	g.localAnchorD = j2.localAnchorA; g.localAnchorB = j2.localAnchorB; g.referenceAngleB = j2.referenceAngle;
	g.localAxisD = j2.type == B2D_JOINT_PRISMATIC ? j2.localAxisA : v2(0.0f, 0.0f);
	const float coordinateA = gearCoordinate(w, j1, ids[0], ids[2]);
	const float coordinateB = gearCoordinate(w, j2, ids[1], ids[3]);
	g.ratio = def->ratio;
	g.constant = coordinateA + g.ratio * coordinateB;
	JointRec j;
	memset(&j, 0, sizeof(j));
	j.type = B2D_JOINT_GEAR;
	j.bodyA = ids[0];
	j.bodyB = ids[1];
	j.enableLimit = (int)w->gears.size();
	j.collideConnected = def->collide_connected;
	w->gears.push_back(g);
	return addJoint(w, j);
}

// b2Body::SetAwake(true) on both bodies of a joint whose definition changed (b2RevoluteJoint.cpp:418-500)
static void wakeJointBodies(b2hip_world* w, const JointRec& j)
{
	setAwake(w, j.bodyA);
	setAwake(w, j.bodyB);
}

int b2hip_destroy_joint(b2hip_world* w, int joint)
{
	// (the id before the world's state, unlike checkJoint: a null world is a "bad joint id" here)
	if (!w || joint < 0 || joint >= (int)w->joints.size()) return setError(B2HIP_ERR_INVALID, "bad joint id");
	if (int rcu = checkUsable(w, "b2hip_destroy_joint", true)) return rcu;
	JointRec& j = w->joints[joint];
	if (j.type == B2D_JOINT_DEAD) return setError(B2HIP_ERR_INVALID, "joint already destroyed");
	// (a gear joint must be destroyed before the joints it couples, as in the reference)
	wakeJointBodies(w, j);
	// contacts between the two bodies are filtered again when the joint kept them from colliding (b2World.cpp:833-845)
	if (j.collideConnected == 0) w->pendingFilter.push_back(std::make_pair(j.bodyA, j.bodyB));
	if (j.type == B2D_JOINT_MOUSE) w->nMouseJoints -= 1;
	j.type = B2D_JOINT_DEAD;
	w->jadjJoints = (size_t)-1; // per-body joint lists are rebuilt without it
	queueJointEdit(w, joint, JOINT_EDIT_DESTROY);
	return 0;
}

// What every single-joint setter and getter starts with: a usable world, then an id in range.
static int checkJoint(b2hip_world* w, const char* what, int joint)
{
	if (int rcu = checkUsable(w, what, true)) return rcu;
	if (joint < 0 || joint >= (int)w->joints.size()) return setError(B2HIP_ERR_INVALID, "bad joint id");
	return 0;
}

static bool jointHasMotor(int type) { return type == B2D_JOINT_REVOLUTE || type == B2D_JOINT_PRISMATIC || type == B2D_JOINT_WHEEL; }
static bool jointHasLimits(int type) { return type == B2D_JOINT_REVOLUTE || type == B2D_JOINT_PRISMATIC; }
static bool jointHasSpring(int type) { return type == B2D_JOINT_WHEEL || type == B2D_JOINT_DISTANCE || type == B2D_JOINT_WELD || type == B2D_JOINT_MOUSE; }

int b2hip_joint_set_target(b2hip_world* w, int joint, float x, float y)
{
	if (int rc = checkJoint(w, "b2hip_joint_set_target", joint)) return rc;
	JointRec& j = w->joints[joint];
	if (j.type != B2D_JOINT_MOUSE) return setError(B2HIP_ERR_INVALID, "not a mouse joint");
	if (x == j.targetA.x && y == j.targetA.y) return 0;
	setAwake(w, j.bodyB);
	j.targetA = v2(x, y);
	queueJointEdit(w, joint, JOINT_EDIT_ANCHORS);
	return 0;
}

int b2hip_joint_set_motor(b2hip_world* w, int joint, int enable_motor, float motor_speed, float max_motor)
{
	if (int rc = checkJoint(w, "b2hip_joint_set_motor", joint)) return rc;
	JointRec& j = w->joints[joint];
	if (!jointHasMotor(j.type)) return setError(B2HIP_ERR_INVALID, "joint type has no motor");
	if ((enable_motor != 0) == (j.enableMotor != 0) && motor_speed == j.motorSpeed && max_motor == j.maxMotorTorque) return 0;
	wakeJointBodies(w, j);
	j.enableMotor = enable_motor != 0;
	j.motorSpeed = motor_speed;
	j.maxMotorTorque = max_motor;
	queueJointEdit(w, joint, JOINT_EDIT_MEMBERS);
	return 0;
}

int b2hip_joint_set_offsets(b2hip_world* w, int joint, float linear_x, float linear_y, float angular)
{
	if (int rc = checkJoint(w, "b2hip_joint_set_offsets", joint)) return rc;
	JointRec& j = w->joints[joint];
	if (j.type != B2D_JOINT_MOTOR) return setError(B2HIP_ERR_INVALID, "not a motor joint");
	if (linear_x == j.linearOffset.x && linear_y == j.linearOffset.y && angular == j.angularOffset) return 0;
	wakeJointBodies(w, j);
	j.linearOffset = v2(linear_x, linear_y);
	j.angularOffset = angular;
	queueJointEdit(w, joint, JOINT_EDIT_ANCHORS);
	return 0;
}

int b2hip_joint_set_limits(b2hip_world* w, int joint, int enable_limit, float lower, float upper)
{
	if (int rc = checkJoint(w, "b2hip_joint_set_limits", joint)) return rc;
	JointRec& j = w->joints[joint];
	if (!jointHasLimits(j.type)) return setError(B2HIP_ERR_INVALID, "joint type has no limits");
	if (lower > upper) return setError(B2HIP_ERR_INVALID, "lower limit above upper limit");
	if ((enable_limit != 0) == (j.enableLimit != 0) && lower == j.lowerAngle && upper == j.upperAngle) return 0;
	wakeJointBodies(w, j);
	j.enableLimit = enable_limit != 0;
	j.lowerAngle = lower;
	j.upperAngle = upper;
	queueJointEdit(w, joint, JOINT_EDIT_LIMITS); // the limit impulse restarts from zero
	return 0;
}

// The scalar setters of the joint classes: plain assignments in the reference (b2DistanceJoint.h:117, b2RopeJoint.h:80,
// b2FrictionJoint.cpp:206-228, b2MotorJoint.cpp:222-251, b2MouseJoint.cpp:48-76, b2GearJoint.cpp:402-406)
int b2hip_joint_set_param(b2hip_world* w, int joint, int param, float value)
{
	if (int rc = checkJoint(w, "b2hip_joint_set_param", joint)) return rc;
	JointRec& j = w->joints[joint];
	const int t = j.type;
	int kind = JOINT_EDIT_MEMBERS;
	if (param == B2HIP_JOINT_LENGTH && (t == B2D_JOINT_DISTANCE || t == B2D_JOINT_ROPE)) { j.length = value; kind = JOINT_EDIT_ANCHORS; }
	else if (param == B2HIP_JOINT_MAX_FORCE && (t == B2D_JOINT_FRICTION || t == B2D_JOINT_MOTOR || t == B2D_JOINT_MOUSE)) j.maxForce = value;
	else if (param == B2HIP_JOINT_MAX_TORQUE && (t == B2D_JOINT_FRICTION || t == B2D_JOINT_MOTOR)) j.maxTorque = value;
	else if (param == B2HIP_JOINT_RATIO && t == B2D_JOINT_GEAR)
	{
		// (a gear's definition lives in its own record, GearRec; JointRec::enableLimit is its index there)
		const int gi = j.enableLimit;
		if (gi < 0 || gi >= (int)w->gears.size()) return setError(B2HIP_ERR_INVALID, "gear record missing");
		w->gears[(size_t)gi].ratio = value;
		if ((size_t)gi < w->upGears)
		{
			DEVICE_GUARD(w);
			HIP_TRY(hipMemcpy((char*)(w->d_gears.p + gi) + offsetof(GearRec, ratio), &value, sizeof(float), hipMemcpyHostToDevice));
		}
		return B2HIP_OK;
	}
	else if (param == B2HIP_JOINT_CORRECTION_FACTOR && t == B2D_JOINT_MOTOR) j.correctionFactor = value;
	else return setError(B2HIP_ERR_INVALID, "b2hip_joint_set_param: the joint's type has no such parameter");
	queueJointEdit(w, joint, kind);
	return B2HIP_OK;
}

int b2hip_joint_set_spring(b2hip_world* w, int joint, float frequency_hz, float damping_ratio)
{
	if (int rc = checkJoint(w, "b2hip_joint_set_spring", joint)) return rc;
	JointRec& j = w->joints[joint];
	if (!jointHasSpring(j.type)) return setError(B2HIP_ERR_INVALID, "joint type has no spring");
	j.frequencyHz = frequency_hz;
	j.dampingRatio = damping_ratio;
	queueJointEdit(w, joint, JOINT_EDIT_MEMBERS);
	return B2HIP_OK;
}

// b2RopeJoint::GetLimitState (b2RopeJoint.h:84) and the limit state of revolute / prismatic joints: the solver's, from the
// device record; 0 inactive, 1 at lower, 2 at upper, 3 equal (b2LimitState, b2Joint.h:58-64); negative: error
int b2hip_get_joint_limit_state(b2hip_world* w, int joint)
{
	if (int rc = checkJoint(w, "b2hip_get_joint_limit_state", joint)) return rc;
	DEVICE_GUARD(w);
	int state = w->joints[joint].limitState;
	if ((size_t)joint < w->upJoints && w->d_joints.p != nullptr)
	{
		HIP_TRY(hipMemcpyAsync(&state, (const char*)(w->d_joints.p + joint) + offsetof(JointRec, limitState), sizeof(int), hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
	}
	return state;
}

int b2hip_get_joint_reaction(b2hip_world* w, int joint, float inv_dt, float out4[4])
{
	if (int rc = checkJoint(w, "b2hip_get_joint_reaction", joint)) return rc;
	if (!out4) return setError(B2HIP_ERR_INVALID, "bad joint id"); // (one message for the id and the pointer, as ever)
	DEVICE_GUARD(w);
	JointRec rec = w->joints[joint];
	GearRec gear;
	memset(&gear, 0, sizeof(gear));
	const bool isGear = rec.type == B2D_JOINT_GEAR;
	// (the solver's state lives in the device copy; a joint the device has not seen yet has done nothing)
	if ((size_t)joint < w->upJoints && w->d_joints.p != nullptr)
	{
		HIP_TRY(hipMemcpyAsync(&rec, w->d_joints.p + joint, sizeof(JointRec), hipMemcpyDeviceToHost, w->stream));
		if (isGear && (size_t)rec.enableLimit < w->upGears) HIP_TRY(hipMemcpyAsync(&gear, w->d_gears.p + rec.enableLimit, sizeof(GearRec), hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
	}
	const JointReaction r = b2dJointReaction(&rec, isGear ? &gear : nullptr, inv_dt);
	out4[0] = r.force.x;
	out4[1] = r.force.y;
	out4[2] = r.torque;
	out4[3] = r.motor;
	return 0;
}
