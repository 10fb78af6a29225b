// b2hip_api_bodies.h - part of the ONE translation unit b2hip.hip, inside its extern "C" block: the bodies of the C ABI of
// include/b2hip.h - create / destroy, mass data, the single-body pushes (force, impulses, velocity) and every b2Body setter
// (the batched calls: b2hip_api_body_writes.h).
// (No include guard on purpose: b2hip.hip includes it exactly once, in order - the fragments share one scope.)

int b2hip_create_body(b2hip_world* w, const b2hip_body_def* def)
{
	if (!w || !def) return setError(B2HIP_ERR_INVALID, "null argument");
	if (int rcu = checkUsable(w, "b2hip_create_body", true)) return rcu;
	HostBody b{}; // (what is not set below starts at zero: local centre, forces, sleep time, inertia)
	b.type = def->type;
	if (def->bullet) b.flags |= BF_BULLET;
	if (def->fixed_rotation) b.flags |= BF_FIXEDROT;
	if (def->allow_sleep) b.flags |= BF_AUTOSLEEP;
	if (def->awake) b.flags |= BF_AWAKE;
	if (def->active) b.flags |= BF_ACTIVE;
	b.px = def->px;
	b.py = def->py;
	b.qs = sinf(def->angle); // b2Rot::Set (b2Math.h:294-299)
	b.qc = cosf(def->angle);
	b.c0x = b.cx = def->px;
	b.c0y = b.cy = def->py;
	b.a0 = b.a = def->angle;
	b.vx = def->vx;
	b.vy = def->vy;
	b.w = def->w;
	b.linearDamping = def->linear_damping;
	b.angularDamping = def->angular_damping;
	b.gravityScale = def->gravity_scale;
	b.pullEpoch = w->mirrorEpoch;
	b.forceEpoch = w->stepEpoch;
	b.mass = b.invMass = def->type == B2HIP_DYNAMIC_BODY ? 1.0f : 0.0f;
	b.dirty = true;
	b.worldIndex = -1;
	if (def->type != B2HIP_STATIC_BODY)
	{
		// b2World::CreateBody (b2World.cpp:571-575): appended to m_nonStaticBodies
		b.worldIndex = (int)w->nonStatic.size();
		w->nonStatic.push_back((int)w->bodies.size());
		w->orderDirty = true;
	}
	w->bodies.push_back(b);
	if (w->spatial) w->spOwnersDirty = true; // (the new body falls into the strip of its x at the next step)
	w->dirtyList.push_back((int)w->bodies.size() - 1);
	return (int)w->bodies.size() - 1;
}

int b2hip_destroy_body(b2hip_world* w, int body)
{
	if (int rc = checkBody(w, body, "b2hip_destroy_body")) return rc;
	// joints first, newest first (the body's joint list is newest first, b2World.cpp:697-710)
	for (int j = (int)w->joints.size() - 1; j >= 0; --j)
	{
		if (w->joints[j].type == B2D_JOINT_DEAD) continue;
		bool touches = w->joints[j].bodyA == body || w->joints[j].bodyB == body;
		if (w->joints[j].type == B2D_JOINT_GEAR)
		{
			const GearRec& g = w->gears[w->joints[j].enableLimit];
			touches = touches || g.bodyC == body || g.bodyD == body;
		}
		if (touches)
		{
			const int rc = b2hip_destroy_joint(w, j);
			if (rc) return rc;
		}
	}
	HostBody& b = editBody(w, body);
	queueOp(w, EDIT_DESTROY_BODY, body);
	for (int k = (int)b.fixtures.size() - 1; k >= 0; --k) dropFixture(w, b.fixtures[k]); // newest first
	b.fixtures.clear();
	if (b.worldIndex >= 0)
	{
		// b2RemoveAndSwapBack on m_nonStaticBodies (b2World.cpp:662-667)
		const int slot = b.worldIndex, last = w->nonStatic.back();
		w->nonStatic[(size_t)slot] = last;
		w->bodies[last].worldIndex = slot;
		w->nonStatic.pop_back();
		b.worldIndex = -1;
		w->orderDirty = true;
	}
	b.dead = 1;
	b.type = B2HIP_STATIC_BODY;
	b.flags &= ~(BF_ACTIVE | BF_AWAKE | BF_BULLET);
	b.vx = b.vy = b.w = 0.0f;
	b.fx = b.fy = b.torque = 0.0f;
	b.invMass = b.invI = 0.0f;
	return B2HIP_OK;
}

int b2hip_body_is_destroyed(const b2hip_world* w, int body)
{
	return w && body >= 0 && body < (int)w->bodies.size() && w->bodies[body].dead ? 1 : 0;
}

int b2hip_get_mass_data(const b2hip_world* w, int body, b2hip_mass_data* out)
{
	if (!w || !out || body < 0 || body >= (int)w->bodies.size()) return setError(B2HIP_ERR_INVALID, "bad argument");
	const HostBody& b = w->bodies[body];
	out->mass = b.mass;
	// b2Body::GetInertia (b2Body.h:585-588)
	out->inertia = b.I + b.mass * (b.lcx * b.lcx + b.lcy * b.lcy);
	out->local_center[0] = b.lcx;
	out->local_center[1] = b.lcy;
	out->inv_mass = b.invMass;
	out->inv_inertia = b.invI;
	return 0;
}

// b2Body::SetMassData (b2Body.cpp:387-424); mass_data == NULL: b2Body::ResetMassData (b2Body.cpp:310-385)
int b2hip_set_mass_data(b2hip_world* w, int body, const b2hip_mass_data* md)
{
	if (int rc = checkBody(w, body, "b2hip_set_mass_data")) return rc;
	HostBody& b = editBody(w, body);
	if (md == nullptr)
	{
		resetMassData(w, b);
		b.resetSweep = 1;
		return B2HIP_OK;
	}
	if (b.type != B2HIP_DYNAMIC_BODY) return B2HIP_OK;
	storeMass(b, massFromData(b, md));
	moveCenter(b);
	b.resetSweep = 1;
	return B2HIP_OK;
}

// What a force or an impulse starts with (b2Body.h:848-942): a sleeping body is woken if the caller asks for it, and only an
// awake body takes the push. Returns whether the body is awake.
static bool wakeIfAsked(HostBody& b, int wake)
{
	if (wake && (b.flags & BF_AWAKE) == 0)
	{
		b.flags |= BF_AWAKE;
		b.sleepTime = 0.0f;
	}
	return (b.flags & BF_AWAKE) != 0;
}

int b2hip_apply_force(b2hip_world* w, int body, float fx, float fy, float torque, int wake)
{
	if (int rcu = checkUsable(w, "b2hip_apply_force", true)) return rcu;
	if (!w || body < 0 || body >= (int)w->bodies.size()) return setError(B2HIP_ERR_INVALID, "bad argument");
	if (w->bodies[body].type != B2HIP_DYNAMIC_BODY) return 0;
	HostBody& b = editBody(w, body);
	// (a row that was already dirty - an edit from a callback of the last step - has not been through pullBody: the forces it
	// holds are the last step's, which the step cleared on the device, and its epoch must say that THIS force is new; else a
	// later pull of the same step - a PreSolve edit - takes the force for a stale one and drops it)
	if (w->def.auto_clear_forces && b.forceEpoch != w->stepEpoch) { b.fx = b.fy = b.torque = 0.0f; }
	b.forceEpoch = w->stepEpoch;
	if (wakeIfAsked(b, wake))
	{
		b.fx += fx;
		b.fy += fy;
		b.torque += torque;
	}
	return 0;
}

int b2hip_set_velocity(b2hip_world* w, int body, float vx, float vy, float omega)
{
	if (int rcu = checkUsable(w, "b2hip_set_velocity", true)) return rcu;
	if (!w || body < 0 || body >= (int)w->bodies.size()) return setError(B2HIP_ERR_INVALID, "bad argument");
	if (w->bodies[body].type == B2HIP_STATIC_BODY) return 0;
	HostBody& b = editBody(w, body);
	if (vx * vx + vy * vy > 0.0f || omega * omega > 0.0f)
	{
		b.flags |= BF_AWAKE;
		b.sleepTime = 0.0f;
	}
	b.vx = vx;
	b.vy = vy;
	b.w = omega;
	return 0;
}

int b2hip_apply_linear_impulse(b2hip_world* w, int body, float ix, float iy, float px, float py, int wake)
{
	if (int rc = checkBody(w, body, "b2hip_apply_linear_impulse")) return rc;
	if (w->bodies[body].type != B2HIP_DYNAMIC_BODY) return B2HIP_OK;
	HostBody& b = editBody(w, body);
	if (wakeIfAsked(b, wake))
	{
		// b2Body.h:915-921
		const float sx = b.invMass * ix, sy = b.invMass * iy;
		b.vx += sx;
		b.vy += sy;
		b.w += b.invI * ((px - b.cx) * iy - (py - b.cy) * ix);
	}
	return B2HIP_OK;
}

int b2hip_apply_linear_impulse_to_center(b2hip_world* w, int body, float ix, float iy, int wake)
{
	if (int rc = checkBody(w, body, "b2hip_apply_linear_impulse_to_center")) return rc;
	if (w->bodies[body].type != B2HIP_DYNAMIC_BODY) return B2HIP_OK;
	HostBody& b = editBody(w, body);
	if (wakeIfAsked(b, wake))
	{
		const float sx = b.invMass * ix, sy = b.invMass * iy; // b2Body.h:923-942
		b.vx += sx;
		b.vy += sy;
	}
	return B2HIP_OK;
}

int b2hip_apply_angular_impulse(b2hip_world* w, int body, float impulse, int wake)
{
	if (int rc = checkBody(w, body, "b2hip_apply_angular_impulse")) return rc;
	if (w->bodies[body].type != B2HIP_DYNAMIC_BODY) return B2HIP_OK;
	HostBody& b = editBody(w, body);
	if (wakeIfAsked(b, wake)) b.w += b.invI * impulse;
	return B2HIP_OK;
}

// The fat AABB a fixture's proxy has right now (the device owns it once the fixture is uploaded)
static int currentFat(b2hip_world* w, int fixture, float out4[4])
{
	if ((size_t)fixture >= w->upFixtures || std::find(w->fatEdits.begin(), w->fatEdits.end(), fixture) != w->fatEdits.end())
	{
		memcpy(out4, w->fixtures[fixture].fat, 16);
		return 0;
	}
	DEVICE_GUARD(w);
	HIP_TRY(hipStreamSynchronize(w->stream));
	HIP_TRY(hipMemcpy(out4, w->p_fat.p + fixture, 16, hipMemcpyDeviceToHost));
	return 0;
}

// b2DynamicTree::MoveProxy with zero displacement at the body's transform: a proxy whose fat AABB still holds the shape's keeps
// it; one that left it gets a new box and is queued as edited. 1: the proxy moved, 0: it stayed, negative: an error.
static int refitProxy(b2hip_world* w, const HostBody& b, int id)
{
	HostFixture& f = w->fixtures[id];
	float fat[4];
	if (int rc = currentFat(w, id, fat)) return rc;
	const AABB aabb = b2dShapeAABB(&w->shapes[f.shape], hostXf(b));
	if (fat[0] <= aabb.lo.x && fat[1] <= aabb.lo.y && aabb.hi.x <= fat[2] && aabb.hi.y <= fat[3])
	{
		memcpy(f.fat, fat, 16);
		return 0;
	}
	fatAround(aabb, f.fat);
	w->proxyEdits.push_back(id);
	w->fatEdits.push_back(id);
	return 1;
}

int b2hip_set_transform(b2hip_world* w, int body, float x, float y, float angle)
{
	if (int rc = checkBody(w, body, "b2hip_set_transform")) return rc;
	HostBody& b = editBody(w, body);
	b.qs = sinf(angle);
	b.qc = cosf(angle);
	b.px = x;
	b.py = y;
	const V2 c = b2dMulXV(hostXf(b), v2(b.lcx, b.lcy));
	b.cx = b.c0x = c.x;
	b.cy = b.c0y = c.y;
	b.a = b.a0 = angle;
	b.resetSweep = 1;
	// b2Fixture::Synchronize(broadPhase, xf, xf) for every fixture, newest first -> b2DynamicTree::MoveProxy with zero displacement
	for (int k = (int)b.fixtures.size() - 1; k >= 0; --k)
	{
		const int id = b.fixtures[k], moved = refitProxy(w, b, id);
		if (moved < 0) return moved;
		// (moves alone do not ask for the top-of-step pair update: the end-of-step one takes them)
		if (moved && ((size_t)id < w->upFixtures || std::find(w->pendingMoves.begin(), w->pendingMoves.end(), id) == w->pendingMoves.end())) w->pendingMoves.push_back(id);
	}
	return B2HIP_OK;
}

int b2hip_set_active(b2hip_world* w, int body, int active)
{
	if (int rc = checkBody(w, body, "b2hip_set_active")) return rc;
	if (((w->bodies[body].flags & BF_ACTIVE) != 0) == (active != 0)) return B2HIP_OK;
	HostBody& b = editBody(w, body);
	if (active)
	{
		b.flags |= BF_ACTIVE;
		// b2Fixture::CreateProxies for every fixture, newest first: fat AABB at the body's transform, a fresh proxy id, a buffered move
		for (int k = (int)b.fixtures.size() - 1; k >= 0; --k)
		{
			const int id = b.fixtures[k];
			HostFixture& f = w->fixtures[id];
			fatAround(b2dShapeAABB(&w->shapes[f.shape], hostXf(b)), f.fat);
			f.proxyKey = allocProxyKey(w);
			if (f.proxyKey < 0) return setError(B2HIP_ERR_UNSUPPORTED, "proxy id reuse after the broad-phase tree was emptied is not modelled");
			f.noProxy = false;
			w->proxyEdits.push_back(id);
			w->fatEdits.push_back(id);
			w->pendingMoves.push_back(id);
		}
		w->proxyListsStale = true;
		return B2HIP_OK;
	}
	b.flags &= ~BF_ACTIVE;
	// b2Fixture::DestroyProxies, newest fixture first, then the body's contacts in its contact-list order
	for (int k = (int)b.fixtures.size() - 1; k >= 0; --k)
	{
		const int id = b.fixtures[k];
		HostFixture& f = w->fixtures[id];
		if (f.noProxy) continue;
		freeProxyKey(w, f.proxyKey);
		f.proxyKey = -1;
		f.noProxy = true;
		w->proxyEdits.push_back(id);
		w->pendingMoves.erase(std::remove(w->pendingMoves.begin(), w->pendingMoves.end(), id), w->pendingMoves.end());
	}
	w->proxyListsStale = true;
	queueOp(w, EDIT_DESTROY_BODY, body);
	return B2HIP_OK;
}

int b2hip_set_type(b2hip_world* w, int body, int type)
{
	if (int rc = checkBody(w, body, "b2hip_set_type")) return rc;
	if (type < B2HIP_STATIC_BODY || type > B2HIP_DYNAMIC_BODY) return setError(B2HIP_ERR_INVALID, "b2hip_set_type: bad body type");
	if (w->bodies[body].type == type) return B2HIP_OK;
	HostBody& b = editBody(w, body);
	if (b.type == B2HIP_STATIC_BODY)
	{
		// out of m_staticBodies, to the end of m_nonStaticBodies (b2Body.cpp:131-140)
		b.worldIndex = (int)w->nonStatic.size();
		w->nonStatic.push_back(body);
		w->orderDirty = true;
	}
	b.type = type;
	resetMassData(w, b);
	b.resetSweep = 1; // (the mass data moved the sweep origin with the centre)
	if (type == B2HIP_STATIC_BODY)
	{
		b.vx = b.vy = b.w = 0.0f;
		b.a0 = b.a;
		b.c0x = b.cx;
		b.c0y = b.cy;
		b.resetSweep = 1;
		// b2Body::SynchronizeFixtures with xf1 == xf (the sweep origin was just reset): MoveProxy with zero displacement
		for (int k = (int)b.fixtures.size() - 1; k >= 0; --k)
		{
			const int id = b.fixtures[k];
			if (w->fixtures[id].noProxy) continue;
			const int moved = refitProxy(w, b, id);
			if (moved < 0) return moved;
			if (moved) w->pendingMoves.push_back(id);
		}
		// b2RemoveAndSwapBack on m_nonStaticBodies (b2Body.cpp:154-160)
		const int slot = b.worldIndex, last = w->nonStatic.back();
		w->nonStatic[(size_t)slot] = last;
		w->bodies[(size_t)last].worldIndex = slot;
		w->nonStatic.pop_back();
		b.worldIndex = -1;
		w->orderDirty = true;
	}
	b.flags |= BF_AWAKE;
	b.sleepTime = 0.0f;
	b.fx = b.fy = b.torque = 0.0f;
	// every contact of the body goes, in its contact-list order; TouchProxy on every proxy, newest fixture first
	queueOp(w, EDIT_DESTROY_BODY, body);
	for (int k = (int)b.fixtures.size() - 1; k >= 0; --k)
	{
		const int id = b.fixtures[k];
		if (!w->fixtures[id].noProxy) w->pendingMoves.push_back(id);
	}
	return B2HIP_OK;
}

int b2hip_set_awake(b2hip_world* w, int body, int awake)
{
	if (int rc = checkBody(w, body, "b2hip_set_awake")) return rc;
	if (awake)
	{
		setAwake(w, body);
		return B2HIP_OK;
	}
	HostBody& b = editBody(w, body);
	b.flags &= ~BF_AWAKE;
	b.sleepTime = 0.0f;
	b.vx = b.vy = b.w = 0.0f;
	b.fx = b.fy = b.torque = 0.0f;
	return B2HIP_OK;
}

int b2hip_set_bullet(b2hip_world* w, int body, int bullet)
{
	if (int rc = checkBody(w, body, "b2hip_set_bullet")) return rc;
	HostBody& b = editBody(w, body);
	const bool was = (b.flags & BF_BULLET) != 0;
	if (bullet) b.flags |= BF_BULLET; else b.flags &= ~BF_BULLET;
	if (was != (bullet != 0)) queueOp(w, EDIT_RECALC_BODY, body);
	return B2HIP_OK;
}

// b2Body::SetLinearDamping / SetAngularDamping / SetGravityScale (b2Body.h:620-648): read by the next Solve
int b2hip_set_body_damping(b2hip_world* w, int body, float linear_damping, float angular_damping, float gravity_scale)
{
	if (int rc = checkBody(w, body, "b2hip_set_body_damping")) return rc;
	HostBody& b = editBody(w, body);
	b.linearDamping = linear_damping;
	b.angularDamping = angular_damping;
	b.gravityScale = gravity_scale;
	return B2HIP_OK;
}

// b2Body::SetFixedRotation (b2Body.cpp:546-565): the flag, no spin, mass data again
int b2hip_set_fixed_rotation(b2hip_world* w, int body, int flag)
{
	if (int rc = checkBody(w, body, "b2hip_set_fixed_rotation")) return rc;
	HostBody& probe = w->bodies[body];
	if (((probe.flags & BF_FIXEDROT) != 0) == (flag != 0)) return B2HIP_OK;
	HostBody& b = editBody(w, body);
	if (flag) b.flags |= BF_FIXEDROT; else b.flags &= ~BF_FIXEDROT;
	b.w = 0.0f;
	resetMassData(w, b);
	b.resetSweep = 1;
	return B2HIP_OK;
}

// b2Body::SetSleepingAllowed (b2Body.h:674-688): a body that may not sleep is woken
int b2hip_set_sleeping_allowed(b2hip_world* w, int body, int flag)
{
	if (int rc = checkBody(w, body, "b2hip_set_sleeping_allowed")) return rc;
	HostBody& b = editBody(w, body);
	if (flag) b.flags |= BF_AUTOSLEEP;
	else
	{
		b.flags &= ~BF_AUTOSLEEP;
		b.flags |= BF_AWAKE; // SetAwake(true) (b2Body.h:690-718): the sleep timer restarts whether or not the body slept
		b.sleepTime = 0.0f;
	}
	return B2HIP_OK;
}

