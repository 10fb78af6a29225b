// b2hip_api_body_props.h - batched body property sets between steps (include/b2hip.h, block K: b2hip_set_types,
// b2hip_set_bullets, b2hip_set_fixed_rotations, b2hip_set_sleeping_alloweds, b2hip_set_body_dampings, b2hip_set_mass_datas,
// b2hip_reset_mass_datas; kernels: b2d_kernels_body_props.h).
//
// Seven more write calls of the family of b2hip_api_body_writes.h, b2hip_api_body_lifecycle.h and b2hip_api_fixture_batch.h. The
// single calls (b2hip_api_bodies.h) edit the host's mirror - markDirty -> pullBody, then eight rows per dirty body uploaded by
// the next flushEdits - and b2hip_set_type / b2hip_set_bullet queue one contact-array op per body for k_apply_edits; these
// calls edit the device's rows in one launch and visit the contact array once per call. No editBody / markDirty, no proxyEdits,
// fatEdits, pendingMoves or queueOp.
//   pending edits   go first, queued contact ops included (lifecycleBegin): they lie underneath the call.
//   host-only       fields follow at once, in entry order: the dampings, the type, the seed order (nonStatic, worldIndex,
//                   orderDirty), mass, I, invMass, invI and the local centre - computed by the functions the single calls use
//                   (massFromFixtures, massFromData: the fixtures, shapes and densities are the host's) - and the host's copy of
//                   the bullet, fixed-rotation and auto-sleep bits, which the single calls test before they pull anything.
//   device rows     a body whose rows the launch changed is marked as not pulled (bodyWritesMirror): the next markDirty reads
//                   its row again. Nothing is queued for upload. b2hip_set_types marks before the tail of the contact pass,
//                   whose read-back is the newer one; its force rows are zeroed on the device (BODY_FORCES_ZEROED).
//   mouse joints    read their body's mass through refreshMouseMasses at the next flushEdits: the host's `mass` being right is
//                   all they need.
//   the TOI list    of b2hip_set_bullets borrows the pair update's key buffer and block J's sort and replay
//                   (toiCandidacyBatch); the contacts of b2hip_set_types go the way of block I's (lifecycleContacts).

extern "C++"
{
// What every call of the block checks, in the header's order; *done: nothing is left to do (n == 0).
static int bodyPropsBegin(b2hip_world* w, const char* what, int n, const int32_t* bodies, const void* values, const std::string& bad, bool* done)
{
	*done = false;
	if (int rc = bodyWritesArgs(what, n, bodies, values, what)) return rc; // (a write call has no output: any non-null pointer)
	if (int rc = queryUsable(w, what)) return rc;
	if (!bad.empty()) return setError(B2HIP_ERR_INVALID, std::string(what) + bad);
	if (int rc = bodyContactsIds(w, what, n, bodies, true, true)) return rc;
	*done = n == 0;
	return B2HIP_OK;
}

// the static body's awake flag, which setAwake tests on the host before it pulls anything (b2hip_set_awakes)
static void bodyPropsStaticAwake(b2hip_world* w, int body)
{
	HostBody& b = w->bodies[(size_t)body];
	if (b.type == B2HIP_STATIC_BODY) b.flags |= BF_AWAKE;
}

static BodyMassRec bodyMassRec(const BodyMass& m, uint32_t op)
{
	BodyMassRec r;
	r.invMass = m.invMass;
	r.invI = m.invI;
	r.lcx = m.localCenter.x;
	r.lcy = m.localCenter.y;
	r.op = op;
	r.pad0 = r.pad1 = r.pad2 = 0u;
	return r;
}

// b2hip_set_sleeping_alloweds / b2hip_set_bullets
template <int KIND>
static int bodyFlagSets(b2hip_world* w, const char* what, int n, const int32_t* bodies, const uint8_t* flag)
{
	bool done;
	if (int rc = bodyPropsBegin(w, what, n, bodies, flag, std::string(), &done)) return rc;
	if (done) return B2HIP_OK;
	DEVICE_GUARD(w);
	if (int rc = lifecycleBegin(w)) return rc;
	const uint32_t bit = KIND == BODY_PROP_SLEEPING ? BF_AUTOSLEEP : BF_BULLET;
	std::vector<uint8_t> recs((size_t)n);
	std::vector<int32_t> part;
	for (int i = 0; i < n; ++i)
	{
		HostBody& b = w->bodies[(size_t)bodies[i]];
		const bool want = flag[i] != 0, changes = ((b.flags & bit) != 0) != want;
		recs[(size_t)i] = (uint8_t)((want ? 1 : 0) | (changes ? 2 : 0));
		b.flags = want ? (b.flags | bit) : (b.flags & ~bit);
		// (SetSleepingAllowed(false) wakes whether or not the flag changes; SetBullet changes a row only where the bit does)
		if (KIND == BODY_PROP_SLEEPING ? (changes || !want) : changes) part.push_back(bodies[i]);
		if (KIND == BODY_PROP_SLEEPING && !want) bodyPropsStaticAwake(w, bodies[i]);
	}
	int rc = w->lcNamed.ensure(std::max<size_t>(w->bodies.size(), 1), w->stream, false, true); // (every word 0 between calls)
	if (!rc) rc = w->lcWords.ensure(4, w->stream, false, true);
	if (!rc) rc = bodyWritesStage(w, n, bodies, recs.data(), (size_t)n, 0);
	if (rc) return lifecycleDone(w, rc);
	auto device = [&]() -> int {
		LAUNCH(w, k_body_flag_sets<KIND>, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, (const uint8_t*)w->bwIn.p, w->dw.nBodies, w->b_flags.p, w->b_pos.p,
		       w->lcNamed.p);
		if (int rcm = bodyWritesMirror(w, (int)part.size(), part.data(), BODY_FORCES_NONE)) return rcm; // (drains the stream)
		if (KIND == BODY_PROP_SLEEPING || part.empty()) return B2HIP_OK;
		const int nContacts = std::max(w->h_dstate->c.nContacts, 0);
		auto listPass = [&](int room) -> int {
			LAUNCH(w, k_body_bullet_contacts, gridFor((size_t)std::max(nContacts, 1)), 256, w->dw, (const int*)w->lcNamed.p, (unsigned long long*)w->dw.pairKey, room,
			       w->lcWords.p);
			return B2HIP_OK;
		};
		auto unname = [&]() -> int {
			LAUNCH(w, k_lifecycle_unname, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, w->dw.nBodies, w->lcNamed.p);
			return B2HIP_OK;
		};
		return toiCandidacyBatch(w, n, listPass, unname);
	};
	return lifecycleDone(w, device());
}

// The mass-data calls behind their host bookkeeping: recs one BodyMassRec per entry, part the bodies whose rows change.
static int bodyMassDevice(b2hip_world* w, int n, const int32_t* bodies, const std::vector<BodyMassRec>& recs, const std::vector<int32_t>& part)
{
	int rc = w->lcNamed.ensure(std::max<size_t>(w->bodies.size(), 1), w->stream, false, true);
	if (!rc) rc = bodyWritesStage(w, n, bodies, recs.data(), recs.size() * sizeof(BodyMassRec), 0);
	if (rc) return rc;
	LAUNCH(w, k_body_mass_rows, gridFor((size_t)n), 256, w->dw, (const int*)w->bcIds.p, (const BodyMassRec*)w->bwIn.p, n, w->lcNamed.p);
	return bodyWritesMirror(w, (int)part.size(), part.data(), BODY_FORCES_NONE); // (drains the stream: the pinned buffer is the next call's)
}

// b2hip_set_mass_datas / b2hip_reset_mass_datas (md == nullptr: the call has no records, the ids stand in for them)
static int bodyMassDatas(b2hip_world* w, const char* what, int n, const int32_t* bodies, const b2hip_mass_data* md, bool reset)
{
	bool done;
	if (int rc = bodyPropsBegin(w, what, n, bodies, reset ? (const void*)bodies : (const void*)md, std::string(), &done)) return rc;
	if (done) return B2HIP_OK;
	DEVICE_GUARD(w);
	if (int rc = lifecycleBegin(w)) return rc;
	std::vector<BodyMassRec> recs((size_t)n);
	std::vector<int32_t> part;
	for (int i = 0; i < n; ++i)
	{
		HostBody& b = w->bodies[(size_t)bodies[i]];
		if (md && b.type != B2HIP_DYNAMIC_BODY)
		{
			// b2Body::SetMassData leaves a body that is not dynamic alone (the single call has uploaded its rows all the same)
			recs[(size_t)i] = bodyMassRec(BodyMass{ b.mass, b.I, b.invMass, b.invI, v2(b.lcx, b.lcy) }, BODY_MASS_UPLOADS);
			continue;
		}
		const BodyMass m = md ? massFromData(b, md + i) : massFromFixtures(w, b);
		storeMass(b, m);
		recs[(size_t)i] = bodyMassRec(m, BODY_MASS_PART | (b.type != B2HIP_DYNAMIC_BODY ? BODY_MASS_ORIGIN : 0u));
		part.push_back(bodies[i]);
	}
	return lifecycleDone(w, bodyMassDevice(w, n, bodies, recs, part));
}
} // extern "C++"

int b2hip_set_body_dampings(b2hip_world* w, int n, const int32_t* bodies, const b2hip_body_damping* d, int mask)
{
	const char* what = "b2hip_set_body_dampings";
	const int all = B2HIP_DAMPING_LINEAR | B2HIP_DAMPING_ANGULAR | B2HIP_DAMPING_GRAVITY_SCALE;
	bool done;
	if (int rc = bodyPropsBegin(w, what, n, bodies, d, (mask & ~all) != 0 || mask == 0 ? ": mask must be a non-empty subset of the three B2HIP_DAMPING_* bits" : "", &done))
		return rc;
	if (done) return B2HIP_OK;
	DEVICE_GUARD(w);
	if (int rc = lifecycleBegin(w)) return rc;
	for (int i = 0; i < n; ++i)
	{
		HostBody& b = w->bodies[(size_t)bodies[i]];
		if (mask & B2HIP_DAMPING_LINEAR) b.linearDamping = d[i].linear_damping;
		if (mask & B2HIP_DAMPING_ANGULAR) b.angularDamping = d[i].angular_damping;
		if (mask & B2HIP_DAMPING_GRAVITY_SCALE) b.gravityScale = d[i].gravity_scale;
	}
	int rc = bodyWritesStage(w, n, bodies, d, (size_t)n * sizeof(b2hip_body_damping), 0);
	if (rc) return lifecycleDone(w, rc);
	auto device = [&]() -> int {
		LAUNCH(w, k_body_dampings, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, (const float4*)w->bwIn.p, mask, w->dw.nBodies, w->b_damp.p, w->b_flags.p);
		HIP_TRY(hipStreamSynchronize(w->stream)); // (the pinned buffer is the next call's; the state rows carry no damping)
		return B2HIP_OK;
	};
	return lifecycleDone(w, device());
}

int b2hip_set_sleeping_alloweds(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* flag)
{
	return bodyFlagSets<BODY_PROP_SLEEPING>(w, "b2hip_set_sleeping_alloweds", n, bodies, flag);
}

int b2hip_set_bullets(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* bullet)
{
	return bodyFlagSets<BODY_PROP_BULLETS>(w, "b2hip_set_bullets", n, bodies, bullet);
}

int b2hip_set_fixed_rotations(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* flag)
{
	const char* what = "b2hip_set_fixed_rotations";
	bool done;
	if (int rc = bodyPropsBegin(w, what, n, bodies, flag, std::string(), &done)) return rc;
	if (done) return B2HIP_OK;
	DEVICE_GUARD(w);
	if (int rc = lifecycleBegin(w)) return rc;
	std::vector<BodyMassRec> recs((size_t)n);
	std::vector<int32_t> part;
	for (int i = 0; i < n; ++i)
	{
		HostBody& b = w->bodies[(size_t)bodies[i]];
		const bool want = flag[i] != 0;
		if (((b.flags & BF_FIXEDROT) != 0) == want)
		{
			// (the single call returns before it pulls anything: the entry takes no part)
			recs[(size_t)i] = bodyMassRec(BodyMass{ b.mass, b.I, b.invMass, b.invI, v2(b.lcx, b.lcy) }, 0u);
			continue;
		}
		b.flags = want ? (b.flags | BF_FIXEDROT) : (b.flags & ~(uint32_t)BF_FIXEDROT);
		const BodyMass m = massFromFixtures(w, b);
		storeMass(b, m);
		recs[(size_t)i] = bodyMassRec(m, BODY_MASS_PART | BODY_MASS_ZERO_SPIN | (want ? BODY_MASS_FIXED_ON : BODY_MASS_FIXED_OFF) |
		                                     (b.type != B2HIP_DYNAMIC_BODY ? BODY_MASS_ORIGIN : 0u));
		part.push_back(bodies[i]);
	}
	if (part.empty()) return B2HIP_OK;
	return lifecycleDone(w, bodyMassDevice(w, n, bodies, recs, part));
}

int b2hip_set_mass_datas(b2hip_world* w, int n, const int32_t* bodies, const b2hip_mass_data* md)
{
	return bodyMassDatas(w, "b2hip_set_mass_datas", n, bodies, md, false);
}

int b2hip_reset_mass_datas(b2hip_world* w, int n, const int32_t* bodies)
{
	return bodyMassDatas(w, "b2hip_reset_mass_datas", n, bodies, nullptr, true);
}

int b2hip_set_types(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* type)
{
	const char* what = "b2hip_set_types";
	std::string bad;
	if (n > 0 && n <= B2HIP_QUERY_MAX && bodies && type) // (n and the pointers are refused first, then the world: bodyPropsBegin)
		for (int i = 0; i < n && bad.empty(); ++i)
			if (type[i] > B2HIP_DYNAMIC_BODY) bad = ": entry " + std::to_string(i) + " asks for type " + std::to_string((int)type[i]) + ", which is no body type";
	bool done;
	if (int rc = bodyPropsBegin(w, what, n, bodies, type, bad, &done)) return rc;
	if (done) return B2HIP_OK;
	DEVICE_GUARD(w);
	if (int rc = lifecycleBegin(w)) return rc;
	// An entry whose type is the requested one already takes no part. Every proxy of a changing active body is buffered as moved
	// (TouchProxy), newest fixture first within a body, bodies in entry order, behind the moves the device holds.
	std::vector<int32_t> part, toStatic;
	std::vector<int2> moves;
	for (int i = 0; i < n; ++i)
	{
		const HostBody& b = w->bodies[(size_t)bodies[i]];
		if (b.type == (int)type[i]) continue;
		part.push_back(bodies[i]);
		for (int k = (int)b.fixtures.size() - 1; k >= 0; --k)
		{
			const int fid = b.fixtures[(size_t)k];
			if (w->fixtures[(size_t)fid].noProxy) continue;
			if (type[i] == B2HIP_STATIC_BODY) toStatic.push_back(fid);
			moves.push_back(make_int2(fid, (int)moves.size()));
		}
	}
	if (part.empty()) return B2HIP_OK;
	const int buffered = w->h_dstate->c.nMoves;
	if (buffered < 0 || (size_t)buffered + moves.size() > (size_t)w->dw.capMoves)
		return setError(B2HIP_ERR_UNSUPPORTED, std::string(what) + ": the move buffer holds " + std::to_string(buffered) + " of " + std::to_string(w->dw.capMoves) +
		                " entries and the batch can add " + std::to_string(moves.size()) + ": step the world first");
	int rc = w->lcNamed.ensure(std::max<size_t>(w->bodies.size(), 1), w->stream, false, true); // (every word 0 between calls: k_lifecycle_unname)
	if (!rc) rc = w->lcWords.ensure(4, w->stream, false, true);
	if (rc) return rc;
	if (!toStatic.empty())
	{
		// A body that turns static synchronises its fixtures with zero displacement (refitProxy): a proxy moves only if its fat
		// AABB no longer holds its shape's box, which a step and a flushed teleport both see to. Should one have, the batch IS the
		// loop of single calls - between the pending edits and the application of what the loop queued, as b2hip_destroy_bodies
		// treats a jointed batch. Nothing has been written so far.
		int left = 0;
		auto census = [&]() -> int {
			if (int rcs = bodyWritesStage(w, (int)toStatic.size(), toStatic.data(), nullptr, 0, 0)) return rcs;
			HIP_TRY(hipMemsetAsync(w->lcWords.p + 1, 0, sizeof(int), w->stream));
			LAUNCH(w, k_body_refit_count, gridFor(toStatic.size()), 256, w->dw, (const int*)w->bcIds.p, (int)toStatic.size(), w->lcWords.p + 1);
			HIP_TRY(hipMemcpyAsync(&left, w->lcWords.p + 1, sizeof(int), hipMemcpyDeviceToHost, w->stream));
			HIP_TRY(hipStreamSynchronize(w->stream));
			return B2HIP_OK;
		};
		if ((rc = census())) return lifecycleDone(w, rc);
		if (left != 0)
		{
			w->statBodyPropRefits += 1;
			for (int i = 0; i < n; ++i)
				if ((rc = b2hip_set_type(w, bodies[i], (int)type[i]))) return lifecycleDone(w, rc);
			return lifecycleDone(w, lifecycleBegin(w));
		}
	}
	// the host's bookkeeping, in entry order (b2hip_set_type)
	std::vector<BodyMassRec> recs((size_t)n);
	for (int i = 0; i < n; ++i)
	{
		const int id = bodies[i];
		HostBody& b = w->bodies[(size_t)id];
		if (b.type == (int)type[i])
		{
			recs[(size_t)i] = bodyMassRec(BodyMass{ b.mass, b.I, b.invMass, b.invI, v2(b.lcx, b.lcy) }, 0u);
			continue;
		}
		if (b.type == B2HIP_STATIC_BODY)
		{
			// out of m_staticBodies, to the end of m_nonStaticBodies (b2Body.cpp:131-140)
			b.worldIndex = (int)w->nonStatic.size();
			w->nonStatic.push_back(id);
			w->orderDirty = true;
		}
		b.type = (int)type[i];
		const BodyMass m = massFromFixtures(w, b);
		storeMass(b, m);
		uint32_t op = BODY_MASS_PART | BODY_MASS_TYPE | ((uint32_t)type[i] << BODY_MASS_TYPE_SHIFT);
		if (type[i] != B2HIP_DYNAMIC_BODY) op |= BODY_MASS_ORIGIN;
		if (type[i] == B2HIP_STATIC_BODY)
		{
			op |= BODY_MASS_STATIC;
			// b2RemoveAndSwapBack on m_nonStaticBodies (b2Body.cpp:154-160)
			const int slot = b.worldIndex, last = w->nonStatic.back();
			w->nonStatic[(size_t)slot] = last;
			w->bodies[(size_t)last].worldIndex = slot;
			w->nonStatic.pop_back();
			b.worldIndex = -1;
			w->orderDirty = true;
		}
		b.flags |= BF_AWAKE; // (setAwake tests a static body's flag on the host before it pulls anything)
		recs[(size_t)i] = bodyMassRec(m, op);
	}
	auto device = [&]() -> int {
		const int nToi = std::max(w->h_dstate->c.nToiOrder, 0), nContacts = std::max(w->h_dstate->c.nContacts, 0);
		const int eventsBefore = w->h_dstate->c.nEvents;
		// the records, and behind them (16-byte aligned: a record is 32 bytes) the moves
		std::vector<char> blob(recs.size() * sizeof(BodyMassRec) + moves.size() * sizeof(int2));
		memcpy(blob.data(), recs.data(), recs.size() * sizeof(BodyMassRec));
		if (!moves.empty()) memcpy(blob.data() + recs.size() * sizeof(BodyMassRec), moves.data(), moves.size() * sizeof(int2));
		if (int rcs = bodyWritesStage(w, n, bodies, blob.data(), blob.size(), 0)) return rcs;
		const BodyMassRec* dRecs = (const BodyMassRec*)w->bwIn.p;
		LAUNCH(w, k_body_mass_rows, gridFor((size_t)n), 256, w->dw, (const int*)w->bcIds.p, dRecs, n, w->lcNamed.p);
		if (!moves.empty())
			LAUNCH(w, k_body_prop_moves, gridFor(moves.size()), 256, w->dw, (const int2*)(dRecs + n), (int)moves.size(), buffered, (int)moves.size());
		// (the mirror before the tail: its read-back is the newer one)
		if (int rcm = bodyWritesMirror(w, (int)part.size(), part.data(), BODY_FORCES_ZEROED)) return rcm;
		return lifecycleContacts(w, n, nToi, nContacts, eventsBefore);
	};
	return lifecycleDone(w, device());
}
