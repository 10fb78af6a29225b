// b2hip_host_upload.h - part of the ONE translation unit b2hip.hip: what the host edited between steps on its way to the
// device - flushEdits as a list of stages (rows of dirty bodies, tables, joint edits, proxies, moves), the re-filter marks of
// new and destroyed joints (applyPendingFilters), the queued contact-array ops (applyEditOps).
// (No include guard on purpose: b2hip.hip includes it exactly once, in order - the fragments share one scope.)

// Every dirty body gets all its rows rewritten from the host mirror, one set of copies per run of consecutive ids.
static int uploadDirtyBodies(b2hip_world* w)
{
	hipStream_t s = w->stream;
	const size_t nb = w->bodies.size();
	std::sort(w->dirtyList.begin(), w->dirtyList.end());
	w->dirtyList.erase(std::unique(w->dirtyList.begin(), w->dirtyList.end()), w->dirtyList.end());
	std::vector<float4> pos, pos0, vel, xf, mass, damp, force;
	std::vector<uint32_t> flags;
	size_t di = 0;
	while (di < w->dirtyList.size())
	{
		const size_t i = (size_t)w->dirtyList[di];
		size_t j = i;
		pos.clear(); pos0.clear(); vel.clear(); xf.clear(); mass.clear(); damp.clear(); force.clear(); flags.clear();
		while (di < w->dirtyList.size() && (size_t)w->dirtyList[di] == j)
		{
			HostBody& b = w->bodies[j];
			pos.push_back(make_float4(b.cx, b.cy, b.a, b.sleepTime));
			pos0.push_back(make_float4(b.c0x, b.c0y, b.a0, 0.0f));
			vel.push_back(make_float4(b.vx, b.vy, b.w, 0.0f));
			xf.push_back(make_float4(b.px, b.py, b.qs, b.qc));
			mass.push_back(make_float4(b.invMass, b.invI, b.lcx, b.lcy));
			damp.push_back(make_float4(b.linearDamping, b.angularDamping, b.gravityScale, 0.0f));
			force.push_back(make_float4(b.fx, b.fy, b.torque, 0.0f));
			if (b.fx != 0.0f || b.fy != 0.0f || b.torque != 0.0f) w->forceOnDevice = true;
			flags.push_back((b.flags & ~BF_TYPE_MASK) | (uint32_t)b.type);
			b.dirty = false;
			++j;
			++di;
		}
		const size_t cnt = j - i;
		HIP_TRY(hipMemcpyAsync(w->b_pos.p + i, pos.data(), cnt * sizeof(float4), hipMemcpyHostToDevice, s));
		// the sweep origin (c0, a0, alpha0) is device-owned state: only NEW bodies get it from the host mirror, an edited
		// body keeps the one the last solve left (the read-back does not carry it, and TOI needs the true one)
		if (i + cnt > w->upBodies)
		{
			const size_t first = std::max(i, w->upBodies);
			HIP_TRY(hipMemcpyAsync(w->b_pos0.p + first, pos0.data() + (first - i), (i + cnt - first) * sizeof(float4), hipMemcpyHostToDevice, s));
		}
		for (size_t k = 0; k < cnt; ++k)
		{
			// b2Body::SetTransform moves the sweep origin too (b2Body.cpp:463-467)
			if (w->bodies[i + k].resetSweep && i + k < w->upBodies)
				HIP_TRY(hipMemcpyAsync(w->b_pos0.p + i + k, pos0.data() + k, sizeof(float4), hipMemcpyHostToDevice, s));
			w->bodies[i + k].resetSweep = 0;
		}
		HIP_TRY(hipMemcpyAsync(w->b_vel.p + i, vel.data(), cnt * sizeof(float4), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(w->b_xf.p + i, xf.data(), cnt * sizeof(float4), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(w->b_mass.p + i, mass.data(), cnt * sizeof(float4), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(w->b_damp.p + i, damp.data(), cnt * sizeof(float4), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(w->b_force.p + i, force.data(), cnt * sizeof(float4), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(w->b_flags.p + i, flags.data(), cnt * sizeof(uint32_t), hipMemcpyHostToDevice, s));
		HIP_TRY(hipStreamSynchronize(s)); // staging vectors are reused
	}
	w->dirtyList.clear();
	w->upBodies = nb;
	return 0;
}

// The island seed order (m_nonStaticBodies): rewritten whole when a non-static body was created or destroyed.
static int uploadSeedOrder(b2hip_world* w)
{
	if (!w->orderDirty) return 0;
	const size_t nb = w->bodies.size();
	std::vector<int> order(nb, 0x7fffffff);
	for (size_t k = 0; k < w->nonStatic.size(); ++k) order[(size_t)w->nonStatic[k]] = (int)k;
	HIP_TRY(hipMemcpyAsync(w->b_order.p, order.data(), nb * sizeof(int), hipMemcpyHostToDevice, w->stream));
	if (!w->nonStatic.empty()) HIP_TRY(hipMemcpyAsync(w->orderBody.p, w->nonStatic.data(), w->nonStatic.size() * sizeof(int), hipMemcpyHostToDevice, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	w->orderDirty = false;
	return 0;
}

// Shapes: a small table, rewritten whole when it grew. Joints and gears: the new ones are appended; the device keeps the
// persistent impulses of the ones it already has.
static int uploadTables(b2hip_world* w)
{
	hipStream_t s = w->stream;
	if (w->upShapes != w->shapes.size())
	{
		HIP_TRY(hipMemcpyAsync(w->d_shapes.p, w->shapes.data(), w->shapes.size() * sizeof(ShapeRec), hipMemcpyHostToDevice, s));
		w->upShapes = w->shapes.size();
	}
	if (w->upJoints != w->joints.size())
	{
		const size_t first = w->upJoints, cnt = w->joints.size() - first;
		HIP_TRY(hipMemcpyAsync(w->d_joints.p + first, w->joints.data() + first, cnt * sizeof(RevoluteJoint), hipMemcpyHostToDevice, s));
		w->upJoints = w->joints.size();
	}
	if (w->upGears != w->gears.size())
	{
		const size_t first = w->upGears, cnt = w->gears.size() - first;
		HIP_TRY(hipMemcpyAsync(w->d_gears.p + first, w->gears.data() + first, cnt * sizeof(GearRec), hipMemcpyHostToDevice, s));
		w->upGears = w->gears.size();
	}
	return 0;
}

// A mouse joint reads bodyB's mass (b2MouseJoint.cpp:110), which a fixture added later changes: such a joint is queued as edited.
static void refreshMouseMasses(b2hip_world* w)
{
	if (w->nMouseJoints <= 0) return;
	for (size_t k = 0; k < w->upJoints; ++k)
	{
		JointRec& j = w->joints[k];
		if (j.type == B2D_JOINT_MOUSE && j.bodyMass != w->bodies[j.bodyB].mass)
		{
			j.bodyMass = w->bodies[j.bodyB].mass;
			queueJointEdit(w, (int)k, JOINT_EDIT_ANCHORS);
		}
	}
}

// The members a setter may have changed, per queued edit in call order (JointEditKind); everything else in the device record is
// solver state.
static int uploadJointEdits(b2hip_world* w)
{
	hipStream_t s = w->stream;
	for (size_t k = 0; k < w->jointEdits.size(); ++k)
	{
		const int id = w->jointEdits[k].joint, kind = w->jointEdits[k].kind;
		char* dst = (char*)(w->d_joints.p + id);
		const char* src = (const char*)&w->joints[id];
		const size_t off = offsetof(JointRec, enableLimit), len = offsetof(JointRec, collideConnected) - off;
		HIP_TRY(hipMemcpyAsync(dst + off, src + off, len, hipMemcpyHostToDevice, s));
		if (kind == JOINT_EDIT_ANCHORS)
		{
			const size_t o2 = offsetof(JointRec, localAnchorA), l2 = offsetof(JointRec, enableLimit) - o2;
			HIP_TRY(hipMemcpyAsync(dst + o2, src + o2, l2, hipMemcpyHostToDevice, s));
		}
		if (kind == JOINT_EDIT_DESTROY)
			HIP_TRY(hipMemcpyAsync(dst + offsetof(JointRec, type), &w->joints[id].type, sizeof(int), hipMemcpyHostToDevice, s));
		static const float zero = 0.0f;
		if (kind == JOINT_EDIT_LIMITS)
			HIP_TRY(hipMemcpyAsync(dst + offsetof(JointRec, impulseZ), &zero, sizeof(float), hipMemcpyHostToDevice, s));
	}
	w->jointEdits.clear();
	return 0;
}

// Per-body joint edges, newest first (b2World.cpp:697-710): a CSR by counting, rebuilt only when bodies or joints were added
// (or a joint destroyed: b2hip_destroy_joint resets jadjJoints).
static int uploadJointAdjacency(b2hip_world* w)
{
	if (w->jadjBodies == w->bodies.size() && w->jadjJoints == w->joints.size()) return 0;
	const size_t nbod = w->bodies.size();
	w->jadjBodies = nbod;
	w->jadjJoints = w->joints.size();
	std::vector<int> start(nbod + 1, 0), adj;
	for (size_t j = 0; j < w->joints.size(); ++j)
	{
		if (w->joints[j].type == B2D_JOINT_DEAD) continue;
		start[w->joints[j].bodyA + 1] += 1;
		if (w->joints[j].bodyB != w->joints[j].bodyA) start[w->joints[j].bodyB + 1] += 1;
	}
	for (size_t b = 0; b < nbod; ++b) start[b + 1] += start[b];
	adj.resize((size_t)start[nbod]);
	std::vector<int> cursor(start.begin(), start.end() - 1);
	for (int j = (int)w->joints.size() - 1; j >= 0; --j)
	{
		if (w->joints[j].type == B2D_JOINT_DEAD) continue;
		adj[(size_t)cursor[w->joints[j].bodyA]++] = j;
		if (w->joints[j].bodyB != w->joints[j].bodyA) adj[(size_t)cursor[w->joints[j].bodyB]++] = j;
	}
	HIP_TRY(hipMemcpyAsync(w->jadjStart.p, start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice, w->stream));
	if (!adj.empty()) HIP_TRY(hipMemcpyAsync(w->jadj.p, adj.data(), adj.size() * sizeof(int), hipMemcpyHostToDevice, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	return 0;
}

// The per-body proxy lists, newest first like b2Body::m_fixtureList (b2Body.cpp:203-205): head per body, next per fixture; a
// destroyed fixture and one without a proxy are in no list.
static void buildProxyLists(const b2hip_world* w, std::vector<int>& head, std::vector<int>& next)
{
	head.assign(w->bodies.size(), -1);
	next.assign(w->fixtures.size(), -1);
	for (size_t k = 0; k < w->fixtures.size(); ++k)
	{
		if (w->fixtures[k].dead || w->fixtures[k].noProxy) continue;
		const int b = w->fixtures[k].body;
		next[k] = head[b];
		head[b] = (int)k;
	}
}

static int uploadProxyLists(b2hip_world* w)
{
	std::vector<int> head, next;
	buildProxyLists(w, head, next);
	HIP_TRY(hipMemcpyAsync(w->b_proxyHead.p, head.data(), head.size() * sizeof(int), hipMemcpyHostToDevice, w->stream));
	HIP_TRY(hipMemcpyAsync(w->p_next.p, next.data(), next.size() * sizeof(int), hipMemcpyHostToDevice, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	w->proxyListsStale = false;
	return 0;
}

// The device's record of a fixture's proxy, shape index aside: owner -1 once the fixture is destroyed or its body inactive.
struct ProxyWords
{
	float4 fat;
	int body, key;
	uint32_t filter0;
	int filter1;
	float2 mat;
};
static ProxyWords proxyWords(const HostFixture& f)
{
	ProxyWords p;
	p.fat = make_float4(f.fat[0], f.fat[1], f.fat[2], f.fat[3]);
	p.body = (f.dead || f.noProxy) ? -1 : f.body;
	p.key = f.proxyKey;
	p.filter0 = (uint32_t)f.categoryBits | ((uint32_t)f.maskBits << 16);
	p.filter1 = ((int)(uint16_t)f.groupIndex) | (f.isSensor ? PF_SENSOR : 0) | (f.thick ? PF_THICK : 0);
	p.mat = make_float2(f.friction, f.restitution);
	return p;
}

// Broad-phase cell: 1.5 x the largest fat extent among non-static proxies, ignoring outliers
// (> 8 x median), which are handled by the brute-force "large proxy" path.
static void chooseCell(b2hip_world* w)
{
	std::vector<float> ext;
	for (size_t k = 0; k < w->fixtures.size(); ++k)
	{
		const HostFixture& f = w->fixtures[k];
		if (f.dead || f.noProxy || w->bodies[f.body].type == B2HIP_STATIC_BODY) continue;
		ext.push_back(std::max(f.fat[2] - f.fat[0], f.fat[3] - f.fat[1]));
	}
	float cell = 1.0f;
	if (!ext.empty())
	{
		std::sort(ext.begin(), ext.end());
		float median = ext[ext.size() / 2];
		float mx = median;
		for (size_t k = 0; k < ext.size(); ++k)
			if (ext[k] <= 8.0f * median) mx = std::max(mx, ext[k]);
		cell = 1.5f * mx;
	}
	w->dw.cellSize = cell;
	w->dw.invCellSize = 1.0f / cell;
}

// Fixtures created since the last upload: their seven arrays, the proxy lists with them in, the cell size they ask for.
static int uploadNewProxies(b2hip_world* w)
{
	const size_t np = w->fixtures.size();
	if (w->upFixtures >= np) return 0;
	hipStream_t s = w->stream;
	const size_t first = w->upFixtures, cnt = np - first;
	std::vector<float4> fat(cnt);
	std::vector<int> body(cnt), shape(cnt), key(cnt), f1(cnt);
	std::vector<uint32_t> f0(cnt);
	std::vector<float2> mat(cnt);
	for (size_t k = 0; k < cnt; ++k)
	{
		const ProxyWords p = proxyWords(w->fixtures[first + k]);
		fat[k] = p.fat; body[k] = p.body; shape[k] = w->fixtures[first + k].shape; key[k] = p.key;
		f0[k] = p.filter0; f1[k] = p.filter1; mat[k] = p.mat;
	}
	HIP_TRY(hipMemcpyAsync(w->p_fat.p + first, fat.data(), cnt * sizeof(float4), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(w->p_body.p + first, body.data(), cnt * sizeof(int), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(w->p_shape.p + first, shape.data(), cnt * sizeof(int), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(w->p_key.p + first, key.data(), cnt * sizeof(int), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(w->p_filter0.p + first, f0.data(), cnt * sizeof(uint32_t), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(w->p_filter1.p + first, f1.data(), cnt * sizeof(int), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(w->p_mat.p + first, mat.data(), cnt * sizeof(float2), hipMemcpyHostToDevice, s));
	if (int rc = uploadProxyLists(w)) return rc; // (its synchronisation frees the staging vectors above)
	w->upFixtures = np;
	chooseCell(w);
	return 0;
}

// Edited proxies of fixtures the device already has: fat AABB (SetTransform), filter words (SetFilterData, SetSensor,
// SetThickShape), owner (-1: the fixture was destroyed), material - one blocking copy per word.
static int uploadProxyEdits(b2hip_world* w)
{
	if (w->proxyEdits.empty()) return 0;
	std::sort(w->proxyEdits.begin(), w->proxyEdits.end());
	w->proxyEdits.erase(std::unique(w->proxyEdits.begin(), w->proxyEdits.end()), w->proxyEdits.end());
	for (size_t k = 0; k < w->proxyEdits.size(); ++k)
	{
		const int id = w->proxyEdits[k];
		if ((size_t)id >= w->upFixtures) continue; // (a new fixture: uploaded whole above)
		const ProxyWords p = proxyWords(w->fixtures[id]);
		// (the fat AABB of an uploaded fixture is device state: the host copy is only current if SetTransform wrote it)
		if (std::find(w->fatEdits.begin(), w->fatEdits.end(), id) != w->fatEdits.end())
			HIP_TRY(hipMemcpy(w->p_fat.p + id, &p.fat, sizeof(float4), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(w->p_body.p + id, &p.body, sizeof(int), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(w->p_key.p + id, &p.key, sizeof(int), hipMemcpyHostToDevice)); // (a re-activated body's proxies have new ids)
		HIP_TRY(hipMemcpy(w->p_filter0.p + id, &p.filter0, sizeof(uint32_t), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(w->p_filter1.p + id, &p.filter1, sizeof(int), hipMemcpyHostToDevice));
		// (b2Fixture::SetFriction / SetRestitution: for contacts created from now on)
		HIP_TRY(hipMemcpy(w->p_mat.p + id, &p.mat, sizeof(float2), hipMemcpyHostToDevice));
	}
	w->proxyEdits.clear();
	w->fatEdits.clear();
	return 0;
}

// The move buffer: proxies created or moved since the last step go behind the moves the device still holds
// (b2BroadPhase::CreateProxy buffers a move).
static int appendPendingMoves(b2hip_world* w)
{
	if (w->pendingMoves.empty()) return 0;
	if (int rc = readState(w)) return rc;
	int have = w->h_dstate->c.nMoves;
	HIP_TRY(hipMemcpyAsync(w->moveBuf.p + have, w->pendingMoves.data(), w->pendingMoves.size() * sizeof(int), hipMemcpyHostToDevice, w->stream));
	int total = have + (int)w->pendingMoves.size();
	HIP_TRY(hipMemcpyAsync(&w->d_state.p->c.nMoves, &total, sizeof(int), hipMemcpyHostToDevice, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	w->pendingMoves.clear();
	return 0;
}

// Scan lengths that live on the device: uploaded when they change, not every step.
static int uploadScanLengths(b2hip_world* w)
{
	const int consts[3] = { (int)w->bodies.size(), (int)(w->dw.gridMask + 1), (int)w->bodies.size() + 1 };
	if (consts[0] == w->constsUploaded[0] && consts[1] == w->constsUploaded[1] && w->consts.p == w->constsUploadedAt) return 0;
	HIP_TRY(hipMemcpyAsync(w->consts.p, consts, sizeof(int) * 2, hipMemcpyHostToDevice, w->stream));
	// [4]: scan length of the TOI adjacency (nBodies + 1 so that adjStart[nBodies] is the total)
	HIP_TRY(hipMemcpyAsync(w->consts.p + 4, &consts[2], sizeof(int), hipMemcpyHostToDevice, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	w->constsUploaded[0] = consts[0];
	w->constsUploaded[1] = consts[1];
	w->constsUploadedAt = w->consts.p;
	return 0;
}

// Upload bodies / fixtures / shapes / joints created or edited since the last step: the stages above, in this order.
static int flushEdits(b2hip_world* w)
{
	forestDrop(w); // (bodies, fixtures and joints may change under the forest)
	int rc = ensureCapacity(w, (size_t)w->lastContacts);
	if (!rc) rc = uploadDirtyBodies(w);
	if (!rc) rc = uploadSeedOrder(w);
	if (!rc) rc = uploadTables(w);
	if (!rc) refreshMouseMasses(w);
	if (!rc) rc = uploadJointEdits(w);
	if (!rc) rc = uploadJointAdjacency(w);
	// (a fixture was destroyed or a body switched off or on, and no fixture is new: with new ones uploadNewProxies rebuilds the lists)
	if (!rc && w->proxyListsStale && w->upFixtures == w->fixtures.size() && !w->fixtures.empty()) rc = uploadProxyLists(w);
	if (!rc) rc = uploadNewProxies(w);
	if (!rc) rc = uploadProxyEdits(w);
	if (!rc) rc = appendPendingMoves(w);
	if (!rc) rc = uploadScanLengths(w);
	return rc;
}

// Flags the contacts between the bodies of every joint created or destroyed since the last step for re-filtering
// (b2World.cpp:716-732, 833-845): one upload of the sorted pair keys, one launch. Called by the step and by the snapshot
// (so that a snapshot taken right after CreateJoint / DestroyJoint carries the flags).
static int applyPendingFilters(b2hip_world* w)
{
	if (w->pendingFilter.empty()) return 0;
	std::vector<unsigned long long> keys(w->pendingFilter.size());
	for (size_t k = 0; k < keys.size(); ++k)
	{
		const unsigned a = (unsigned)std::min(w->pendingFilter[k].first, w->pendingFilter[k].second);
		const unsigned b = (unsigned)std::max(w->pendingFilter[k].first, w->pendingFilter[k].second);
		keys[k] = ((unsigned long long)a << 32) | b;
	}
	std::sort(keys.begin(), keys.end());
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	int rc = w->filterPairs.ensure(keys.size(), w->stream, false, false);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(w->filterPairs.p, keys.data(), keys.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, w->stream));
	LAUNCH(w, k_flag_filter, gridFor(w->dw.capContacts), 256, w->dw, w->filterPairs.p, (int)keys.size());
	HIP_TRY(hipStreamSynchronize(w->stream)); // `keys` is pageable host memory
	w->pendingFilter.clear();
	w->refilterPending = true;
	return 0;
}

// Applies the queued contact-array ops (b2d_kernels_edit.h) in call order, then compacts the contact array if contacts
// were destroyed. Called by the step right after its counters are zeroed, and by whoever reads the contacts between steps.
static int downloadState(b2hip_world* w, int clearForces, bool skipRowsIfRedo = false);
static int startEarlyRows(b2hip_world* w);

// What follows the ops on the stream: the compaction of the contact array if contacts were destroyed, and the device state
// back. (The batched destruction and activation sets, b2hip_api_body_lifecycle.h, mark their contacts themselves and end here too.)
static int editOpsTail(b2hip_world* w, bool destroys, bool betweenSteps)
{
	DW& d = w->dw;
	int rc = 0;
	if (destroys)
	{
		LAUNCH(w, k_edit_keepflags, gridFor(d.capContacts), 256, d);
		deviceExclusiveScan<int>(w->stream, d.keepFlag, d.keepScan, d.scanTmp, w->scanCtx, &d.st->c.nContacts, d.capContacts);
		LAUNCH(w, k_compact_contacts, gridFor(d.capContacts), 256, d); // (its last workgroup switches the buffers)
		LAUNCH(w, k_edit_finish, 1, 1, d);
		if (betweenSteps)
		{
			// destroying a touching contact wakes its bodies (b2Contact::Destroy, b2Contact.cpp:105-111): the host rows are
			// read again from the device (every edit made so far has been uploaded by the caller)
			rc = downloadState(w, 0);
			if (rc) return rc;
			w->stateCount = w->bodies.size();
			++w->mirrorEpoch;
		}
	}
	rc = readState(w); // (also makes the staging vector reusable, and the state rows above readable)
	if (rc) return rc;
	w->contactsKnown = true; // (read back behind everything that was queued)
	w->lastContacts = w->h_dstate->c.nContacts;
	w->last.nContacts = w->lastContacts;
	return 0;
}

static int applyEditOps(b2hip_world* w, bool betweenSteps)
{
	forestDrop(w); // (destroyed contacts leave the array)
	if (w->editOps.empty()) return 0;
	bool destroys = false;
	for (size_t k = 0; k < w->editOps.size(); ++k) destroys = destroys || w->editOps[k].x == EDIT_DESTROY_BODY || w->editOps[k].x == EDIT_DESTROY_FIXTURE;
	int rc = w->d_editOps.ensure(w->editOps.size(), w->stream, false, false);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(w->d_editOps.p, w->editOps.data(), w->editOps.size() * sizeof(int2), hipMemcpyHostToDevice, w->stream));
	DW& d = w->dw;
	LAUNCH(w, k_apply_edits, 1, 1024, d, (const int2*)w->d_editOps.p, (int)w->editOps.size());
	rc = editOpsTail(w, destroys, betweenSteps);
	if (rc) return rc;
	w->editOps.clear();
	return 0;
}
