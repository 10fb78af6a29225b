// b2hip_api_body_writes.h - batched forces, impulses, velocity sets, teleports and sleep / wake sets between steps, and the
// state rows of a batch of bodies (include/b2hip.h, blocks F and H; kernels: b2d_kernels_body_writes.h).
//
// A write call has the effect of the single-body calls made for its entries in order (include/b2hip.h says which). It goes
// round their cost - markDirty -> pullBody, then eight rows per dirty body uploaded by the next flushEdits - by editing the
// device's rows in one launch. That makes the DEVICE the newer copy of the named bodies, and the host has caches that must not
// be believed over it:
//   pending host edits  go first: flushEdits and applyEditOps run before the launch, so an edit made before the batch lies
//                       underneath it, as in the loop of single calls.
//   h_state, the shadow the rows are marked pending (rowsPending): the next reader runs fetchRows, which covers every body the
//                       device holds - flushEdits has just uploaded the ones created since the last step, hence stateCount.
//                       Nothing is fetched by the call itself (a lazy world keeps its table on the device).
//   HostBody rows       a named body is marked as not pulled, whatever it was: the next markDirty reads its row again, so a
//                       single-body edit made after the batch starts from the batch's velocity, not from a stale one.
//   HostBody forces     are not in the row. A named body whose force row the batch wrote - or whose host copy holds forces of
//                       this step interval, which an un-pulled row's owner would take for stale - is marked forceDev: its
//                       next pull fetches b_force too (pullForce), and a single b2hip_apply_force adds to the device's sum.
//                       (The mark carries the step epoch: once an auto-clear world has stepped, the row is zero again and
//                       nothing is fetched.)
//   a static body's     awake flag is tested by setAwake on the host before anything is pulled: b2hip_set_awakes, the one
//   awake flag          batched call that can clear it, writes the host's copy of that bit as well.
//   forceOnDevice       is raised by b2hip_apply_forces: the end of the step has forces to clear.
//   fat AABBs, moves    of an uploaded fixture are the device's (currentFat reads them there): b2hip_set_transforms writes no
//                       HostFixture::fat and queues no pending move.
// The ids and records travel through the queries' pinned buffer with one copy; the call returns when the stream has drained
// (the pinned buffer is the next call's).

extern "C++"
{
// checked before the world is looked at: n, null pointers (the per-body contact calls' convention: an output always,
// inputs when there are entries)
static int bodyWritesArgs(const char* what, int n, const int32_t* bodies, const void* in, const void* out)
{
	if (n < 0 || n > B2HIP_QUERY_MAX) return setError(B2HIP_ERR_INVALID, std::string(what) + ": n must lie in [0, 2^24]");
	if (!out || (n > 0 && (!bodies || !in))) return setError(B2HIP_ERR_INVALID, std::string(what) + ": null input or output");
	return 0;
}

// pending host edits to the device: they lie underneath the batch
static int bodyWritesEdits(b2hip_world* w)
{
	int rc = flushEdits(w);
	if (!rc) rc = applyEditOps(w, true);
	return rc;
}

// the ids and `bytes` of records (null: none) through the pinned buffer - made at least `atLeast` bytes, what comes back
// through it - into bcIds / bwIn
static int bodyWritesStage(b2hip_world* w, int n, const int32_t* bodies, const void* records, size_t bytes, size_t atLeast)
{
	int rc = 0;
	hipStream_t s = w->stream;
	const size_t idBytes = (((size_t)n * sizeof(int32_t)) + 15) & ~(size_t)15; // (the records start 16-byte aligned)
	rc = n ? w->bcIds.ensure((size_t)n, s, false, false) : 0;
	if (!rc && bytes) rc = w->bwIn.ensure((bytes + sizeof(float4) - 1) / sizeof(float4), s, false, false);
	if (!rc) rc = queryPinned(w, std::max(idBytes + bytes, atLeast));
	if (rc) return rc;
	if (n) // (none: the records name their targets themselves - the motor edits of b2hip_api_joint_batch.h)
	{
		memcpy(w->qPinned, bodies, (size_t)n * sizeof(int32_t));
		HIP_TRY(hipMemcpyAsync(w->bcIds.p, w->qPinned, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
	}
	if (bytes)
	{
		memcpy((char*)w->qPinned + idBytes, records, bytes);
		HIP_TRY(hipMemcpyAsync(w->bwIn.p, (const char*)w->qPinned + idBytes, bytes, hipMemcpyHostToDevice, s));
	}
	return 0;
}

// edits to the device, then the ids and the records
static int bodyWritesBegin(b2hip_world* w, int n, const int32_t* bodies, const void* records, size_t bytes, size_t atLeast)
{
	if (int rc = bodyWritesEdits(w)) return rc;
	return bodyWritesStage(w, n, bodies, records, bytes, atLeast);
}

// behind the launch: the host's caches of the named bodies (the head of this file). forces: what the launch did to the named
// bodies' force rows - nothing, added to them (the end of the step has forces to clear), or zeroed some of them
enum { BODY_FORCES_NONE = 0, BODY_FORCES_ADDED = 1, BODY_FORCES_ZEROED = 2 };
static int bodyWritesMirror(b2hip_world* w, int n, const int32_t* bodies, int forces)
{
	HIP_TRY(hipStreamSynchronize(w->stream));
	w->stateCount = w->bodies.size(); // (what fetchRows will have covered: dw.nBodies, set by flushEdits just now)
	for (int i = 0; i < n; ++i)
	{
		HostBody& b = w->bodies[(size_t)bodies[i]];
		uint32_t bits[3];
		memcpy(bits, &b.fx, sizeof(bits)); // (fx, fy, torque lie side by side)
		const bool hostForces = b.forceEpoch == w->stepEpoch && (bits[0] | bits[1] | bits[2]) != 0u;
		if (forces != BODY_FORCES_NONE || hostForces)
		{
			if (b.forceDev == 0u) w->forceDevCount += 1;
			b.forceDev = w->stepEpoch;
		}
		b.pullEpoch = w->mirrorEpoch - 1u; // not pulled: h_state's row, once fetched, is the newer one
	}
	if (forces == BODY_FORCES_ADDED) w->forceOnDevice = true;
	w->rowsPending.store(true, std::memory_order_release);
	return B2HIP_OK;
}

template <int FAMILY>
static int bodyWrites(b2hip_world* w, const char* what, int n, const int32_t* bodies, const void* records, size_t recordBytes, int arg)
{
	if (int rc = bodyWritesArgs(what, n, bodies, records, what)) return rc; // (a write call has no output: any non-null pointer)
	if (FAMILY == BODY_WRITE_VELOCITIES && (arg < 1 || arg > 3)) return setError(B2HIP_ERR_INVALID, std::string(what) + ": mask must be 1, 2 or 3");
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = bodyContactsIds(w, what, n, bodies, true, true)) return rc;
	if (n == 0) return B2HIP_OK;
	if (int rc = bodyWritesBegin(w, n, bodies, records, (size_t)n * recordBytes, 0)) return rc;
	LAUNCH(w, k_body_write<FAMILY>, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, (const void*)w->bwIn.p, arg, w->dw.nBodies, w->b_flags.p,
	       w->b_pos.p, (const float4*)w->b_mass.p, w->b_vel.p, w->b_force.p);
	return bodyWritesMirror(w, n, bodies, FAMILY == BODY_WRITE_FORCES ? BODY_FORCES_ADDED : BODY_FORCES_NONE);
}
} // extern "C++"

int b2hip_apply_forces(b2hip_world* w, int n, const int32_t* bodies, const b2hip_body_push* push, int wake)
{
	return bodyWrites<BODY_WRITE_FORCES>(w, "b2hip_apply_forces", n, bodies, push, sizeof(b2hip_body_push), wake != 0);
}

int b2hip_apply_impulses(b2hip_world* w, int n, const int32_t* bodies, const b2hip_body_push* push, int wake)
{
	return bodyWrites<BODY_WRITE_IMPULSES>(w, "b2hip_apply_impulses", n, bodies, push, sizeof(b2hip_body_push), wake != 0);
}

int b2hip_set_velocities(b2hip_world* w, int n, const int32_t* bodies, const float* v3, int mask)
{
	return bodyWrites<BODY_WRITE_VELOCITIES>(w, "b2hip_set_velocities", n, bodies, v3, 3 * sizeof(float), mask);
}

// ---- block H: teleports and sleep / wake sets -------------------------------------------------------------------------------
// b2hip_set_transforms moves proxies, and every proxy that leaves its fat AABB takes a place in the move buffer, which holds
// 2 x proxies + 64 entries and is emptied by the step's pair update. Neither the reference nor the single route removes
// duplicates from buffered moves, so repeated teleports between two steps can fill it: the call is refused when the moves the
// device has buffered (its counter: four bytes fetched) plus every live proxy of the named bodies would not fit. Pending edits
// can buffer moves of their own, so they go to the device before the counter is read; the refusal comes before the batch's own
// ids and poses are staged.
int b2hip_set_transforms(b2hip_world* w, int n, const int32_t* bodies, const float* pose3, int mask)
{
	const char* what = "b2hip_set_transforms";
	if (int rc = bodyWritesArgs(what, n, bodies, pose3, what)) return rc; // (a write call has no output: any non-null pointer)
	if (mask < 1 || mask > 3) return setError(B2HIP_ERR_INVALID, std::string(what) + ": mask must be 1, 2 or 3");
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = bodyContactsIds(w, what, n, bodies, true, true)) return rc;
	if (n == 0) return B2HIP_OK;
	if (int rc = bodyWritesEdits(w)) return rc;
	size_t proxies = 0;
	for (int i = 0; i < n; ++i)
	{
		const HostBody& b = w->bodies[(size_t)bodies[i]];
		for (size_t k = 0; k < b.fixtures.size(); ++k)
		{
			const HostFixture& f = w->fixtures[(size_t)b.fixtures[k]];
			if (!f.dead && !f.noProxy) proxies += 1;
		}
	}
	int buffered = 0;
	HIP_TRY(hipMemcpyAsync(&buffered, &w->d_state.p->c.nMoves, sizeof(int), hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	if (buffered < 0 || (size_t)buffered + proxies > (size_t)w->dw.capMoves)
		return setError(B2HIP_ERR_UNSUPPORTED, std::string(what) + ": the move buffer holds " + std::to_string(buffered) + " of " + std::to_string(w->dw.capMoves) +
		                " entries and the batch can add " + std::to_string(proxies) + ": step the world first");
	if (int rc = bodyWritesStage(w, n, bodies, pose3, (size_t)n * 3 * sizeof(float), 0)) return rc;
	LAUNCH(w, k_set_transforms, gridFor((size_t)n), 256, w->dw, (const int*)w->bcIds.p, n, (const float*)w->bwIn.p, mask);
	return bodyWritesMirror(w, n, bodies, BODY_FORCES_NONE);
}

int b2hip_set_awakes(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* awake)
{
	const char* what = "b2hip_set_awakes";
	if (int rc = bodyWritesArgs(what, n, bodies, awake, what)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = bodyContactsIds(w, what, n, bodies, true, true)) return rc;
	if (n == 0) return B2HIP_OK;
	if (int rc = bodyWritesBegin(w, n, bodies, awake, (size_t)n, 0)) return rc;
	LAUNCH(w, k_set_awakes, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, (const uint8_t*)w->bwIn.p, w->dw.nBodies, w->b_flags.p, w->b_pos.p,
	       w->b_vel.p, w->b_force.p);
	// (SetAwake(false) zeroes the force row: the device's is the newer one, as behind b2hip_apply_forces, with nothing to clear)
	if (int rc = bodyWritesMirror(w, n, bodies, BODY_FORCES_ZEROED)) return rc;
	// setAwake tests a static body's awake flag on the host before it pulls anything (b2hip_host_world.h): the host's copy of
	// that one bit follows the batch, or a single b2hip_set_awake(w, ground, 1) after a batch that put the ground to sleep would
	// believe the stale flag and do nothing
	for (int i = 0; i < n; ++i)
	{
		HostBody& b = w->bodies[(size_t)bodies[i]];
		if (b.type != B2HIP_STATIC_BODY) continue;
		if (awake[i] != 0) b.flags |= BF_AWAKE;
		else b.flags &= ~(uint32_t)BF_AWAKE;
	}
	return B2HIP_OK;
}

int b2hip_get_body_states_of(b2hip_world* w, int n, const int32_t* bodies, b2hip_body_state* out)
{
	const char* what = "b2hip_get_body_states_of";
	if (int rc = bodyWritesArgs(what, n, bodies, bodies, out)) return rc;
	if (int rc = queryUsable(w, what)) return rc;
	DEVICE_GUARD(w);
	if (int rc = bodyContactsIds(w, what, n, bodies, true, false)) return rc;
	if (n == 0) return B2HIP_OK;
	int rc = bodyWritesBegin(w, n, bodies, nullptr, 0, (size_t)n * sizeof(b2hip_body_state));
	if (!rc) rc = w->bwRows.ensure(5 * (size_t)n, w->stream, false, false);
	if (rc) return rc;
	LAUNCH(w, k_body_rows, gridFor((size_t)n), 256, (const int*)w->bcIds.p, n, w->dw.nBodies, (const uint32_t*)w->b_flags.p, (const float4*)w->b_pos.p,
	       (const float4*)w->b_vel.p, (const float4*)w->b_xf.p, w->bwRows.p);
	if ((rc = bodyContactsOut(w, (const b2hip_body_state*)w->bwRows.p, n, out))) return rc;
	// (the type as b2hip_get_body_states reports it: the host's)
	for (int i = 0; i < n; ++i) out[i].flags = (out[i].flags & 0x7cu) | (uint32_t)w->bodies[(size_t)bodies[i]].type;
	return B2HIP_OK;
}
