// b2hip_api_world.h - part of the ONE translation unit b2hip.hip, inside its extern "C" block: the world itself in the C ABI of
// include/b2hip.h - create / destroy, gravity, flags, counts, b2hip_shift_origin - and what the mutators of its bodies,
// fixtures and joints share (b2hip_api_fixtures.h, b2hip_api_bodies.h, b2hip_api_joints.h).
// (No include guard on purpose: b2hip.hip includes it exactly once, in order - the fragments share one scope.)

// ---- what the mutators share: a usable world and a live id; a contact-array op queued for applyEditOps --------------------
static int checkBody(b2hip_world* w, int body, const char* what)
{
	if (int rcu = checkUsable(w, what, true)) return rcu;
	if (body < 0 || body >= (int)w->bodies.size() || w->bodies[body].dead) return setError(B2HIP_ERR_INVALID, std::string(what) + ": bad body id");
	return 0;
}

static int checkFixture(b2hip_world* w, int fixture, const char* what)
{
	if (int rcu = checkUsable(w, what, true)) return rcu;
	if (fixture < 0 || fixture >= (int)w->fixtures.size() || w->fixtures[fixture].dead) return setError(B2HIP_ERR_INVALID, std::string(what) + ": bad fixture id");
	return 0;
}

static void queueOp(b2hip_world* w, int kind, int id)
{
	w->editOps.push_back(make_int2(kind, id));
}

const char* b2hip_last_error(void)
{
	return g_lastError.c_str();
}

const char* b2hip_version(void)
{
	return "b2hip 0.1 (gfx950)";
}

int b2hip_world_create(const b2hip_world_def* def, b2hip_world** out)
{
	if (!def || !out) return setError(B2HIP_ERR_INVALID, "null argument");
	int count = 0;
	hipError_t e = hipGetDeviceCount(&count);
	if (e != hipSuccess || count <= 0)
	{
		return setError(B2HIP_ERR_NO_DEVICE, "no HIP device available: the b2hip Step() path has no CPU fallback");
	}
	int current = 0;
	if (hipGetDevice(&current) != hipSuccess) current = 0;
	const int device = def->device >= 0 ? def->device : current;
	if (device >= count) return setError(B2HIP_ERR_NO_DEVICE, "no such HIP device");
	b2hip_world* w = new b2hip_world();
	w->def = *def;
	w->device = device; // the ordinal itself, also when the caller asked for "current": later calls select it again
	DEVICE_GUARD(w);
	{
		int now = -1;
		if (hipGetDevice(&now) != hipSuccess || now != device)
		{
			delete w;
			return setError(B2HIP_ERR_NO_DEVICE, "hipSetDevice failed");
		}
	}
	e = hipStreamCreateWithFlags(&w->stream2, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&w->evFork, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&w->evJoin, hipEventDisableTiming);
	if (e == hipSuccess) e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
	if (e != hipSuccess)
	{
		delete w;
		return setError(B2HIP_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
	}
	readSwitches(w);
	{
		// how many workgroups of the solvers whose workgroups wait for one another are resident together on this device
		hipDeviceProp_t prop;
		int devId = 0;
		if (hipGetDevice(&devId) == hipSuccess && hipGetDeviceProperties(&prop, devId) == hipSuccess)
		{
			int perCU = 0, perCU2 = 0, perCU3 = 0;
			if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, k_solve_blocks<256>, 256, 0) == hipSuccess &&
				hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU2, k_solve_blocks<512>, 512, 0) == hipSuccess &&
				hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU3, k_solve_blocks<BLOCK_LANES>, BLOCK_LANES, 0) == hipSuccess &&
				perCU > 0 && perCU2 > 0 && perCU3 > 0)
			{
				// one block per CU is all this sizing relies on (the occupancy query can be one too high, MI355X_MICROARCH.md)
				w->blocksMaxWG = prop.multiProcessorCount - 8;
				int s0 = 0, s1 = 0, s2 = 0;
				if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&s0, k_blocks_sweep<256>, 256, 0) == hipSuccess &&
					hipOccupancyMaxActiveBlocksPerMultiprocessor(&s1, k_blocks_sweep<512>, 512, 0) == hipSuccess &&
					hipOccupancyMaxActiveBlocksPerMultiprocessor(&s2, k_blocks_sweep<BLOCK_LANES>, BLOCK_LANES, 0) == hipSuccess)
				{
					// (the blocks of a launch wait for one another: all of them must be resident together)
					w->sweepMaxWG[0] = std::max(1, s0 - 1) * w->blocksMaxWG;
					w->sweepMaxWG[1] = std::max(1, s1 - 1) * w->blocksMaxWG;
					w->sweepMaxWG[2] = std::max(1, s2 - 1) * w->blocksMaxWG;
				}
			}
			// the workgroups of k_large_rest / k_rest_hub wait for one another's rows: all of a launch must be resident together
			// (the grid was sized from the colour census alone)
			int r1 = 0, r2 = 0, f1 = 0, f2 = 0;
			const int cus = std::max(1, prop.multiProcessorCount - 8);
			if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&r1, k_large_rest<1>, 256, 0) == hipSuccess &&
				hipOccupancyMaxActiveBlocksPerMultiprocessor(&r2, k_large_rest<2>, 256, 0) == hipSuccess && r1 > 0 && r2 > 0)
				w->restMaxWG = std::min(r1, r2) * cus;
			if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&f1, k_rest_hub<1>, SWEEP_END_LANES, 0) == hipSuccess &&
				hipOccupancyMaxActiveBlocksPerMultiprocessor(&f2, k_rest_hub<2>, SWEEP_END_LANES, 0) == hipSuccess && f1 > 0 && f2 > 0)
				w->restHubMaxWG = std::min(f1, f2) * cus;
		}
	}
	int rc = 0;
	for (int i = 0; i < 13 && !rc; ++i)
		if (hipEventCreate(&w->ev[i]) != hipSuccess) rc = setError(B2HIP_ERR_HIP, "hipEventCreate failed");
	// (h_pub, h_pub2, h_solverWord: written by a kernel, polled by the host - mapped and coherent)
	if (!rc) rc = w->h_dstate.alloc(1, hipHostMallocDefault);
	if (!rc) rc = w->h_pub.alloc(1, hipHostMallocMapped | hipHostMallocCoherent);
	if (!rc) rc = w->h_pub2.alloc(1, hipHostMallocMapped | hipHostMallocCoherent);
	if (!rc) rc = w->h_solverWord.alloc(16, hipHostMallocMapped | hipHostMallocCoherent);
	if (!rc)
	{
		memset(w->h_pub, 0, sizeof(DState));
		memset(w->h_pub2, 0, sizeof(DState));
		memset(w->h_solverWord, 0, 16 * sizeof(int));
		rc = ensureCapacity(w, 0);
	}
	if (rc == 0 && hipStreamSynchronize(w->stream) != hipSuccess) rc = setError(B2HIP_ERR_HIP, "stream sync failed");
	if (rc)
	{
		const std::string why = g_lastError;
		b2hip_world_destroy(w);
		return setError(rc, why);
	}
	*out = w;
	return B2HIP_OK;
}

void b2hip_world_destroy(b2hip_world* w)
{
	if (!w) return;
	DEVICE_GUARD(w);
	if (w->stream) (void)hipStreamSynchronize(w->stream);
	if (w->rowStream)
	{
		(void)hipStreamSynchronize(w->rowStream);
		(void)hipStreamDestroy(w->rowStream);
		(void)hipEventDestroy(w->rowFork);
		(void)hipEventDestroy(w->rowJoin);
		w->rowStream = nullptr;
	}
	if (w->shardComm != nullptr && g_rcclDestroy != nullptr) g_rcclDestroy(w->shardComm);
	w->shardComm = nullptr;
	for (size_t k = 0; k < w->spTape.size(); ++k) (void)hipFree(w->spTape[k].first);
	w->spTape.clear();
	if (w->qPinned) (void)hipHostFree(w->qPinned);
	for (int i = 0; i < 13; ++i)
		if (w->ev[i]) (void)hipEventDestroy(w->ev[i]);
	for (size_t i = 0; i < w->ktEvents.size(); ++i) (void)hipEventDestroy(w->ktEvents[i]);
	if (w->stream) (void)hipStreamDestroy(w->stream);
	if (w->stream2) (void)hipStreamDestroy(w->stream2);
	if (w->evFork) (void)hipEventDestroy(w->evFork);
	if (w->evJoin) (void)hipEventDestroy(w->evJoin);
	delete w; // (frees the device arrays and the pinned buffers, with the world's device still current)
}

int b2hip_set_gravity(b2hip_world* w, float gx, float gy)
{
	if (int rcu = checkUsable(w, "b2hip_set_gravity", true)) return rcu;
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	w->def.gravity_x = gx;
	w->def.gravity_y = gy;
	return 0;
}

int b2hip_set_flags(b2hip_world* w, int allow_sleep, int warm_starting, int continuous, int sub_stepping)
{
	if (int rcu = checkUsable(w, "b2hip_set_flags", true)) return rcu;
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	w->def.allow_sleep = allow_sleep;
	w->def.warm_starting = warm_starting;
	w->def.continuous = continuous;
	w->def.sub_stepping = sub_stepping;
	return 0;
}

int b2hip_body_count(const b2hip_world* w)
{
	return w ? (int)w->bodies.size() : 0;
}

int b2hip_fixture_count(const b2hip_world* w)
{
	return w ? (int)w->fixtures.size() : 0;
}

// b2World::ShiftOrigin (b2World.cpp:1862-1887)
int b2hip_shift_origin(b2hip_world* w, float x, float y)
{
	if (int rcu = checkUsable(w, "b2hip_shift_origin", true)) return rcu;
	if (w->stepActive) return setError(B2HIP_ERR_INVALID, "b2hip_shift_origin inside a step");
	DEVICE_GUARD(w);
	// every edit made so far goes to the device first: from here on the device state is the one that is shifted
	int rc = flushEdits(w);
	if (rc) return rc;
	rc = applyEditOps(w, true);
	if (rc) return rc;
	const int n = std::max(std::max(w->dw.nBodies, w->dw.nProxies), std::max(w->dw.nJoints, 1));
	LAUNCH(w, k_shift_origin, gridFor(n), 256, w->dw, x, y);
	// the host's copies: joint records (uploaded again when a setter edits them), fat AABBs, and the body rows - read back
	for (size_t j = 0; j < w->joints.size(); ++j)
	{
		JointRec& jn = w->joints[j];
		if (jn.type == B2D_JOINT_MOUSE) { jn.targetA.x -= x; jn.targetA.y -= y; }
		else if (jn.type == B2D_JOINT_PULLEY) { jn.groundAnchorA.x -= x; jn.groundAnchorA.y -= y; jn.s1 -= x; jn.s2 -= y; }
	}
	for (size_t f = 0; f < w->fixtures.size(); ++f)
	{
		w->fixtures[f].fat[0] -= x; w->fixtures[f].fat[1] -= y;
		w->fixtures[f].fat[2] -= x; w->fixtures[f].fat[3] -= y;
	}
	rc = downloadState(w, 0);
	if (rc) return rc;
	w->stateCount = w->bodies.size();
	++w->mirrorEpoch;
	return B2HIP_OK;
}

