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
	w->nextNode = 0;
	w->leafCount = 0;
	w->upBodies = w->upFixtures = w->upShapes = w->upJoints = 0;
	w->stateCount = 0;
	w->mirrorEpoch = 1;
	w->stepEpoch = 1;
	w->newFixture = false;
	w->inv_dt0 = 0.0f;
	w->stepActive = false;
	w->callbackWindow = false;
	w->h_state = nullptr;
	w->h_stateCap = 0;
	w->lastContacts = 0;
	memset(&w->last, 0, sizeof(w->last));
	memset(&w->dw, 0, sizeof(w->dw));
	memset(w->profile, 0, sizeof(w->profile));
	w->solverMs = 0.0f;
	w->solverBytes = 0.0;
	w->solverConstraints = w->solverBodies = 0;
	w->kernelTiming = 0;
	w->ktUnitsA = w->ktUnitsB = 0;
	w->ktUsed = 0;
	w->ktKind = 0;
	w->ktMs = 0.0f;
	w->ktLaunches = 0;
	w->ktBytes = 0.0;
	w->dw.cellSize = 1.0f;
	w->dw.invCellSize = 1.0f;
	w->colorSmallPending = false;
	w->hubSteps = 0;
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
	w->dfEpoch = 0;
	for (int i = 0; i < 13; ++i) w->ev[i] = nullptr;
	w->h_dstate = nullptr;
	for (int i = 0; i < 13; ++i)
	{
		if (hipEventCreate(&w->ev[i]) != hipSuccess)
		{
			b2hip_world_destroy(w);
			return setError(B2HIP_ERR_HIP, "hipEventCreate failed");
		}
	}
	if (hipHostMalloc((void**)&w->h_dstate, sizeof(DState), hipHostMallocDefault) != hipSuccess)
	{
		b2hip_world_destroy(w);
		return setError(B2HIP_ERR_HIP, "hipHostMalloc failed");
	}
	// (written by a kernel, polled by the host: mapped and coherent)
	if (hipHostMalloc((void**)&w->h_pub, sizeof(DState), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
		hipHostGetDevicePointer((void**)&w->d_pub, w->h_pub, 0) != hipSuccess)
	{
		b2hip_world_destroy(w);
		return setError(B2HIP_ERR_HIP, "hipHostMalloc (coherent) failed");
	}
	memset(w->h_pub, 0, sizeof(DState));
	if (hipHostMalloc((void**)&w->h_pub2, sizeof(DState), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
		hipHostGetDevicePointer((void**)&w->d_pub2, w->h_pub2, 0) != hipSuccess)
	{
		b2hip_world_destroy(w);
		return setError(B2HIP_ERR_HIP, "hipHostMalloc (coherent) failed");
	}
	memset(w->h_pub2, 0, sizeof(DState));
	if (hipHostMalloc((void**)&w->h_solverWord, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
		hipHostGetDevicePointer((void**)&w->d_solverWord, w->h_solverWord, 0) != hipSuccess)
	{
		b2hip_world_destroy(w);
		return setError(B2HIP_ERR_HIP, "hipHostMalloc (coherent) failed");
	}
	memset(w->h_solverWord, 0, 64);
	int rc = ensureCapacity(w, 0);
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
	w->shardSend.release(); w->shardRecv.release();
	w->b_owner.release(); w->spNewOwner.release(); w->spAwake.release(); w->spStraddle.release(); w->spCount.release(); w->spTarget.release();
	w->spSend.release(); w->spRecv.release(); w->spTailKey.release(); w->spVirt.release();
	if (w->spHost) (void)hipHostFree(w->spHost);
	w->spHost = nullptr;
	if (w->spOwnHost) (void)hipHostFree(w->spOwnHost);
	w->spOwnHost = nullptr;
	if (w->spHdrHost) (void)hipHostFree(w->spHdrHost);
	w->spHdrHost = nullptr;
	for (size_t k = 0; k < w->spTape.size(); ++k) (void)hipFree(w->spTape[k].first);
	w->spTape.clear();
	w->d_state.release();
	w->b_pos.release(); w->b_pos0.release(); w->b_vel.release(); w->b_xf.release(); w->b_mass.release(); w->b_damp.release();
	w->b_force.release(); w->b_flags.release(); w->b_wake.release(); w->b_rowDirty.release();
	w->p_fat.release(); w->p_body.release(); w->p_shape.release(); w->p_key.release(); w->p_filter0.release(); w->p_filter1.release();
	w->p_mat.release(); w->d_shapes.release();
	for (int k = 0; k < 2; ++k)
	{
		w->c_ids[k].release(); w->c_key[k].release(); w->c_flags[k].release(); w->c_mat[k].release(); w->c_man0[k].release();
		w->c_man1[k].release(); w->c_imp[k].release(); w->c_man3[k].release(); w->c_color[k].release();
	}
	w->ht_keys.release(); w->d_joints.release(); w->d_gears.release(); w->li_ref.release();
	w->jadjStart.release(); w->jadj.release(); w->rootJointStart.release(); w->rootJointCursor.release();
	w->lj_list.release(); w->rootJointOkay.release();
	w->parent.release(); w->rootSeed.release(); w->rootBodies.release(); w->rootContacts.release(); w->rootJoints.release();
	w->rootIsland.release(); w->deg.release(); w->adjStart.release(); w->adjCursor.release(); w->adj.release(); w->adjSlot.release();
	w->rootScanIn.release(); w->rootScanOut.release();
	w->si_root.release(); w->si_bodyStart.release(); w->si_contactStart.release(); w->si_wStart.release(); w->si_maxLevel.release();
	w->si_bodies.release(); w->si_contacts.release(); w->si_level.release(); w->si_stack.release(); w->si_lastLevel.release();
	w->b_slot.release(); w->b_island.release(); w->chunkFirst.release();
	w->li_bodies.release(); w->li_contacts.release(); w->li_roots.release(); w->li_color.release(); w->colorCount.release();
	w->colorStart.release(); w->colorCursor.release(); w->li_sorted.release(); w->bodyClaim.release(); w->rootPen.release();
	w->bodyActive.release(); w->bodyRest.release(); w->b_posv.release(); w->evKey.release(); w->evInfo.release(); w->uncolList.release(); w->compactList.release(); w->gridBar.release(); w->hubRowOf.release(); w->hubList.release(); w->hubDelta.release(); w->hubMeta.release(); w->hubFirst.release(); w->solveSnapBody.release(); w->solveSnapImp.release(); w->solveSnapCFlags.release(); w->solveSnapJoints.release(); w->solveSnapGears.release();
	w->b_proxyHead.release(); w->p_next.release(); w->toiList.release(); w->toiPos2c.release(); w->toiDestroyList.release(); w->toiNewList.release(); w->collideCounts.release(); w->collideGroups.release();
	w->b_toiGroup.release(); w->toiGroups.release(); w->toiGroupCount.release(); w->toiGroupList.release(); w->toiMoved.release(); w->toiNew.release(); w->toiParent.release(); w->toiDomOf.release(); w->toiDomRoot.release(); w->toiDomCount.release(); w->toiDomBase.release(); w->toiDomFill.release(); w->toiDomFailed.release(); w->toiDomEvents.release(); w->toiDomList.release(); w->toiHull.release(); w->snapBody.release(); w->snapFat.release();
	w->c_mgr[0].release(); w->c_mgr[1].release(); w->dbgPreVel.release(); w->dbgVel.release(); w->dbgLi.release();
	w->rootSleepMin.release(); w->bodyColorMask.release(); w->rootDone.release(); w->lc.release(); w->warmDelta.release();
	w->moveBuf.release(); w->gridCount.release(); w->gridStart.release(); w->gridCursor.release(); w->gridItems.release(); w->gridFat.release(); w->arriveTree.release();
	w->largeProxies.release(); w->largeMoves.release(); w->pairKey.release(); w->pairKey2.release(); w->pairProxy.release(); w->pairProxy2.release();
	w->filterPairs.release();
	w->d_editOps.release();
	w->b_order.release(); w->orderBody.release(); w->bigRoots.release();
	w->pre_o0.release(); w->pre_o1.release(); w->pre_oimp.release(); w->pre_o3.release(); w->preRecs.release();
	w->postRecs.release(); w->filterList.release(); w->hostList.release(); w->toiLog.release(); w->toiVerdict.release();
	w->b_blk1.release(); w->b_adopt.release(); w->b_adoptStage.release(); w->blkRows.release(); w->blkRowStart.release(); w->blkCursor.release(); w->blkBodyCount.release(); w->blkBodyCursor.release();
	w->blkBodyStart.release(); w->blkBodies.release(); w->rowColor.release(); w->b_cutv.release();
	w->pairFirst.release(); w->pairRank.release(); w->scanTmp.release(); w->radixHist.release(); w->radixHistScan.release();
	w->keepFlag.release(); w->keepScan.release(); w->scanTmp4.release(); w->scanFlags.release(); w->radixCounts.release(); w->radixGroups.release(); w->radixGlobalHist.release(); w->stateOut.release(); w->consts.release();
	w->qIn.release(); w->qCounts.release(); w->qOffsets.release(); w->qItems.release(); w->qFlags.release(); w->qScanWork.release();
	w->qScanWords.release(); w->qWords.release(); w->qHits.release(); w->qDistances.release(); w->qPoses.release(); w->qShapes.release();
	w->qKeys.release(); w->qKeysWork.release(); w->qAny.release();
	w->bcSlot.release(); w->bcIds.release(); w->bcCounts.release(); w->bcRecords.release(); w->bcTotals.release();
	w->bwIn.release(); w->bwRows.release(); w->jbOut.release(); w->lcNamed.release(); w->lcWords.release(); w->fxNamed.release();
	if (w->qPinned) (void)hipHostFree(w->qPinned);
	if (w->h_state) (void)hipHostFree(w->h_state);
	if (w->h_dstate) (void)hipHostFree(w->h_dstate);
	if (w->h_pub) (void)hipHostFree(w->h_pub);
	if (w->h_pub2) (void)hipHostFree(w->h_pub2);
	if (w->h_solverWord) (void)hipHostFree(w->h_solverWord);
	for (int i = 0; i < 13; ++i)
		if (w->ev[i]) (void)hipEventDestroy(w->ev[i]);
	for (size_t i = 0; i < w->ktEvents.size(); ++i) (void)hipEventDestroy(w->ktEvents[i]);
	if (w->stream) (void)hipStreamDestroy(w->stream);
	if (w->stream2) (void)hipStreamDestroy(w->stream2);
	if (w->evFork) (void)hipEventDestroy(w->evFork);
	if (w->evJoin) (void)hipEventDestroy(w->evJoin);
	delete w;
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

