// b2hip_api_callbacks.h - part of the ONE translation unit b2hip.hip, inside its extern "C" block: listener / filter callbacks,
// island labels, fat AABBs, debug reads, profile, counters and the kernel-timing hooks bench.py uses.
// (No include guard on purpose: b2hip.hip includes it exactly once, in order - the fragments share one scope.)

int b2hip_set_contact_filter(b2hip_world* w, b2hip_should_collide_fn fn, void* user)
{
	if (int rcu = checkUsable(w, "b2hip_set_contact_filter", true)) return rcu;
	w->filterFn = fn;
	w->filterUser = user;
	w->dw.userFilter = hasFilter(w) ? 1 : 0;
	return B2HIP_OK;
}

int b2hip_set_contact_filter_batch(b2hip_world* w, b2hip_should_collide_batch_fn fn, void* user)
{
	if (int rcu = checkUsable(w, "b2hip_set_contact_filter_batch", true)) return rcu;
	w->filterBatchFn = fn;
	if (fn) w->filterUser = user;
	w->dw.userFilter = hasFilter(w) ? 1 : 0;
	return B2HIP_OK;
}

int b2hip_default_should_collide(b2hip_world* w, int fixture_a, int fixture_b)
{
	if (!w || fixture_a < 0 || fixture_b < 0 || fixture_a >= (int)w->fixtures.size() || fixture_b >= (int)w->fixtures.size())
		return setError(B2HIP_ERR_INVALID, "bad fixture id");
	// b2ContactFilter::ShouldCollide (b2WorldCallbacks.cpp:24-38)
	const HostFixture& a = w->fixtures[fixture_a];
	const HostFixture& b = w->fixtures[fixture_b];
	if (a.groupIndex == b.groupIndex && a.groupIndex != 0) return a.groupIndex > 0 ? 1 : 0;
	return ((a.maskBits & b.categoryBits) != 0 && (a.categoryBits & b.maskBits) != 0) ? 1 : 0;
}

int b2hip_set_pre_solve(b2hip_world* w, b2hip_pre_solve_fn fn, void* user)
{
	if (int rcu = checkUsable(w, "b2hip_set_pre_solve", true)) return rcu;
	w->preSolveFn = fn;
	w->preSolveUser = user;
	w->dw.preSolveOn = hasPreSolve(w) ? 1 : 0;
	return B2HIP_OK;
}

int b2hip_set_pre_solve_batch(b2hip_world* w, b2hip_pre_solve_batch_fn fn, void* user)
{
	if (int rcu = checkUsable(w, "b2hip_set_pre_solve_batch", true)) return rcu;
	w->preSolveBatchFn = fn;
	if (fn) w->preSolveUser = user;
	w->dw.preSolveOn = hasPreSolve(w) ? 1 : 0;
	return B2HIP_OK;
}

int b2hip_enable_post_solve(b2hip_world* w, int enable)
{
	if (int rcu = checkUsable(w, "b2hip_enable_post_solve", true)) return rcu;
	w->postSolveOn = enable != 0;
	w->dw.postSolveOn = enable ? 1 : 0;
	w->postSolve.clear();
	return B2HIP_OK;
}

int b2hip_get_post_solve(b2hip_world* w, int cap, b2hip_contact_impulse* out)
{
	if (!w || (cap > 0 && !out)) return setError(B2HIP_ERR_INVALID, "null argument");
	const int n = (int)w->postSolve.size();
	for (int i = 0; i < n && i < cap; ++i) out[i] = w->postSolve[i];
	return n;
}

int b2hip_get_island_labels(b2hip_world* w, int cap, int32_t* out)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	DEVICE_GUARD(w);
	if (!w || !out) return setError(B2HIP_ERR_INVALID, "null argument");
	const int n = std::min(cap, (int)w->bodies.size());
	if (n <= 0) return 0;
	std::vector<int> parent(n), tier(n);
	HIP_TRY(hipMemcpy(parent.data(), w->parent.p, n * sizeof(int), hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(tier.data(), w->rootIsland.p, n * sizeof(int), hipMemcpyDeviceToHost));
	for (int i = 0; i < n; ++i)
	{
		const HostBody& b = w->bodies[i];
		if (b.type == B2HIP_STATIC_BODY) { out[i] = -1; continue; }
		int r = parent[i];
		out[i] = (r >= 0 && r < n && tier[r] != ROOT_NONE) ? r : -1;
	}
	return n;
}

int b2hip_get_fat_aabb(b2hip_world* w, int fixture, float out4[4])
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	DEVICE_GUARD(w);
	if (!w || !out4 || fixture < 0 || fixture >= (int)w->fixtures.size()) return setError(B2HIP_ERR_INVALID, "bad fixture id");
	if ((size_t)fixture >= w->upFixtures)
	{
		memcpy(out4, w->fixtures[fixture].fat, 16);
		return 0;
	}
	HIP_TRY(hipMemcpy(out4, w->p_fat.p + fixture, 16, hipMemcpyDeviceToHost));
	return 0;
}

int b2hip_get_fat_aabbs(b2hip_world* w, int first, int count, float* out4n)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	DEVICE_GUARD(w);
	if (!w || (count > 0 && !out4n) || first < 0 || count < 0 || (size_t)(first + count) > w->fixtures.size())
		return setError(B2HIP_ERR_INVALID, "bad fixture range");
	const int onDevice = std::max(0, std::min(first + count, (int)w->upFixtures) - first);
	if (onDevice > 0) HIP_TRY(hipMemcpy(out4n, w->p_fat.p + first, (size_t)onDevice * 16, hipMemcpyDeviceToHost));
	for (int i = onDevice; i < count; ++i) memcpy(out4n + 4 * (size_t)i, w->fixtures[first + i].fat, 16); // not uploaded yet
	return 0;
}

// Debug / test hook: FNV-1a over a group of device arrays, read back after a stream sync. Valid between
// phase calls (b2hip_collide ... b2hip_step_end), so two worlds can be compared phase by phase.
//   which 0: bodies (pos, pos0, vel, xf, flags)   1: contacts (ids, key, flags & 0x7f, manifold, impulses)
//         2: proxies (fat AABBs)                  3: contact impulses only
static uint64_t fnv(uint64_t h, const void* data, size_t n)
{
	const unsigned char* p = (const unsigned char*)data;
	for (size_t i = 0; i < n; ++i)
	{
		h ^= p[i];
		h *= 1099511628211ull;
	}
	return h;
}

int b2hip_debug_hash(b2hip_world* w, int which, uint64_t* out)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	DEVICE_GUARD(w);
	if (!w || !out) return setError(B2HIP_ERR_INVALID, "null argument");
	HIP_TRY(hipStreamSynchronize(w->stream));
	DState st;
	HIP_TRY(hipMemcpy(&st, w->d_state.p, sizeof(DState), hipMemcpyDeviceToHost));
	uint64_t h = 1469598103934665603ull;
	std::vector<unsigned char> buf;
	auto pull = [&](const void* dev, size_t bytes) -> int
	{
		buf.resize(bytes);
		if (bytes == 0) return 0;
		if (hipMemcpy(buf.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 1;
		h = fnv(h, buf.data(), bytes);
		return 0;
	};
	const size_t nb = w->upBodies, np = w->upFixtures, nc = (size_t)st.c.nContacts;
	const int cur = st.cur;
	int bad = 0;
	if (which == 0)
	{
		bad |= pull(w->b_pos.p, nb * 16); bad |= pull(w->b_pos0.p, nb * 16); bad |= pull(w->b_vel.p, nb * 16);
		bad |= pull(w->b_xf.p, nb * 16);
		std::vector<uint32_t> f(nb);
		if (nb && hipMemcpy(f.data(), w->b_flags.p, nb * 4, hipMemcpyDeviceToHost) != hipSuccess) bad = 1;
		for (size_t i = 0; i < nb; ++i) f[i] &= 0x7fu;
		h = fnv(h, f.data(), nb * 4);
	}
	else if (which == 1)
	{
		bad |= pull(w->c_ids[cur].p, nc * 16); bad |= pull(w->c_key[cur].p, nc * 8);
		std::vector<uint32_t> f(nc);
		if (nc && hipMemcpy(f.data(), w->c_flags[cur].p, nc * 4, hipMemcpyDeviceToHost) != hipSuccess) bad = 1;
		for (size_t i = 0; i < nc; ++i) f[i] &= 0x1fu;
		h = fnv(h, f.data(), nc * 4);
		bad |= pull(w->c_man0[cur].p, nc * 16); bad |= pull(w->c_man1[cur].p, nc * 16);
		bad |= pull(w->c_imp[cur].p, nc * 16); bad |= pull(w->c_man3[cur].p, nc * 16);
	}
	else if (which == 2)
	{
		bad |= pull(w->p_fat.p, np * 16);
	}
	else
	{
		bad |= pull(w->c_imp[cur].p, nc * 16);
	}
	if (bad) return setError(B2HIP_ERR_HIP, "debug hash read-back failed");
	*out = h;
	return 0;
}

// Debug hook: raw read of a device array (0 b_pos, 1 b_vel, 2 li_bodies, 3 b_force, 4 b_flags, 5 b_damp, 6 b_mass,
// 7 counters as ints) into `out` (bytes).
// 22: pair-update statistics since the world was created, `count` (<= 2) long longs from `first`: [0] radix sorts queued,
//     [1] of them in the one-launch form (b2d_scan.h: k_radix_prepare + one k_radix_onepass per pass).
// 23: the kept contact-key set since the world was created, `count` (<= 12) long longs from `first`: [0] pair updates that
//     kept the set, [1 .. 6] rebuilds because the set was invalid / stale / built under another mask / too full / the world
//     is sharded / B2HIP_KEYSET_KEEP=0, [7] tombstones written, [8] keys inserted into a kept set, [9] deletes that found no
//     key, [10] slots in use now (live + tombstones), [11] the mask now.
// 24: one long long: narrow phases since the world was created in which k_collide<0, false, true> stored the compacted contact
//     array itself (no scan of the keep flags, no k_compact_contacts behind it).
// 25: the host side of SolveTOI since the world was created (ToiStats), `count` (<= 10) long longs from `first`. Runs of the
//     phase that had impacts pending, by path: [0] chains queued without the first pass's census, [1] chains after it,
//     [2] components queued without it, [3] components after it, [4] the serial loop chosen from it (second runs count under
//     [1], [3], [4] again). Rungs of the fall-back ladder: [5] redo behind a late pair sort, [6] chains again with the hash grid,
//     [7] serial replay (toi_serial_fallbacks), [8] re-run after a full contact array, [9] PreSolve re-run (toi_pre_solve_reruns).
// 12 - 21, 26 - 28: the plan of the large-island solve, read by tests/plan_ref.py (its docstring says from which launch to which
//     each array holds the step's plan). 12 the colour census (ints, [0, 65)), 13 bodyColorMask, 14 deg, 15 hubList, 16 bodyActive,
//     17 b_blk1, 18 li_ref (int4 per row), 19 rowColor, 20 blkRowStart, 21 bodyRest: raw device arrays, `count` elements from `first`.
// 26: the effective block (+ 1, 0 = none) of `count` bodies from `first`, ints: what effBlk (b2d_kernels_island.h) returns,
//     evaluated on the host from copies of b_blk1, b_adopt, b_flags and the device's counters. Launches nothing.
// 27: the last pass of the large-island solve as the host planned it (LargePass, b2hip_host_phases.h) and the counters that
//     belong to it, `count` (<= 28) ints from `first`: [0] passes run since the world was created, [1] solver (0 a launch per
//     colour, 1 k_solve_blocks, 2 k_blocks_sweep, 3 exact order, -1 none yet), [2] the safe pass behind a recovery, [3] restFirst
//     (0x7fffffff: no rest colours), [4] tailFirst, [5] bigEnd, [6] useRest, [7] fuseHub, [8] blockSort, [9] hubWide,
//     [10] serialOrphans, [11] colours the pass sweeps, [12] hasHubs, [13] hasJoints, [14] hub list by k_hub_build, [15] sweeps
//     end in k_sweep_end / k_rest_hub, [16] leftover hub rows go to k_large_hub; from the device's counters as they stand now:
//     [17] nHubRows, [18] nHubWide, [19] the primary hub's body id (hubMeta[0]; -1: no hub), [20] its degree, [21] nBlocks,
//     [22] nColors, [23] maxDegree; switches: [24] B2HIP_FORCE_LARGE, [25] smallMaxW, [26] B2HIP_TEST_MAX_COLORS, [27] joints
//     created so far (destroyed ones included: the range of id 28).
// 28: the bodies of `count` joints from `first`, four ints each: bodyA, bodyB (-1, -1: destroyed), a gear joint's bodyC, bodyD
//     (else -1, -1). From the host's mirror.
// 29: one long long: batched destroy / set-active calls since the world was created whose list of contacts with a TOI slot went
//     through the radix sort (longer than the one-workgroup sort takes; B2HIP_TEST_LIFECYCLE_SORT_MAX lowers that).
// 30: two long longs: batched b2hip_fixture_set_sensors / _thicks calls since the world was created [0] whose list of contacts
//     with a changed TOI candidacy went through the radix sort (the same threshold and hook), [1] that listed a second time
//     because the first listing's room was short (B2HIP_TEST_FIXTURE_LIST_ROOM lowers that room).
// 31: one long long: island builds since the world was created that ran no union pass over the contacts, because the step's
//     narrow phase - k_collide<0, false, true, true> - had united them (B2HIP_COLLIDE_UNION=0: never).
// 32: one long long: b2hip_set_types batches since the world was created that ran as the loop of single calls, because a proxy
//     of a body that turns static had left its fat AABB (include/b2hip.h, block K: believed unreachable). The batched
//     b2hip_set_bullets calls count their long sorts and second listings in 30.
int b2hip_debug_read(b2hip_world* w, int which, int first, int count, void* out)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	DEVICE_GUARD(w);
	if (!w || !out) return setError(B2HIP_ERR_INVALID, "null argument");
	HIP_TRY(hipStreamSynchronize(w->stream));
	const void* src = nullptr;
	size_t elem = 16;
	switch (which)
	{
	case 0: src = w->b_pos.p; break;
	case 1: src = w->b_vel.p; break;
	case 2: src = w->li_bodies.p; elem = 4; break;
	case 3: src = w->b_force.p; break;
	case 4: src = w->b_flags.p; elem = 4; break;
	case 5: src = w->b_damp.p; break;
	case 6: src = w->b_mass.p; break;
	case 7: src = w->d_state.p; elem = 4; break;
	case 8: src = w->dbgPreVel.p; break;
	case 9: src = w->dbgVel.p; break;
	case 10: src = w->dbgLi.p; elem = 4; break;
	case 11: src = w->gridBar.p; elem = 4; break;
	case 12:
	{
		// (the colour census: counter c at colorSlot(c) - the first 65 a 128-byte line apart)
		if (first < 0 || count < 0 || first + count > COLOR_SLOT_PADDED) return setError(B2HIP_ERR_INVALID, "colour census: [0, 65)");
		HIP_TRY(hipStreamSynchronize(w->stream));
		if (count > 0) HIP_TRY(hipMemcpy2D(out, sizeof(int), w->colorCount.p + colorSlot(first), COLOR_SLOT_STRIDE * sizeof(int), sizeof(int), (size_t)count, hipMemcpyDeviceToHost));
		return 0;
	}
	case 13: src = w->bodyColorMask.p; elem = 8; break;
	case 14: src = w->deg.p; elem = 4; break;
	case 15: src = w->hubList.p; elem = 4; break;
	case 16: src = w->bodyActive.p; elem = 8; break;
	case 17: src = w->b_blk1.p; elem = 4; break;
	case 18: src = w->li_ref.p; break;
	case 19: src = w->rowColor.p; elem = 4; break;
	case 20: src = w->blkRowStart.p; elem = 4; break;
	case 21: src = w->bodyRest.p; elem = 8; break;
	case 22:
	{
		const long long stats[2] = { w->statSorts, w->statSortsOnepass };
		if (first < 0 || count < 0 || first + count > 2) return setError(B2HIP_ERR_INVALID, "pair-update statistics: [0, 2)");
		memcpy(out, stats + first, (size_t)count * sizeof(long long));
		return 0;
	}
	case 23:
	{
		if (first < 0 || count < 0 || first + count > KS_STATS + 2) return setError(B2HIP_ERR_INVALID, "key-set statistics: [0, 12)");
		Counters c;
		HIP_TRY(hipMemcpy(&c, &w->d_state.p->c, sizeof(Counters), hipMemcpyDeviceToHost));
		long long stats[KS_STATS + 2];
		for (int k = 0; k < KS_STATS; ++k) stats[k] = (long long)c.ksStats[k];
		stats[KS_STATS] = c.ksFill;
		stats[KS_STATS + 1] = c.ksMask;
		memcpy(out, stats + first, (size_t)count * sizeof(long long));
		return 0;
	}
	case 24:
	{
		if (first != 0 || count != 1) return setError(B2HIP_ERR_INVALID, "narrow-phase statistics: [0, 1)");
		memcpy(out, &w->statCollideCompact, sizeof(long long));
		return 0;
	}
	case 31:
	{
		if (first != 0 || count != 1) return setError(B2HIP_ERR_INVALID, "island-build statistics: [0, 1)");
		memcpy(out, &w->statUnionSkipped, sizeof(long long));
		return 0;
	}
	case 29:
	{
		if (first != 0 || count != 1) return setError(B2HIP_ERR_INVALID, "lifecycle statistics: [0, 1)");
		memcpy(out, &w->statLifecycleLongSorts, sizeof(long long));
		return 0;
	}
	case 30:
	{
		const long long stats[2] = { w->statFixtureLongSorts, w->statFixtureRelists };
		if (first < 0 || count < 0 || first + count > 2) return setError(B2HIP_ERR_INVALID, "fixture-batch statistics: [0, 2)");
		memcpy(out, stats + first, (size_t)count * sizeof(long long));
		return 0;
	}
	case 32:
	{
		if (first != 0 || count != 1) return setError(B2HIP_ERR_INVALID, "body-property statistics: [0, 1)");
		memcpy(out, &w->statBodyPropRefits, sizeof(long long));
		return 0;
	}
	case 25:
	{
		if (first < 0 || count < 0 || first + count > ToiStats::N) return setError(B2HIP_ERR_INVALID, "TOI host statistics: [0, 10)");
		memcpy(out, w->toiStats.n + first, (size_t)count * sizeof(long long));
		return 0;
	}
	case 26:
	{
		// (effBlk, b2d_kernels_island.h, evaluated here from copies of what it reads; ownIdBlock is the device's own function)
		const int nb = (int)std::min(w->bodies.size(), w->upBodies); // (the bodies the device has rows for)
		if (first < 0 || count < 0 || first + count > nb) return setError(B2HIP_ERR_INVALID, "effective blocks: [0, uploaded bodies)");
		if (count == 0) return 0;
		if (!w->d_state.p || !w->b_blk1.p || !w->b_adopt.p || !w->b_flags.p) return setError(B2HIP_ERR_INVALID, "effective blocks: nothing uploaded yet");
		Counters c;
		HIP_TRY(hipMemcpy(&c, &w->d_state.p->c, sizeof(Counters), hipMemcpyDeviceToHost));
		std::vector<int> blk1((size_t)count), adopt((size_t)count);
		std::vector<uint32_t> flags((size_t)count);
		HIP_TRY(hipMemcpy(blk1.data(), w->b_blk1.p + first, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(adopt.data(), w->b_adopt.p + first, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(flags.data(), w->b_flags.p + first, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
		const int blocks = c.nBlocks < MAX_BLOCKS ? c.nBlocks : MAX_BLOCKS;
		const bool ownIdOff = (w->dw.nJoints != 0 || c.maxDegree > HUB_DEGREE) && w->dw.noOwnIdBlocks >= 0;
		int* e = (int*)out;
		for (int k = 0; k < count; ++k)
		{
			const int offered = adopt[k] & 0x7ff; // (adoptBlock)
			if (blk1[k]) e[k] = blk1[k];
			else if (offered || w->dw.noOwnIdBlocks > 0) e[k] = offered;
			else if ((flags[k] & BF_LARGE) == 0 || ownIdOff) e[k] = 0;
			else e[k] = blocks > 0 ? ownIdBlock(first + k, blocks) : 0;
		}
		return 0;
	}
	case 27:
	{
		const int N = 28;
		if (first < 0 || count < 0 || first + count > N) return setError(B2HIP_ERR_INVALID, "large-island plan: [0, 28)");
		const b2hip_world::PlanRecord& r = w->planRecord;
		Counters c;
		memset(&c, 0, sizeof(c));
		unsigned long long meta = 0ull;
		if (w->d_state.p) HIP_TRY(hipMemcpy(&c, &w->d_state.p->c, sizeof(Counters), hipMemcpyDeviceToHost));
		if (w->hubMeta.p) HIP_TRY(hipMemcpy(&meta, w->hubMeta.p, sizeof(meta), hipMemcpyDeviceToHost));
		const int v[N] = { (int)(r.passes & 0x7fffffff), r.solver, r.safe, r.restFirst, r.tailFirst, r.bigEnd, r.useRest, r.fuseHub, r.blockSort, r.hubWide,
			r.serialOrphans, r.nColors, r.hasHubs, r.hasJoints, r.hubBuildOne, r.useSweepEnd, r.leftoverApart,
			c.nHubRows, c.nHubWide, meta != 0ull ? (int)(uint32_t)(meta & 0xffffffffull) : -1, (int)(meta >> 32),
			c.nBlocks, c.nColors, c.maxDegree, w->forceLarge, w->dw.smallMaxW, w->dw.testMaxColors, (int)w->joints.size() };
		memcpy(out, v + first, (size_t)count * sizeof(int));
		return 0;
	}
	case 28:
	{
		const int nj = (int)w->joints.size();
		if (first < 0 || count < 0 || first + count > nj) return setError(B2HIP_ERR_INVALID, "joint bodies: [0, joints)");
		int* q = (int*)out;
		for (int k = 0; k < count; ++k)
		{
			const RevoluteJoint& j = w->joints[(size_t)(first + k)];
			const bool dead = j.type == B2D_JOINT_DEAD;
			const bool gear = j.type == B2D_JOINT_GEAR && j.enableLimit >= 0 && (size_t)j.enableLimit < w->gears.size();
			q[4 * k + 0] = dead ? -1 : j.bodyA;
			q[4 * k + 1] = dead ? -1 : j.bodyB;
			q[4 * k + 2] = gear ? w->gears[(size_t)j.enableLimit].bodyC : -1;
			q[4 * k + 3] = gear ? w->gears[(size_t)j.enableLimit].bodyD : -1;
		}
		return 0;
	}
	default: return setError(B2HIP_ERR_INVALID, "bad array id");
	}
	HIP_TRY(hipMemcpy(out, (const char*)src + (size_t)first * elem, (size_t)count * elem, hipMemcpyDeviceToHost));
	return 0;
}

// Test hook: radixSort (b2hip_host_phases.h) over the caller's arrays on the world's stream - `count` keys with two payload
// ints each, sorted in place by the passes (shift, width <= RADIX_BITS) given, in the form the world would take for a sort of
// count / RADIX_TILE + 1 tiles (B2HIP_SORT_ONEPASS, RADIX_ONEPASS_MAX_TILES, RADIX_MAX_PASSES).
int b2hip_test_radix_sort(b2hip_world* w, int count, uint64_t* keys, int* payloads, int passes, const int* shifts, const int* widths)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	DEVICE_GUARD(w);
	if (count < 0 || passes < 1 || !shifts || !widths || (count > 0 && (!keys || !payloads))) return setError(B2HIP_ERR_INVALID, "bad argument");
	if (w->stepActive) return setError(B2HIP_ERR_INVALID, "inside a step");
	std::vector<std::pair<int, int>> lay;
	for (int p = 0; p < passes; ++p)
	{
		if (widths[p] < 1 || widths[p] > RADIX_BITS || shifts[p] < 0 || shifts[p] + widths[p] > 64) return setError(B2HIP_ERR_INVALID, "bad pass");
		lay.push_back(std::make_pair(shifts[p], widths[p]));
	}
	int rc = ensureCapacity(w, 0);
	if (rc) return rc;
	hipStream_t s = w->stream;
	const int tilesCap = count / RADIX_TILE + 1;
	// the scratch of either form for that many tiles (ensureCapacity sizes it for the world's pair buffers)
	const size_t tiles = (size_t)tilesCap + 1;
	rc = w->radixHist.ensure(RADIX_DIGITS * tiles + 2, s); if (rc) return rc;
	rc = w->radixHistScan.ensure(RADIX_DIGITS * tiles + 4, s); if (rc) return rc;
	rc = w->scanTmp.ensure(3 * (RADIX_DIGITS * tiles / SCAN_TILE + 8), s); if (rc) return rc;
	rc = w->scanFlags.ensure(RADIX_DIGITS * tiles / SCAN_TILE + 8, s); if (rc) return rc;
	if (w->sortOnepass)
	{
		const size_t onepassTiles = std::min<size_t>(tiles, RADIX_ONEPASS_MAX_TILES);
		rc = w->radixCounts.ensure(onepassTiles * RADIX_DIGITS, s, false); if (rc) return rc;
		rc = w->radixGroups.ensure((onepassTiles / RADIX_GROUP + 1) * RADIX_DIGITS, s, false); if (rc) return rc;
	}
	rc = ensureCapacity(w, 0); // (the kernarg block and the scan / radix contexts point at the grown arrays)
	if (rc) return rc;
	DevArray<uint64_t> k0, k1;
	DevArray<int2> v0, v1;
	DevArray<int> nDev;
	const size_t room = (size_t)count + 1;
	rc = k0.ensure(room, s, false, false);
	if (!rc) rc = k1.ensure(room, s, false, false);
	if (!rc) rc = v0.ensure(room, s, false, false);
	if (!rc) rc = v1.ensure(room, s, false, false);
	if (!rc) rc = nDev.ensure(1, s, false, true);
	auto done = [&](int code) { (void)hipStreamSynchronize(s); return code; }; // (the arrays free themselves: not under a running stream)
	if (rc) return done(rc);
	hipError_t e = hipMemcpyAsync(nDev.p, &count, sizeof(int), hipMemcpyHostToDevice, s);
	if (e == hipSuccess && count > 0) e = hipMemcpyAsync(k0.p, keys, (size_t)count * sizeof(uint64_t), hipMemcpyHostToDevice, s);
	if (e == hipSuccess && count > 0) e = hipMemcpyAsync(v0.p, payloads, (size_t)count * sizeof(int2), hipMemcpyHostToDevice, s);
	if (e != hipSuccess) return done(setError(B2HIP_ERR_HIP, hipGetErrorString(e)));
	uint64_t *kin = k0.p, *kout = k1.p;
	int2 *vin = v0.p, *vout = v1.p;
	rc = radixSort(w, kin, kout, vin, vout, nDev.p, tilesCap, lay);
	if (rc) return done(rc);
	int overflow = 0;
	e = hipMemcpyAsync(&overflow, &w->d_state.p->c.overflow, sizeof(int), hipMemcpyDeviceToHost, s);
	if (e == hipSuccess && count > 0) e = hipMemcpyAsync(keys, kin, (size_t)count * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
	if (e == hipSuccess && count > 0) e = hipMemcpyAsync(payloads, vin, (size_t)count * sizeof(int2), hipMemcpyDeviceToHost, s);
	if (e == hipSuccess) e = hipStreamSynchronize(s);
	if (e != hipSuccess) return done(setError(B2HIP_ERR_HIP, hipGetErrorString(e)));
	if (overflow & SCAN_ABORT_BIT) return done(setError(B2HIP_ERR_HIP, "a look-back of the sort gave up waiting for a predecessor tile"));
	return done(0);
}

// Test hook: is the kept contact-key set what it claims to be? Reads only. Two passes behind a synchronisation: over the live
// contacts (keys of non-foreign contacts the set does not hold) and over the table under its mask (live entries,
// tombstones). out[0] the set is valid and not stale, [1] missing keys, [2] live entries - non-foreign live contacts (with
// nothing missing and unique keys, 0 means that no dead contact's entry survives), [3] recounted fill (live + tombstones) -
// Counters::ksFill, [4] live entries, [5] tombstones.
__global__ __launch_bounds__(256) void k_keyset_check(DW W, unsigned long long* out)
{
	const DState* S = W.st;
	const ContactArrays& C = W.ca[S->cur];
	const uint32_t mask = S->c.ksMask;
	const int stride = (int)(gridDim.x * blockDim.x), t0 = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	int missing = 0, own = 0, live = 0, tomb = 0;
	for (int i = t0; i < S->c.nContacts; i += stride)
	{
		if (C.flags[i] & CF_FOREIGN) continue;
		own += 1;
		// (as htContains, without its stale mark)
		const uint64_t key = C.key[i] + 1ull;
		uint32_t h = hashKey(key) & mask;
		bool found = false;
		for (uint32_t probes = 0; probes <= mask; ++probes)
		{
			const uint64_t v = W.ht_keys[h];
			if (v == key) { found = true; break; }
			if (v == 0) break;
			h = (h + 1) & mask;
		}
		if (!found) missing += 1;
	}
	for (uint32_t i = (uint32_t)t0; i <= mask; i += (uint32_t)stride)
	{
		const uint64_t v = W.ht_keys[i];
		if (v == HT_TOMB) tomb += 1;
		else if (v != 0) live += 1;
	}
	missing = waveSumInt(missing); own = waveSumInt(own); live = waveSumInt(live); tomb = waveSumInt(tomb);
	if (waveLane() == 0)
	{
		if (missing) atomicAdd(&out[0], (unsigned long long)missing);
		if (own) atomicAdd(&out[1], (unsigned long long)own);
		if (live) atomicAdd(&out[2], (unsigned long long)live);
		if (tomb) atomicAdd(&out[3], (unsigned long long)tomb);
	}
}

int b2hip_test_keyset_check(b2hip_world* w, long long out[6])
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	DEVICE_GUARD(w);
	if (!out) return setError(B2HIP_ERR_INVALID, "null argument");
	if (w->stepActive) return setError(B2HIP_ERR_INVALID, "inside a step");
	HIP_TRY(hipStreamSynchronize(w->stream));
	memset(out, 0, 6 * sizeof(long long));
	if (!w->d_state.p || !w->ht_keys.p) return 0; // (nothing uploaded yet: no set)
	Counters c;
	HIP_TRY(hipMemcpy(&c, &w->d_state.p->c, sizeof(Counters), hipMemcpyDeviceToHost));
	const bool valid = w->dw.keysetKeep && !w->dw.spatial && c.ksValid && !c.ksStale;
	out[0] = valid ? 1 : 0;
	if (c.ksMask > w->dw.htMask) return valid ? setError(B2HIP_ERR_INVALID, "key set: mask beyond the table") : 0;
	DevArray<unsigned long long> sums;
	int rc = sums.ensure(4, w->stream, false, true);
	if (rc) return rc;
	unsigned long long h[4] = { 0, 0, 0, 0 };
	hipLaunchKernelGGL(k_keyset_check, dim3(gridFor((size_t)c.ksMask + 1)), dim3(256), 0, w->stream, w->dw, sums.p);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(h, sums.p, sizeof(h), hipMemcpyDeviceToHost, w->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
	else (void)hipStreamSynchronize(w->stream);
	if (e != hipSuccess) return setError(B2HIP_ERR_HIP, hipGetErrorString(e));
	out[1] = (long long)h[0];
	out[2] = (long long)h[2] - (long long)h[1];
	out[3] = (long long)h[2] + (long long)h[3] - (long long)c.ksFill;
	out[4] = (long long)h[2];
	out[5] = (long long)h[3];
	return 0;
}

// Test hook: who owns what. out[0] the blocks the owner types (DevArray, PinnedBuf) hold in this process right now - what a
// destroyed world leaves behind shows as a count that does not come back; out[1] the arrays of WORLD_ARRAYS_DW whose pointer
// in the world's kernarg block is not the array's own (0 without a world).
int b2hip_test_storage(b2hip_world* w, long long out[2])
{
	if (!out) return setError(B2HIP_ERR_INVALID, "null argument");
	out[0] = g_liveBlocks.load();
	out[1] = 0;
	if (!w) return 0;
#define X(T, name, count, keep, zeroNew) out[1] += w->dw.name != w->name.p;
	WORLD_ARRAYS_DW(X)
#undef X
	return 0;
}

// Debug hook (B2HIP_TRACE=1): stage labels + state hashes recorded by the last b2hip_solve.
int b2hip_debug_trace(b2hip_world* w, int index, char* label, int label_cap, uint64_t* hash)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	if (index < 0 || index >= (int)w->trace.size()) return 1;
	if (label && label_cap > 0)
	{
		strncpy(label, w->trace[index].first.c_str(), (size_t)label_cap - 1);
		label[label_cap - 1] = 0;
	}
	if (hash) *hash = w->trace[index].second;
	return 0;
}

int b2hip_get_profile(b2hip_world* w, float ms[13])
{
	if (!w || !ms) return setError(B2HIP_ERR_INVALID, "null argument");
	memcpy(ms, w->profile, sizeof(float) * 13);
	return 0;
}

int b2hip_get_counters(b2hip_world* w, b2hip_counters* out)
{
	if (!w || !out) return setError(B2HIP_ERR_INVALID, "null argument");
	memset(out, 0, sizeof(*out));
	out->bodies = (int)w->bodies.size();
	out->proxies = (int)w->fixtures.size();
	out->contacts = w->last.nContacts;
	out->touching_contacts = w->last.nTouching;
	out->islands = w->last.nIslands;
	out->small_islands = w->last.nSIslands;
	out->large_islands = w->last.nLIslands;
	out->small_island_bodies = w->last.nSBodies;
	out->small_island_contacts = w->last.nSContacts;
	out->large_island_bodies = w->last.nLBodies;
	out->large_island_contacts = w->last.nLContacts;
	out->colors = w->last.nColors;
	out->moved_proxies = w->last.nMoves;
	out->new_contacts = w->last.nNewContacts;
	out->destroyed_contacts = w->last.nDestroy;
	out->solver_chunks = w->last.nChunks;
	out->pos_iterations_large = w->last.posItersLarge;
	out->overflow_flags = w->last.overflow;
	out->toi_events = w->last.nToiEvents;
	out->toi_calls = w->last.nToiCalls;
	out->toi_pending_first_pass = w->last.nToiList;
	out->toi_serial_fallbacks = (int)w->toiStats.n[ToiStats::SerialFallback];
	out->blocks = w->last.nBlocks;
	out->cut_constraints = w->last.nCutRows;
	out->block_max_rows = w->last.blkMaxRows;
	out->partitions = w->last.partitions;
	out->block_solver_steps = w->blockSteps;
	out->free_islands = w->last.nFreeIslands;
	out->sweep_solver_steps = w->sweepSteps;
	out->hub_constraints = w->last.nHubRows;
	out->hub_fixpoint_rounds = w->last.hubRounds;
	out->hub_serial_chunks = w->last.hubSerialChunks;
	out->toi_chain_contacts = (int)w->toiStats.chainContacts;
	out->toi_pre_solve_reruns = (int)w->toiStats.n[ToiStats::PreSolveRerun];
	out->solver_recoveries = w->solverRecoveries + w->colorRecoveries;
	return 0;
}

int b2hip_get_solver_timing(b2hip_world* w, float* ms, double* algorithmic_bytes, int* constraints, int* bodies)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	if (ms) *ms = w->solverMs;
	if (algorithmic_bytes) *algorithmic_bytes = w->solverBytes;
	if (constraints) *constraints = w->solverConstraints;
	if (bodies) *bodies = w->solverBodies;
	return 0;
}

int b2hip_set_kernel_timing(b2hip_world* w, int enable)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	w->kernelTiming = enable;
	return 0;
}

int b2hip_set_kernel_timing_units(b2hip_world* w, long long units_a, long long units_b)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	w->ktUnitsA = units_a;
	w->ktUnitsB = units_b;
	return 0;
}

int b2hip_get_kernel_timing(b2hip_world* w, char* name, int name_cap, float* total_ms, int* launches, double* algorithmic_bytes)
{
	if (!w) return setError(B2HIP_ERR_INVALID, "null world");
	const char* n = w->ktKind == 8 ? "large-island solver family (k_large_integrate / init / velocity / rest / k_sweep_end / position / store_impulses / finalize / sleep)" : w->ktKind == 5 ? "k_collide" : w->ktKind == 6 ? "k_sync_fixtures" : w->ktKind == 7 ? "k_find_pairs_small" : w->ktKind == 4 ? "k_solve_blocks" : w->ktKind == 1 ? "k_large_velocity" : (w->ktKind == 2 ? "k_solve_small" : "");
	if (name && name_cap > 0)
	{
		strncpy(name, n, (size_t)name_cap - 1);
		name[name_cap - 1] = 0;
	}
	if (total_ms) *total_ms = w->ktMs;
	if (launches) *launches = w->ktLaunches;
	if (algorithmic_bytes) *algorithmic_bytes = w->ktBytes;
	return 0;
}

// (diagnostics, not part of include/b2hip.h: the device clock stamps around the mid-step census read-back, in 10 ns ticks)
// (diagnostics: the six phase stamps of the last step's resident solver - or, with B2HIP_SWEEP_STAMPS=1, of its last k_sweep_end<1>)
int b2hip_debug_stamps(b2hip_world* w, int out[6])
{
	if (!w || !out) return setError(B2HIP_ERR_INVALID, "null argument");
	for (int k = 0; k < 6; ++k) out[k] = w->h_dstate->stamps[k];
	return 0;
}

int b2hip_debug_gap_clocks(b2hip_world* w, unsigned long long out[4])
{
	if (!w || !out) return setError(B2HIP_ERR_INVALID, "null argument");
	for (int k = 0; k < 4; ++k) out[k] = w->h_dstate->gapClock[k];
	return 0;
}

