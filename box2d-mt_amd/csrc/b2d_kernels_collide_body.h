// b2d_kernels_collide_body.h - the body of the narrow-phase kernel, included once per form by b2d_kernels_collide.h (no include
// guard on purpose). In scope where it is included: DW W, int sortTile, CollideCompactArgs cc, int voidColors, and the constants
// STAGE, ORDER, COMPACT, UNION (UNION only with COMPACT). Text, not a function: the forms that existed before UNION compile to
// the instruction streams they had.
	b2dPhaseStamp(W);
	DState* S = W.st;
	const int n = S->c.nContacts;
	const ContactArrays& C = W.ca[S->cur];
	int nDestroy = 0, nTouch = 0;
	// (COMPACT: a kept key set loses the keys of the contacts dropped here)
	const bool ksOn = COMPACT && keysetMaintained(W);
	const uint32_t ksMask = COMPACT ? S->c.ksMask : 0u;
	__shared__ int s_bin[64];
	__shared__ int s_perm[256];
	// (152-byte records side by side: lanes read the same member 38 words apart - a two-way bank conflict at worst)
	// (... and, once the contacts are done, the scratch of the last workgroup's toiOrderDestroy)
	__shared__ __attribute__((aligned(16))) unsigned char s_raw[STAGE ? ((512 * sizeof(ShapeRec) > TOI_ORDER_SCRATCH_BYTES || !ORDER) ? 512 * sizeof(ShapeRec) : TOI_ORDER_SCRATCH_BYTES) : (ORDER ? TOI_ORDER_SCRATCH_BYTES : 16)];
	ShapeRec* const s_shape = (ShapeRec*)s_raw;
	// (sortTile bit 2) the shape records of the workgroup's FIRST contact wait in LDS: a world of boxes has one record, and the
	// separating-axis loops fetch its vertices and normals one by one - ~50 loads per contact, every one a round trip to the
	// vector L1 for a value all 64 lanes share, one after the other: that chain, not the bandwidth and not the arithmetic, was
	// this kernel's time on the 100 000-box Tumbler. A polygon pair whose two records are the staged ones reads LDS instead.
	__shared__ __attribute__((aligned(16))) ShapeRec s_uni[2];
	__shared__ int s_uniId[2];
	const bool uniOn = !STAGE && (sortTile & 4) != 0;
	sortTile &= 3;
	auto stageUni = [&]()
	{
		const int i0 = COMPACT ? (int)blockIdx.x * cc.chunk : (int)(blockIdx.x * blockDim.x);
		int idA = 0, idB = 0;
		if (i0 < n)
		{
			const int4 ids0 = C.ids[i0];
			idA = W.p_shape[ids0.x];
			idB = W.p_shape[ids0.y];
		}
		static_assert(sizeof(ShapeRec) % 4 == 0, "ShapeRec is copied word by word");
		constexpr int RW = (int)(sizeof(ShapeRec) / 4);
		if (threadIdx.x < 2 * RW)
		{
			const int which = (int)threadIdx.x / RW, word = (int)threadIdx.x % RW;
			((uint32_t*)&s_uni[which])[word] = ((const uint32_t*)(W.shapes + (which ? idB : idA)))[word];
		}
		if (threadIdx.x == 0) { s_uniId[0] = idA; s_uniId[1] = idB; }
	};
	// (COMPACT: staged behind the contact's own loads, in front of the barrier of the chunk's count - a workgroup has one tile,
	// and three dependent round trips in front of every tile's loads were a fifth of its time)
	if (uniOn && !COMPACT)
	{
		stageUni();
		__syncthreads();
	}
	// COMPACT: workgroup b owns the contacts [b * chunk, (b + 1) * chunk) - one pass, every lane stays to the end (the barriers
	// of the prefix), a lane without a contact reads row 0 of everything and keeps nothing
	// THE LOOP RUNS ONCE UNDER COMPACT. The `for` is the other forms' grid-stride loop, kept so that their code stays what it
	// was; under COMPACT its condition is always true and its increment is never reached: the last statement of the COMPACT
	// store phase, at the bottom of this body, is `break; // (one chunk per workgroup)`. Nothing under COMPACT may `continue`:
	// every lane has to reach the two barriers of the prefix (the `continue`s below are all under `!COMPACT`).
	for (int base = COMPACT ? blockIdx.x * cc.chunk : blockIdx.x * blockDim.x; COMPACT || base < n; base += gridDim.x * blockDim.x)
	{
		int i = base + (int)threadIdx.x;
		const bool valid = !COMPACT || ((int)threadIdx.x < cc.chunk && i < n);
		if (COMPACT && !valid) i = 0;
		if (!COMPACT && sortTile)
		{
			// the tile's contacts by class: a counting sort over 64 keys in LDS (which lane takes which contact of a class does
			// not matter: every contact is evaluated on its own)
			const int key = i < n ? collideClassKey(W, C, i) : 63;
			if (threadIdx.x < 64) s_bin[threadIdx.x] = 0;
			__syncthreads();
			const int within = atomicAdd(&s_bin[key], 1);
			__syncthreads();
			if (threadIdx.x < 64)
			{
				const int v = s_bin[threadIdx.x];
				int incl = v;
				for (int off = 1; off < 64; off <<= 1)
				{
					const int o = __shfl_up(incl, off);
					if ((int)threadIdx.x >= off) incl += o;
				}
				s_bin[threadIdx.x] = incl - v;
			}
			__syncthreads();
			s_perm[s_bin[key] + within] = (int)threadIdx.x;
			__syncthreads();
			i = base + s_perm[threadIdx.x];
		}
		if (!COMPACT && i >= n) continue;
		int4 ids = C.ids[i];
		uint32_t flags = C.flags[i];
		if (COMPACT && !valid) { ids = make_int4(0, 0, 0, 0); flags = 0u; }
		if (!COMPACT && (flags & CF_FOREIGN))
		{
			// a spatially sharded world: the bodies are another rank's, which evaluates the manifold. Here the contact only keeps
			// existing - the structural half of b2ContactManager::Collide (:177-230), the same on every rank: the re-filter, the
			// "both bodies asleep" skip, the fat-AABB test (else destroy)
			int keepF = 1;
			if (flags & CF_FILTER)
			{
				const bool ok = bodiesShouldCollide(W, ids.w, ids.z) &&
					filterShouldCollide(W.p_filter0[ids.x], W.p_filter1[ids.x], W.p_filter0[ids.y], W.p_filter1[ids.y]);
				if (!ok) keepF = 0; else flags &= ~CF_FILTER;
			}
			if (keepF && (bodyActiveForContact(W.b_flags[ids.z]) || bodyActiveForContact(W.b_flags[ids.w])))
			{
				const float4 fA = W.p_fat[ids.x], fB = W.p_fat[ids.y];
				AABB boxA, boxB;
				boxA.lo = v2(fA.x, fA.y); boxA.hi = v2(fA.z, fA.w);
				boxB.lo = v2(fB.x, fB.y); boxB.hi = v2(fB.z, fB.w);
				if (!b2dAabbOverlap(boxA, boxB)) keepF = 0;
			}
			if (!keepF)
			{
				flags |= CF_DESTROY;
				++nDestroy;
				if (flags & CF_TOI_CANDIDATE) b2dStoreAgentI(&W.toiDestroyList[atomicAdd(&S->c.nToiDestroy, 1)], i);
			}
			C.flags[i] = flags;
			W.keepFlag[i] = keepF;
			continue;
		}
		// Everything the update of a live contact reads is fetched in TWO rounds - what hangs on the contact index with the
		// ids, what hangs on the ids right after - instead of level by level behind the tests that need it (flags, then fat
		// AABBs, then the old manifold and the shape indices, then shapes and transforms: five dependent round trips in front
		// of the arithmetic). A contact that turns out inactive or out of its fat AABBs has read a few rows for nothing.
		const int4 m3 = C.man3[i];
		const float4 oldImp = C.imp[i];
		const float4 o0 = C.man0[i], o1 = C.man1[i];
		const int proxyA = ids.x, proxyB = ids.y, bodyA = ids.z, bodyB = ids.w;
		uint32_t bfA = W.b_flags[bodyA], bfB = W.b_flags[bodyB];
		const float4 fatA = W.p_fat[proxyA], fatB = W.p_fat[proxyB];
		const int shapeA = W.p_shape[proxyA], shapeB = W.p_shape[proxyB];
		const Xf xfA = loadXf(W.b_xf, bodyA), xfB = loadXf(W.b_xf, bodyB);
		int keep = 1;

		if (flags & CF_FILTER)
		{
			// (with a user contact filter the host has asked it already: k_filter_list / CF_USER_REJECT)
			bool ok = bodiesShouldCollide(W, bodyB, bodyA) &&
				(W.userFilter ? (flags & CF_USER_REJECT) == 0
				              : filterShouldCollide(W.p_filter0[proxyA], W.p_filter1[proxyA], W.p_filter0[proxyB], W.p_filter1[proxyB]));
			flags &= ~CF_USER_REJECT;
			if (!ok)
			{
				keep = 0;
			}
			else
			{
				flags &= ~CF_FILTER;
			}
		}

		flags &= ~(CF_PRESOLVE | CF_VC_ONE_POINT);
		bool active = bodyActiveForContact(bfA) || bodyActiveForContact(bfB);
		// COMPACT: the manifold as the contact will hold it - what the evaluation does not change stays what was loaded
		CollideManifold<COMPACT> now;
		now.set(o0, o1, oldImp);
		now.set3(m3);
		// COMPACT: who stays is known before any manifold is evaluated (the filter, the awake bits, the fat AABBs - all loaded
		// above) - the chunk's count goes out now, and by the time the evaluation below is through, the chunks before this
		// one have published theirs long ago
		int rank = 0;
		unsigned early = 0u;
		if (COMPACT)
		{
			__shared__ int s_waveKeep[4];
			int stays = valid ? keep : 0;
			if (stays && active && (fatB.x - fatA.z > 0.0f || fatB.y - fatA.w > 0.0f || fatA.x - fatB.z > 0.0f || fatA.y - fatB.w > 0.0f)) stays = 0; // (b2dAabbOverlap, as below)
			const unsigned long long kb = __ballot(stays != 0);
			const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
			rank = __popcll(kb & ((1ull << lane) - 1ull));
			if (lane == 0) s_waveKeep[wave] = __popcll(kb);
			if (uniOn) stageUni();
			__syncthreads();
			int chunkKeep = 0;
			for (int q = 0; q < 4; ++q)
			{
				const int c = s_waveKeep[q];
				chunkKeep += c;
				if (q < wave) rank += c;
			}
			const int chunkId = (int)blockIdx.x, inGroup = chunkId % COLLIDE_GROUP;
			if (threadIdx.x == 0) __hip_atomic_store(cc.counts + chunkId, (cc.tag << 16) | (unsigned)chunkKeep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			// the last chunk of a group of COLLIDE_GROUP publishes the group's sum as soon as the counts before its own are there
			// (a count depends on nothing, a group's sum on counts only: no chain - the scheme of k_radix_onepass, b2d_scan.h)
			if (inGroup == COLLIDE_GROUP - 1 && wave == 0)
			{
				bool gaveUp = false;
				int v = 0;
				if (lane < COLLIDE_GROUP - 1)
				{
					const unsigned* src = cc.counts + (chunkId - inGroup) + lane;
					v = radixAwait(src, __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), cc.tag, cc.abortWord, gaveUp);
				}
				v = waveSumInt(v);
				if (lane == 0) __hip_atomic_store(cc.groups + chunkId / COLLIDE_GROUP, (cc.tag << 16) | (unsigned)(v + chunkKeep), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
			// the first round of the look-back is fetched now, a word per lane: the chunks before this one started before it
			// and have published as a rule - the word is looked at behind the evaluation, and asked for again only if it was early
			if ((int)threadIdx.x < inGroup + chunkId / COLLIDE_GROUP)
				early = __hip_atomic_load(lookBackWord(cc, chunkId, (int)threadIdx.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		if (keep && active && valid)
		{
			AABB boxA, boxB;
			boxA.lo = v2(fatA.x, fatA.y); boxA.hi = v2(fatA.z, fatA.w);
			boxB.lo = v2(fatB.x, fatB.y); boxB.hi = v2(fatB.z, fatB.w);
			bool overlap = b2dAabbOverlap(boxA, boxB);
			if (!overlap)
			{
				keep = 0;
			}
			else if (flags & CF_FOREIGN)
			{
				// a spatially sharded world: the bodies are another rank's, which evaluates the manifold; here the contact only
				// keeps existing (the overlap test above is structure: every rank destroys the same contacts)
			}
			else
			{
				// b2Contact::UpdateImpl (b2Contact.cpp:173-298)
				const uint32_t oldId0 = (uint32_t)m3.x, oldId1 = (uint32_t)m3.y;
				const int oldCount = m3.w;
				flags |= CF_ENABLED;
				bool wasTouching = (flags & CF_TOUCHING) != 0;
				bool touching = false;
				bool sensor = (flags & CF_SENSOR) != 0;
				float4 o0s = make_float4(0, 0, 0, 0), o1s = o0s; // the old manifold's vectors, for PreSolve
				Manifold mf;
				mf.pointCount = 0;
				mf.type = m3.z;
				mf.id[0] = oldId0; // a sensor keeps whatever the manifold held (the reference leaves it untouched)
				mf.id[1] = oldId1;
				if (sensor)
				{
					// b2Contact::Update, sensor branch (b2Contact.cpp:193-202): touching = b2TestOverlap (b2Collision.cpp:233-252),
					// GJK distance with the shape radii below 10 epsilon; no manifold. Sensors never enter the solver.
					const GjkProxy pA = b2dProxy(W.shapes + shapeA);
					const GjkProxy pB = b2dProxy(W.shapes + shapeB);
					GjkCache cache;
					cache.count = 0;
					cache.metric = 0.0f;
					for (int k = 0; k < 3; ++k) cache.indexA[k] = cache.indexB[k] = 0;
					GjkOutput dist;
					b2dDistance(dist, cache, pA, xfA, pB, xfB, true);
					touching = dist.distance < 10.0f * B2D_EPSILON;
					mf.pointCount = 0;
				}
				else
				{
					const ShapeRec* sA = W.shapes + shapeA;
					const ShapeRec* sB = W.shapes + shapeB;
					if (STAGE)
					{
						static_assert(sizeof(ShapeRec) % 8 == 0, "ShapeRec is copied in 8-byte pieces");
						const float2* gA = (const float2*)sA;
						const float2* gB = (const float2*)sB;
						float2* lA = (float2*)&s_shape[2 * threadIdx.x];
						float2* lB = (float2*)&s_shape[2 * threadIdx.x + 1];
#pragma unroll
						for (int q = 0; q < (int)(sizeof(ShapeRec) / 8); ++q) { lA[q] = gA[q]; lB[q] = gB[q]; }
						sA = &s_shape[2 * threadIdx.x];
						sB = &s_shape[2 * threadIdx.x + 1];
					}
					// stale fields survive an early-out exactly like the reference's persistent manifold
					o0s = o0;
					o1s = o1;
					mf.localNormal = v2(o0.x, o0.y);
					mf.localPoint = v2(o0.z, o0.w);
					mf.p[0] = v2(o1.x, o1.y);
					mf.p[1] = v2(o1.z, o1.w);
					mf.id[0] = oldId0;
					mf.id[1] = oldId1;
					bool evaluated = false;
					if (uniOn)
					{
						const int u0 = s_uniId[0], u1 = s_uniId[1];
						const bool a0 = shapeA == u0, b0 = shapeB == u0;
						if ((a0 || shapeA == u1) && (b0 || shapeB == u1))
						{
							const ShapeRec* lA = &s_uni[a0 ? 0 : 1];
							const ShapeRec* lB = &s_uni[b0 ? 0 : 1];
							if (lA->type == B2D_SHAPE_POLYGON && lB->type == B2D_SHAPE_POLYGON && lA->count == 4 && lB->count == 4)
							{
								b2dCollidePolygons<4>(&mf, lA, xfA, lB, xfB);
								evaluated = true;
							}
						}
					}
					if (!evaluated) b2dEvaluate(&mf, sA, xfA, sB, xfB);
					touching = mf.pointCount > 0;
					float ni[2], ti[2];
					ni[0] = oldImp.x; ti[0] = oldImp.y; ni[1] = oldImp.z; ti[1] = oldImp.w;
					for (int k = 0; k < mf.pointCount; ++k)
					{
						mf.ni[k] = 0.0f;
						mf.ti[k] = 0.0f;
						uint32_t id2 = mf.id[k];
						if (oldCount > 0 && oldId0 == id2)
						{
							mf.ni[k] = oldImp.x;
							mf.ti[k] = oldImp.y;
						}
						else if (oldCount > 1 && oldId1 == id2)
						{
							mf.ni[k] = oldImp.z;
							mf.ti[k] = oldImp.w;
						}
						ni[k] = mf.ni[k];
						ti[k] = mf.ti[k];
					}
					if (touching != wasTouching)
					{
						// quirk kept: only fixture A's body is woken (b2ContactManager.cpp:472-485)
						W.b_wake[bodyA] = 1;
					}
					// (round 6) only what CHANGED is stored: five of six contacts of a dense pile are fat-AABB pairs that did not touch
					// before and do not touch now - their manifold comes out of b2dEvaluate bit for bit as it went in (the early-outs leave
					// the stale fields alone, as the reference's persistent manifold does), and storing it again was 64 of this kernel's
					// ~150 written bytes per contact. Compared as bits: what is in memory afterwards is the same either way.
					{
						const float4 n0 = make_float4(mf.localNormal.x, mf.localNormal.y, mf.localPoint.x, mf.localPoint.y);
						const float4 n1 = make_float4(mf.p[0].x, mf.p[0].y, mf.p[1].x, mf.p[1].y);
						const float4 nI = make_float4(ni[0], ti[0], ni[1], ti[1]);
						if (COMPACT) now.set(n0, n1, nI);
						else
						{
							if (!b2dSameBits4(n0, o0)) C.man0[i] = n0;
							if (!b2dSameBits4(n1, o1)) C.man1[i] = n1;
							if (!b2dSameBits4(nI, oldImp)) C.imp[i] = nI;
						}
					}
				}
				if (!COMPACT && W.preSolveOn && !sensor && touching)
				{
					// what PreSolve is handed as the old manifold (the new one has just overwritten it above)
					W.pre_o0[i] = o0s;
					W.pre_o1[i] = o1s;
					W.pre_oimp[i] = oldImp;
					W.pre_o3[i] = m3;
					flags |= CF_PRESOLVE;
				}
				{
					const int4 n3 = make_int4((int)mf.id[0], (int)mf.id[1], mf.type, mf.pointCount);
					if (COMPACT) now.set3(n3);
					else if (n3.x != m3.x || n3.y != m3.y || n3.z != m3.z || n3.w != m3.w) C.man3[i] = n3;
				}
				if (touching) flags |= CF_TOUCHING; else flags &= ~CF_TOUCHING;
			}
		}

		if (COMPACT && !valid)
		{
			// (no contact here)
		}
		else if (!keep)
		{
			if (!COMPACT && W.eventsOn && (flags & CF_REPORTED))
			{
				// b2ContactManager::Destroy (b2ContactManager.cpp:104-107): a touching contact ends when it is destroyed
				const int e = atomicAdd(&S->c.nEvents, 1);
				if (e < W.capContacts)
				{
					W.evKey[e] = C.key[i];
					W.evInfo[e] = make_int4(proxyA, proxyB, 1, -1);
				}
			}
			flags |= CF_DESTROY;
			++nDestroy;
			if (COMPACT)
			{
				// (the host takes this form only while no TOI candidate is alive: the replay of a dying one addresses the contacts
				// by the index they are about to lose. Should one die here all the same, the step fails through the read-back.)
				if (flags & CF_TOI_CANDIDATE) atomicOr(cc.abortWord, SCAN_ABORT_BIT);
			}
			else if (flags & CF_TOI_CANDIDATE) b2dStoreAgentI(&W.toiDestroyList[atomicAdd(&S->c.nToiDestroy, 1)], i); // (read by the last workgroup)
			// b2Contact::Destroy (b2Contact.cpp:100-113): wake both bodies if the manifold had points
			int pc = COMPACT ? m3.w : C.man3[i].w;
			if (pc > 0 && (flags & (CF_SENSOR | CF_FOREIGN)) == 0) // (a foreign contact's point count is not maintained: its owner wakes the bodies)
			{
				W.b_wake[bodyA] = 1;
				W.b_wake[bodyB] = 1;
			}
		}
		else if ((flags & (CF_TOUCHING | CF_FOREIGN)) == CF_TOUCHING)
		{
			++nTouch;
		}
		if (!COMPACT)
		{
			C.flags[i] = flags;
			W.keepFlag[i] = keep;
		}
		else
		{
			// The survivors go to their place in the other half: the survivors of the chunks before this one (the counts of the own
			// group, the sums of the groups before it: a word per lane, every wait bounded as in k_radix_onepass) + the rank inside
			// the chunk. What the evaluation did not need is fetched now, beside the look-back. A contact that is dropped leaves
			// the kept key set here, as it does in k_compact_contacts.
			__shared__ int s_before[4];
			const ContactArrays& B = W.ca[1 - S->cur];
			const uint64_t key = C.key[i];
			const float4 mat = C.mat[i];
			const int color = C.color[i];
			const int mgr = C.mgr[i];
			const int chunkId = (int)blockIdx.x, group = chunkId / COLLIDE_GROUP, inGroup = chunkId % COLLIDE_GROUP;
			int before = 0;
			bool gaveUp = false;
			for (int q = (int)threadIdx.x; q < inGroup + group; q += (int)blockDim.x)
			{
				const unsigned* src = lookBackWord(cc, chunkId, q);
				before += radixAwait(src, q < (int)blockDim.x ? early : __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), cc.tag, cc.abortWord, gaveUp);
			}
			before = waveSumInt(before);
			if (waveLane() == 0) s_before[threadIdx.x >> 6] = before;
			__syncthreads();
			const int j = s_before[0] + s_before[1] + s_before[2] + s_before[3] + rank;
			const bool stored = valid && keep && j <= i; // (j <= i always, unless a look-back gave up)
			if (stored)
			{
				B.ids[j] = ids;
				B.key[j] = key;
				B.flags[j] = UNION ? flags & ~CF_ISLAND : flags; // (UNION: b2World::Solve's wipe, b2World.cpp:1191-1194, as k_island_union does it)
				B.mat[j] = mat;
				B.man0[j] = now.man0();
				B.man1[j] = now.man1();
				B.imp[j] = now.imp();
				B.man3[j] = now.man3();
				B.color[j] = (UNION && voidColors) ? collideVoidColor(W, flags, color) : color;
				B.mgr[j] = mgr;
				if (mgr >= 0) W.toiPos2c[mgr] = j;
			}
			else if (valid && !keep && ksOn)
			{
				// (every contact dropped here is counted in nDestroy and none is foreign: the tombstones written are the
				// destroyed minus the keys not found, so both ride the census' arrival. A key that is not found - a fault of the
				// set, never seen - is counted in the first word of ARRIVE_COMPACT's tree, idle and zero while this form runs.)
				if (!htDelete(W, ksMask, key + 1ull)) __hip_atomic_fetch_add(W.arriveTree + (size_t)ARRIVE_COMPACT * TREE_WORDS, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
			// UNION: the solid survivors join the forest under their new index (every lane arrives here: the tail shuffles)
			if (UNION) collideUnionTail(W, stored && contactSolid(flags), j, bodyA, bodyB);
			break; // (one chunk per workgroup)
		}
	}
	if (COMPACT)
	{
		// (a launch sized for fewer contacts than there are - the host's count was not the device's: the step fails)
		if (blockIdx.x == 0 && threadIdx.x == 0 && (long long)n > (long long)gridDim.x * cc.chunk) atomicOr(cc.abortWord, SCAN_ABORT_BIT);
	}
	// the census of the pass (destroyed, touching) travels with the arrival of the workgroups (b2d_world.h: b2dTreeArrive -
	// one atomic per WAVE on each of the two counters was 2 x 2 000 atomics on one word for the 128 000 contacts of the 1 M
	// field, served one after the other); the last workgroup to finish adds the totals, and:
	// the TOI candidates destroyed by this pass leave the manager's slot order
	{
		__shared__ int s_census[2];
		if (threadIdx.x == 0) { s_census[0] = 0; s_census[1] = 0; }
		__syncthreads();
		nDestroy = waveSumInt(nDestroy);
		nTouch = waveSumInt(nTouch);
		if (waveLane() == 0)
		{
			if (nDestroy) atomicAdd(&s_census[0], nDestroy);
			if (nTouch) atomicAdd(&s_census[1], nTouch);
		}
		__syncthreads();
		const bool fit = (unsigned)W.capContacts <= TREE_SUM_MAX;
		if (!fit && threadIdx.x == 0)
		{
			if (s_census[0]) atomicAdd(&S->c.nDestroy, s_census[0]);
			if (s_census[1]) atomicAdd(&S->c.nTouching, s_census[1]);
		}
		unsigned t0 = 0u, t1 = 0u;
		if (b2dLastBlockArrive(W, ARRIVE_COLLIDE, fit ? (unsigned)s_census[0] : 0u, fit ? (unsigned)s_census[1] : 0u, &t0, &t1))
		{
			if (threadIdx.x == 0)
			{
				if (t0) atomicAdd(&S->c.nDestroy, (int)t0);
				if (t1) atomicAdd(&S->c.nTouching, (int)t1);
				// COMPACT: the other half holds the survivors, in order; every workgroup has read the count and the live half
				if (COMPACT)
				{
					S->c.nContacts = n - (int)t0;
					S->cur = 1 - S->cur;
					if (ksOn)
					{
						// (every workgroup has read Counters::ksStale by now, and its atomics have landed before it arrived)
						const unsigned long long lost = __hip_atomic_exchange(W.arriveTree + (size_t)ARRIVE_COMPACT * TREE_WORDS, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						S->c.ksStats[KS_TOMBSTONES] += (unsigned long long)t0 - lost;
						if (lost) { S->c.ksStats[KS_NOT_FOUND] += lost; S->c.ksStale = 1; } // (a key that must be there is not: rebuild)
					}
				}
			}
			if (ORDER) toiOrderDestroy(W, s_raw);
		}
	}
