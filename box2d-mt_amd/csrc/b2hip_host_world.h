// b2hip_host_world.h - part of the ONE translation unit b2hip.hip (included there, nowhere else): the world behind the C ABI -
// error reporting, device arrays, the host's mirrors of bodies / fixtures / joints, struct b2hip_world with every switch the
// environment can set, the launch macros, capacity management, the proxy-id allocator (the uploads: b2hip_host_upload.h).
// (No include guard on purpose: b2hip.hip includes it exactly once, in order - the fragments share one scope.)

static thread_local std::string g_lastError;

static int setError(int code, const std::string& msg)
{
	g_lastError = msg;
	return code;
}

#define HIP_TRY(expr)                                                                                   \
	do                                                                                                  \
	{                                                                                                   \
		hipError_t _e = (expr);                                                                         \
		if (_e != hipSuccess)                                                                           \
		{                                                                                               \
			return setError(B2HIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
		}                                                                                               \
	} while (0)

// (set when librccl is opened, b2hip_shard_connect: releases a world's communicator)
static void (*g_rcclDestroy)(void* comm) = nullptr;

// Blocks that the two owner types below hold in this process right now (b2hip_test_storage).
static std::atomic<long long> g_liveBlocks{0};

// Device array that keeps its content when it grows and frees its block when it goes. Whoever lets one go drains the
// streams that use it first and has its device current (b2hip_world_destroy).
template <typename T>
struct DevArray
{
	T* p = nullptr;
	size_t cap = 0;
	DevArray() = default;
	DevArray(const DevArray&) = delete;
	DevArray& operator=(const DevArray&) = delete;
	~DevArray() { drop(p); }
	// the capacity ensure(n) leaves: 64 at least, doubled until n fits
	size_t capFor(size_t n) const
	{
		if (n <= cap) return cap;
		size_t ncap = cap ? cap : 64;
		while (ncap < n) ncap *= 2;
		return ncap;
	}
	int ensure(size_t n, hipStream_t stream, bool keep = true, bool zeroNew = true)
	{
		if (n <= cap) return 0;
		const size_t ncap = capFor(n);
		T* np = nullptr;
		HIP_TRY(hipMalloc((void**)&np, ncap * sizeof(T)));
		g_liveBlocks += 1;
		struct Fresh { T* q; ~Fresh() { drop(q); } } fresh = { np }; // (freed again on every way out but the last)
		if (zeroNew) HIP_TRY(hipMemsetAsync(np, 0, ncap * sizeof(T), stream));
		if (keep && p && cap) HIP_TRY(hipMemcpyAsync(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice, stream));
		if (p)
		{
			HIP_TRY(hipStreamSynchronize(stream));
			HIP_TRY(hipFree(p));
			g_liveBlocks -= 1;
		}
		fresh.q = nullptr;
		p = np;
		cap = ncap;
		return 0;
	}
private:
	static void drop(T* q)
	{
		if (q) { (void)hipFree(q); g_liveBlocks -= 1; }
	}
};

// Pinned host memory, typed, freed when its owner goes; dev is its device address where it was allocated mapped. Reads as the
// host pointer it holds.
template <typename T>
struct PinnedBuf
{
	T* p = nullptr;
	T* dev = nullptr;
	PinnedBuf() = default;
	PinnedBuf(const PinnedBuf&) = delete;
	PinnedBuf& operator=(const PinnedBuf&) = delete;
	~PinnedBuf() { free(); }
	// count elements, not initialised; what it held before is freed first
	int alloc(size_t count, unsigned flags)
	{
		free();
		HIP_TRY(hipHostMalloc((void**)&p, count * sizeof(T), flags));
		g_liveBlocks += 1;
		if (flags & hipHostMallocMapped) HIP_TRY(hipHostGetDevicePointer((void**)&dev, p, 0));
		return 0;
	}
	void free()
	{
		if (p) { (void)hipHostFree(p); g_liveBlocks -= 1; }
		p = dev = nullptr;
	}
	void swap(PinnedBuf& o) { std::swap(p, o.p); std::swap(dev, o.dev); }
	T* operator->() const { return p; }
	operator T*() const { return p; }
};

struct HostBody
{
	int type;
	uint32_t flags;
	float px, py, qs, qc;   // m_xf
	float cx, cy, a;        // m_sweep.c, a
	float c0x, c0y, a0;
	float lcx, lcy;         // m_sweep.localCenter
	float vx, vy, w;
	float fx, fy, torque;
	float mass, I, invMass, invI;
	float linearDamping, angularDamping, gravityScale;
	float sleepTime;
	int worldIndex;   // slot in b2hip_world::nonStatic (the reference's m_nonStaticBodies), -1 for static bodies
	int dead;         // destroyed (b2World::DestroyBody): the id stays, the body takes no part in anything any more
	int resetSweep;   // SetTransform: the sweep origin (c0, a0) is rewritten from the host mirror at the next upload
	std::vector<int> fixtures; // creation order (the reference's list is newest first)
	bool dirty;
	uint32_t pullEpoch;  // == b2hip_world::mirrorEpoch: this row has been refreshed from (or is newer than) h_state
	uint32_t forceEpoch; // == b2hip_world::stepEpoch: fx, fy, torque were applied since the last step (auto-clear worlds)
	uint32_t forceDev;   // != 0: a batched write named the body at this stepEpoch, and its b_force row on the device is the newer
	                     // copy of fx, fy, torque (the read-back row does not carry them): fetched by the next pullBody
};

struct HostFixture
{
	int body;
	int shape;
	float density, friction, restitution;
	uint16_t categoryBits, maskBits;
	int16_t groupIndex;
	bool isSensor, thick;
	int proxyKey;
	float fat[4];
	bool dead;        // destroyed (b2Body::DestroyFixture / DestroyBody): the id stays, the proxy is gone
	bool noProxy;     // the body is inactive (b2Body::SetActive(false)): the fixture lives on without a broad-phase proxy
};

struct FreeUnit
{
	int leaf;
};

// What a queued joint edit uploads (uploadJointEdits). Every kind sends the six limit / motor members, JointRec::enableLimit up
// to collideConnected: the springs and the force / torque limits that the scalar setters write lie among them.
enum JointEditKind
{
	JOINT_EDIT_MEMBERS = 0, // those members and nothing else
	JOINT_EDIT_LIMITS = 1,  // ... and a zero into impulseZ: the limit impulse restarts
	JOINT_EDIT_ANCHORS = 2, // ... and localAnchorA up to enableLimit: anchors, offsets, lengths, a mouse joint's target and body mass
	JOINT_EDIT_DESTROY = 3  // ... and the type word, which says B2D_JOINT_DEAD
};
struct JointEdit { int joint, kind; };

// The host side of b2World::SolveTOI (b2hip_host_toi.h): what it keeps on the world, sorted by what it is.
struct ToiSwitches // read from the environment once, when the world is made (readSwitches)
{
	bool serialOnly = false;      // B2HIP_TOI_SERIAL: every event through the serial loop
	bool syncOnly = false;        // B2HIP_TOI_SYNC: always look at the first pass's census before choosing a path (phaseToiSync)
	bool noDomains = false;       // B2HIP_TOI_NO_DOMAINS: bullets / kinematic partners through the serial loop only
	bool noSpecDomains = false;   // B2HIP_TOI_NO_SPEC_DOMAINS=1: the component path always looks at the census first
	bool domWideOnly = false;     // B2HIP_TOI_DOM_WIDE=1: the components' event loops always get 512 lanes (comparison)
	bool assumeFreshGrid = false; // B2HIP_DEBUG_ASSUME_FRESH_GRID=1 (tests: the speculative component path's wrong-guess handling)
	bool why = false;             // B2HIP_TOI_WHY: why a parallel TOI path handed the phase to the serial loop, on stderr
};
struct ToiHints // what one step's phase leaves for the next ones: hysteresis and guesses
{
	int syncSticky = 0;         // steps for which the phase decides from a read-back again (see phaseToi)
	int gridSticky = 0;         // steps for which the TOI chains still get a rebuilt hash grid
	int domainsSticky = 0;      // steps for which the component-wise event loops' preparations start beside k_toi_first (phaseToiSync)
	int domWide = 0;            // steps for which the components' event loops get 512 lanes again (one of them met more candidate contacts than a wave has lanes)
	int lastToiList = 0;        // pending impacts of the last step that took the component path (sizes the speculative launches)
	bool gridFreshLast = false; // ... and whether its pair update had left the grid fresh (what the speculative flow assumes of the next)
	bool eventValid = false;    // b2hip_solve_toi has run in this world: phase stamp 12 is there (b2Profile::solveTOI)
};
// What this step's phase has done so far. Its flags are cleared by begin() and dropVerdict() alone; dropVerdict() is called by
// toiRunAgain (a second run starts), toiSettle (a queued path found nothing pending) and spAfterToi (a sharded rank is done).
struct ToiStep
{
	enum Path { None, Chains, Components, Serial }; // whose result stands: the chains' and the components' is a verdict still out
	Path path = None;             // (Counters::toiUnsafe, read back at the end of the step or carried by a sharded rank's header)
	bool ran = false;             // impacts were pending: the step's TOI counters are reported (b2hip_get_counters)
	bool speculative = false;     // the path was queued without the first pass's census (phaseToi): the end of the step reads what it would have said
	bool chainsHadGrid = false;   // path == Chains: they ran with the hash grid. Stored: toiSettle updates ToiHints::gridSticky, which decided it, before it asks
	bool specGridAssumed = false; // speculative components: queued on the guess of a fresh grid. Stored: the guess came from a hint and a switch
	bool snapshotTaken = false;   // the phase saved the state it started from; stays up through every second run, which goes back to the same state
	bool countersFresh = false;   // the device's TOI counters are still the zeros of k_step_begin (set there, not by begin())
	std::vector<int4> verdicts;   // this step's PreSolve answers per TOI log slot (the device's copy: DW::toiVerdict)

	bool verdictPending() const { return path == Chains || path == Components; }
	bool specComponents() const { return speculative && path == Components; } // the component path queued without its census
	bool hadGrid() const { return path == Components || (path == Chains && chainsHadGrid); } // (the components always have it)
	void dropVerdict() { path = None; speculative = false; }
	void begin() { dropVerdict(); ran = snapshotTaken = false; verdicts.clear(); } // a step's phase starts (solveToiImpl)
};
struct ToiStats // since the world was created; n[] in the order b2hip_debug_read 25 reports and documents it
{
	enum { ChainsQueued, ChainsCensus, ComponentsQueued, ComponentsCensus, SerialDirect, RedoLatePairs, GridRetry, SerialFallback, OverflowRerun, PreSolveRerun, N };
	long long n[N] = {};
	long long chainContacts = 0; // contacts created by the close-out of the parallel TOI chains
};

// ---- the device arrays that ensureCapacity sizes: X(type, name, count, keep, zeroNew), one line each ------------------------
// Three expansions - the members of b2hip_world, ensureCapacity's loop, and for the first list `d.name = w->name.p` - and
// b2hip_test_storage's check of the last. The counts are read inside ensureCapacity: z is its WorldSizes, w the world. An
// array whose name is not here is sized where it is used, or by hand at the top of ensureCapacity.
// WORLD_ARRAYS_DW: DW holds the array's pointer under the same name.
#define WORLD_ARRAYS_DW(X) \
	X(float4, b_pos, z.nb, true, true) \
	X(float4, b_pos0, z.nb, true, true) \
	X(float4, b_vel, z.nb, true, true) \
	X(float4, b_xf, z.nb, true, true) \
	X(float4, b_mass, z.nb, true, true) \
	X(float4, b_damp, z.nb, true, true) \
	X(float4, b_force, z.nb, true, true) \
	X(uint32_t, b_flags, z.nb, true, true) \
	X(int, b_wake, z.nb, true, true) \
	X(int, b_rowDirty, z.nb, true, true) \
	X(int, b_order, z.nb, true, true) \
	X(int, orderBody, z.nb, true, true) \
	X(int, bigRoots, SHARD_BIG_MAX, true, true) /* sharded worlds: roots of this step's big islands */ \
	X(float4, p_fat, z.np, true, true) \
	X(int, p_body, z.np, true, true) \
	X(int, p_shape, z.np, true, true) \
	X(int, p_key, z.np, true, true) \
	X(uint32_t, p_filter0, z.np, true, true) \
	X(int, p_filter1, z.np, true, true) \
	X(float2, p_mat, z.np, true, true) \
	X(int, b_proxyHead, z.nb, true, true) \
	X(int, p_next, z.np, true, true) \
	/* k_solver_snapshot (b2d_kernels_sweep_end.h): what a recovered solve goes back to; B2HIP_NO_RECOVER=1: one element each */ \
	X(RevoluteJoint, solveSnapJoints, w->recoverOn ? z.nj : 1, true, true) \
	X(GearRec, solveSnapGears, w->recoverOn ? z.ng : 1, true, true) \
	X(int, jadjStart, z.nb + 2, true, true) \
	X(int, jadj, 2 * w->joints.size() + 2, true, true) \
	X(int, rootJointStart, z.nb + 2, true, true) \
	X(int, rootJointCursor, z.nb, true, true) \
	X(int, lj_list, w->joints.size() + 2, true, true) \
	X(int, rootJointOkay, z.nb, true, true) \
	X(int, parent, z.nb, true, true) \
	X(int, rootSeed, z.nb, true, true) \
	X(int, rootBodies, z.nb, true, true) \
	X(int, rootContacts, z.nb, true, true) \
	X(int, rootJoints, z.nb, true, true) \
	X(int, rootIsland, z.nb, true, true) \
	X(int, deg, z.nb + 1, true, true) \
	X(int, adjStart, z.nb + 2, true, true) \
	X(int, adjCursor, z.nb, true, true) \
	X(int, adj, 2 * z.cc, true, true) \
	X(int2, adjSlot, z.cc, true, true) \
	X(int4, rootScanIn, z.nb + 1, true, true) \
	X(int4, rootScanOut, z.nb + 2, true, true) \
	X(int, si_root, z.nb + 1, true, true) \
	X(int, si_bodyStart, z.nb + 2, true, true) \
	X(int, si_contactStart, z.nb + 2, true, true) \
	X(int, si_wStart, z.nb + 2, true, true) \
	X(int, si_maxLevel, z.nb + 1, true, true) \
	X(int, si_bodies, z.nb, true, true) \
	X(int, si_contacts, z.cc, true, true) \
	X(int, si_level, z.cc, true, true) \
	X(int, si_stack, z.nb, true, true) \
	X(int, si_lastLevel, z.nb, true, true) \
	X(int, b_slot, z.nb, true, true) \
	X(int, b_island, z.nb, true, true) \
	X(int, chunkFirst, (z.nb + z.cc) / (TINY_CHUNK_LANES / 2) + 4, true, true) \
	X(int, li_bodies, z.nb, true, true) \
	X(int, li_contacts, z.cc, true, true) \
	X(int, li_roots, z.nb, true, true) \
	X(int, li_color, z.cc, true, true) \
	/* (colorSlot: the first 65 colour counters on a line each) */ \
	X(int, colorCount, z.cc + 2 + COLOR_SLOT_PADDED * COLOR_SLOT_STRIDE, true, true) \
	X(int, colorStart, z.cc + 2, true, true) \
	X(int, colorCursor, z.cc + 2 + COLOR_SLOT_PADDED * COLOR_SLOT_STRIDE, true, true) \
	X(int, li_sorted, z.cc, true, true) \
	X(int4, li_ref, z.cc, true, true) \
	X(uint32_t, bodyClaim, z.nb, true, true) \
	X(uint64_t, bodyColorMask, z.nb, true, true) \
	X(uint64_t, bodyActive, z.nb, true, true) \
	X(uint64_t, bodyRest, z.nb, true, true) \
	X(float4, b_posv, z.nb, true, true) \
	X(unsigned long long, evKey, z.cc, true, true) \
	X(int4, evInfo, z.cc, true, true) \
	X(int, uncolList, COLOR_SMALL_MAX, true, true) \
	X(int, compactList, COLOR_SMALL_MAX, true, true) \
	X(int, hubRowOf, z.cc, true, true) \
	X(int, hubList, z.cc, true, true) \
	X(float4, hubDelta, z.cc, true, true) \
	X(unsigned long long, hubMeta, 8, true, true) \
	X(unsigned long long, hubFirst, z.nb, true, true) \
	X(float4, solveSnapBody, w->recoverOn ? 6 * z.nb : 1, true, true) \
	X(float4, solveSnapImp, w->recoverOn ? z.cc : 1, true, true) \
	X(uint32_t, solveSnapCFlags, w->recoverOn ? z.cc : 1, true, true) \
	X(uint32_t, rootPen, ROOT_PEN_SLOTS * z.nb, true, true) \
	X(int, rootDone, z.nb, true, true) \
	X(uint32_t, rootSleepMin, z.nb, true, true) \
	X(float, lc, (size_t)LC_WORDS * z.cc, false, false) \
	X(float4, warmDelta, 4 * z.cc, false, false) /* per-step scratch: k_large_init -> k_large_warm */ \
	X(int, moveBuf, 2 * z.np + 64, true, true) \
	X(int, gridCount, z.gridSize, true, true) \
	X(int, gridStart, z.gridSize + 2, true, true) \
	X(int, gridCursor, z.gridSize, true, true) \
	X(int, gridItems, z.np, true, true) \
	X(float4, gridFat, z.np, true, true) \
	X(unsigned long long, arriveTree, (size_t)ARRIVE_SITES * TREE_WORDS, true, true) \
	X(int, largeProxies, z.np, true, true) \
	X(int, largeMoves, 2 * z.np + 64, true, true) \
	X(uint64_t, pairKey, z.capPairs, true, true) \
	X(uint64_t, pairKey2, z.capPairs, true, true) \
	X(int2, pairProxy, z.capPairs, true, true) \
	X(int2, pairProxy2, z.capPairs, true, true) \
	X(int, pairFirst, z.capPairs + 1, true, true) \
	X(int, pairRank, z.capPairs + 2, true, true) \
	X(int, radixHist, RADIX_DIGITS * z.radixTiles + 2, true, true) \
	X(int, scanTmp, 3 * (std::max(z.maxScanN, RADIX_DIGITS * z.radixTiles) / SCAN_TILE + 8), true, true) \
	X(int, keepFlag, z.cc + 1, true, true) \
	X(int, keepScan, z.cc + 2, true, true) \
	X(int, toiList, z.cc, true, true) \
	X(int, toiPos2c, z.cc, true, true) \
	X(int, toiDestroyList, z.cc, true, true) \
	X(int, toiNewList, TOI_NEW_LIST_MAX, true, true) \
	X(int, b_toiGroup, z.nb, true, true) \
	X(int, toiGroups, z.nb, true, true) \
	X(int, toiGroupCount, std::min<size_t>(z.nb, TOI_GROUPS_MAX), true, true) \
	X(int, toiGroupList, std::min<size_t>(z.nb, TOI_GROUPS_MAX) * CHAIN_ADJ_MAX, true, true) \
	X(int, toiMoved, TOI_MOVED_ALL_MAX, true, true) \
	X(int, toiNew, 8 * TOI_NEWPAIR_MAX, true, true) \
	X(int, toiParent, z.nb, true, true) \
	X(int, toiDomOf, z.nb, true, true) \
	X(int, toiDomRoot, TOI_DOMAINS_MAX, true, true) \
	X(int, toiDomCount, TOI_DOMAINS_MAX, true, true) \
	X(int, toiDomBase, TOI_DOMAINS_MAX, true, true) \
	X(int, toiDomFill, TOI_DOMAINS_MAX, true, true) \
	X(int, toiDomFailed, TOI_DOMAINS_MAX, true, true) \
	X(int, toiDomEvents, TOI_DOMAINS_MAX, true, true) \
	X(int, toiDomList, z.cc, true, true) \
	X(float4, toiHull, z.np, true, true) \
	X(float4, snapBody, 5 * z.nb, true, true) \
	X(float4, snapFat, z.np, true, true) \
	/* listener bridge (nPre, nPost, nFil: contact-sized while the callback is installed) */ \
	X(float4, pre_o0, z.nPre, true, true) \
	X(float4, pre_o1, z.nPre, true, true) \
	X(float4, pre_oimp, z.nPre, true, true) \
	X(int4, pre_o3, z.nPre, true, true) \
	X(PreSolveRec, preRecs, z.nPre, true, true) \
	X(PostSolveRec, postRecs, z.nPost, true, true) \
	X(int, filterList, z.nFil, true, true) \
	/* block partition of the large islands (b2d_kernels_solve_blocks.h) */ \
	X(int, b_blk1, z.nb, true, true) \
	X(int, b_adopt, z.nb, true, true) \
	X(int, b_adoptStage, 3 * z.nb, true, true) \
	X(int, blkRows, (size_t)(MAX_BLOCKS + 2) * BLK_SLOT, true, true) \
	X(int, blkRowStart, MAX_BLOCKS + 2, true, true) \
	X(int, blkCursor, (size_t)(MAX_BLOCKS + 2) * BLK_SLOT, true, true) \
	X(int, blkBodyCount, (size_t)(MAX_BLOCKS + 2) * BLK_SLOT, true, true) \
	X(int, blkBodyCursor, (size_t)(MAX_BLOCKS + 2) * BLK_SLOT, true, true) \
	X(int, blkBodyStart, MAX_BLOCKS + 2, true, true) \
	X(int, blkBodies, z.nb, true, true) \
	X(int, rowColor, z.cc, true, true) \
	X(float4, b_cutv, z.nb, true, true) \
	/* spatial ownership (b2d_kernels_spatial.h; b2hip_shard_spatial): one element each in every other world */ \
	X(uint8_t, b_owner, w->spatial ? z.nb : 1, true, true) \
	X(uint8_t, spNewOwner, w->spatial ? z.nb : 1, true, true) \
	X(uint8_t, spAwake, w->spatial ? z.nb : 1, true, true) \
	X(int, spStraddle, w->spatial ? std::max<size_t>(w->spStraddle.cap, 4096) : 1, true, true) \
	X(int, spCount, w->spatial ? (size_t)SP_RESOLVE_MAX * SHARD_MAX_RANKS : 1, true, true) \
	X(int, spTarget, w->spatial ? SP_RESOLVE_MAX : 1, true, true) \
	X(int4, spTailKey, w->spatial ? z.capContacts : 1, true, true) \
	/* (+ the counters, behind the rows: one copy to the host per step) */ \
	X(float, stateOut, 12 * z.nb + sizeof(DState) / sizeof(float) + 4, true, true)

// WORLD_ARRAYS_HOST: DW does not hold it - the host alone hands it to the kernels that use it - or holds its pointer only
// under a condition, written behind the binds (toiLog, toiVerdict).
#define WORLD_ARRAYS_HOST(X) \
	X(int, radixHistScan, RADIX_DIGITS * z.radixTiles + 4, true, true) \
	X(int4, scanTmp4, 3 * (z.maxScanN / SCAN_TILE + 8), true, true) \
	/* status words of the single-pass scans (b2d_scan.h); a grown array keeps its words: the epoch goes on (scanCtx) */ \
	X(int, scanFlags, std::max(z.maxScanN, RADIX_DIGITS * z.radixTiles) / SCAN_TILE + 8, true, true) \
	/* status words of the one-launch radix passes (b2d_scan.h) for the pair buffers' tiles up to RADIX_ONEPASS_MAX_TILES (a sort */ \
	/* over more takes the three-launch form), and the sorts' two global digit histograms. Here and for k_collide's words below */ \
	/* a grown array starts from zeroed words under the running tag, which no word carries yet. */ \
	X(unsigned, radixCounts, z.onepassTiles * RADIX_DIGITS, false, true) \
	X(unsigned, radixGroups, z.onepassTiles ? (z.onepassTiles / RADIX_GROUP + 1) * RADIX_DIGITS : 0, false, true) \
	X(int, radixGlobalHist, z.onepassTiles ? 2 * RADIX_MAX_PASSES * RADIX_DIGITS : 0, true, true) \
	/* status words of k_collide<0, false, true>, a chunk's count / a group's sum each, for every chunk of the contact array */ \
	X(unsigned, collideCounts, z.collideChunks, false, true) \
	X(unsigned, collideGroups, z.collideChunks ? z.collideChunks / COLLIDE_GROUP + 2 : 0, false, true) \
	X(ToiLogRec, toiLog, listenerOn(w) && w->def.continuous ? z.cc : 1, true, true) \
	/* PreSolve answers for the TOI phase's log slots (DW::toiVerdict) */ \
	X(int4, toiVerdict, hasPreSolve(w) && w->def.continuous ? z.cc : 1, true, true) \
	/* indices uploaded by the host: contacts to disable / reject, pairs to drop (PreSolve material edits: 4 words each) */ \
	X(int, hostList, std::max<size_t>(std::max(4 * z.nPre, z.nFil), hasFilter(w) ? z.capPairs : 1), true, true) \
	/* body pairs a TOI event would have joined over an ownership boundary (k_sp_tail_pairs) */ \
	X(int2, spVirt, w->spatial ? SP_TAIL_MAX + 1 : 1, true, true) \
	X(int, consts, 16, true, true) /* [0] nBodies, [1] gridSize, [2] radix hist count, [3] sorted-pair count */ \
	X(int, gridBar, 32, true, true) /* grid barrier state of the persistent solver */

struct b2hip_world
{
	b2hip_world_def def = {};
	int device = -1;
	hipStream_t stream = nullptr;
	bool debugSync = false;

	std::vector<HostBody> bodies;
	std::vector<HostFixture> fixtures;
	std::vector<ShapeRec> shapes;
	std::map<std::string, int> shapeIndex;
	std::vector<RevoluteJoint> joints;

	// proxy id allocator (b2DynamicTree::AllocateNode / FreeNode, b2DynamicTree.cpp:53-99)
	int nextNode = 0;
	int leafCount = 0;
	std::vector<FreeUnit> freeUnits;

	// what has been uploaded so far
	size_t upBodies = 0, upFixtures = 0, upShapes = 0, upJoints = 0;
	std::vector<int> pendingMoves;
	std::vector<int> dirtyList;   // bodies whose host mirror is newer than the device rows
	std::mutex dirtyMutex;        // the per-body setters may run on several user threads, one body each (ManyBodies.h:39-64)
	size_t stateCount = 0;        // bodies covered by the last read-back in h_state
	uint32_t mirrorEpoch = 1;     // bumped by every read-back into h_state (HostBody::pullEpoch)
	uint32_t stepEpoch = 1;       // bumped by every step (HostBody::forceEpoch)
	bool newFixture = false;
	float inv_dt0 = 0.0f;
	bool stepActive = false;
	bool callbackWindow = false;  // inside the step, while the PreSolve callbacks run: mutators are accepted (and applied right after)
	bool failed = false;          // a step failed half-way: the device state is inconsistent, every later call says so
	std::string failedWhy;
	StepParams sp = {};

	// device: the kernarg block, the arrays of the two tables, and the ones ensureCapacity sizes by hand - the state block, the
	// tables whose names differ from DW's (shapes, joints, gears), the two sets of contact arrays, the contact-key set
	DW dw = [] { DW d = {}; d.cellSize = d.invCellSize = 1.0f; return d; }();
#define X(T, name, count, keep, zeroNew) DevArray<T> name;
	WORLD_ARRAYS_DW(X)
	WORLD_ARRAYS_HOST(X)
#undef X
	DevArray<DState> d_state;
	DevArray<ShapeRec> d_shapes;
	DevArray<RevoluteJoint> d_joints;
	DevArray<GearRec> d_gears;
	DevArray<int4> c_ids[2];
	DevArray<uint64_t> c_key[2];
	DevArray<uint32_t> c_flags[2];
	DevArray<float4> c_mat[2], c_man0[2], c_man1[2], c_imp[2];
	DevArray<int4> c_man3[2];
	DevArray<int> c_color[2], c_mgr[2];
	DevArray<uint64_t> ht_keys;
	std::vector<std::pair<int, int> > pendingFilter; // body pairs whose contacts must be re-filtered (new joint)
	int nMouseJoints = 0;
	size_t jadjBodies = (size_t)-1, jadjJoints = (size_t)-1; // what the device's per-body joint lists were last built for
	std::vector<GearRec> gears;   // gear joints' own records, appended like joints (the device copy keeps the impulses)
	size_t upGears = 0;
	std::vector<JointEdit> jointEdits; // joints a setter changed since the last upload, in call order (queueJointEdit; uploadJointEdits)
	bool eventsOn = false;
	std::vector<b2hip_contact_event> events; // of the last step, in delivery order
	std::vector<b2hip_toi_callback> toiCallbacks; // listener calls of the last step's TOI sub-steps, in call order
	// batched queries (b2hip_api_query.h): the batch and its results on the device, a pinned staging buffer for the copies,
	// scan scratch of their own (the step's scan context reports a look-back failure into Counters::overflow); grown on demand
	DevArray<float4> qIn;
	DevArray<int> qCounts, qOffsets, qItems, qFlags, qScanWork, qScanWords, qWords;
	DevArray<b2hip_ray_hit> qHits;
	DevArray<b2hip_distance_hit> qDistances; // the records of the distance queries
	DevArray<unsigned long long> qKeys, qKeysWork; // b2hip_ray_cast_all: the hits' (fraction bits, fixture id) keys; the long-list sort's room
	DevArray<uint8_t> qAny;                  // b2hip_ray_cast_any
	DevArray<QueryPose> qPoses; // shape queries and casts: pose, shape index, translation per query
	DevArray<ShapeRec> qShapes; // ... and the call's query shapes (the GJK proxies point into this table)
	// per-body contact lists and totals (b2hip_api_body_contacts.h): body -> slot in the batch (-1: not asked for), the batch's
	// ids, two counters per slot ([0, n]: every contact, [n + 1, 2n + 1]: the touching ones), the records; the lists themselves
	// share qOffsets / qItems / qFlags and the scan scratch with the queries. bcSeen / bcEpoch: the host's duplicate check.
	DevArray<int> bcSlot, bcIds, bcCounts;
	DevArray<b2hip_body_contact> bcRecords;
	DevArray<b2hip_body_contact_total> bcTotals;
	std::vector<uint32_t> bcSeen;
	uint32_t bcEpoch = 0;
	// batched body writes and the state gather (b2hip_api_body_writes.h): the batch's records / the gathered rows on the device
	// (the ids share bcIds); forceDevCount: bodies whose force row on the device is newer than the host's (HostBody::forceDev)
	DevArray<float4> bwIn;
	DevArray<float2> bwRows;
	size_t forceDevCount = 0;
	// batched destruction and activation sets (b2hip_api_body_lifecycle.h): lcNamed a word per body, entry + 1 while a call runs
	// and 0 between calls; lcWords[0] the length of the call's list of contacts with a TOI slot (the list itself borrows the
	// pair update's key buffer); lifecycleSortMax: lists up to this long are sorted by one workgroup in LDS
	// (B2HIP_TEST_LIFECYCLE_SORT_MAX: fewer, so that a small world takes the radix sort); carriedEvent*: end events of contacts a
	// batch destroyed, delivered with the next step's
	DevArray<int> lcNamed, lcWords;
	int lifecycleSortMax = LIFECYCLE_SORT_MAX;
	long long statLifecycleLongSorts = 0;
	std::vector<unsigned long long> carriedEventKeys;
	std::vector<int4> carriedEventInfo;
	// batched fixture sets (b2hip_api_fixture_batch.h): fxNamed a word per fixture, entry + 1 while a call runs and 0 between
	// calls (the ids share bcIds, the records bwIn, the list's length lcWords[0], its sort lifecycleSortMax); fbSeen / fbEpoch: the
	// host's duplicate check; fixtureListRoom: room the first listing of a call gets (B2HIP_TEST_FIXTURE_LIST_ROOM; -1: all the
	// pair buffer has), so that a small world lists twice; the statistics of b2hip_debug_read 30
	DevArray<int> fxNamed;
	std::vector<uint32_t> fbSeen;
	uint32_t fbEpoch = 0;
	int fixtureListRoom = -1;
	long long statFixtureLongSorts = 0, statFixtureRelists = 0;
	// batched body property sets (b2hip_api_body_props.h) share all of the above: the ids in bcIds, the records in bwIn, the
	// names in lcNamed, lcWords[0] the list's length and lcWords[1] the census of b2hip_set_types' refit test;
	// statBodyPropRefits: batches of b2hip_set_types that ran as the loop of single calls because a proxy of a body that turns
	// static had left its fat AABB (b2hip_debug_read 32; believed unreachable)
	long long statBodyPropRefits = 0;
	// batched joints (b2hip_api_joint_batch.h): the gathered joint states on the device (the ids share bcIds, the motor edits
	// bwIn); jbSeen / jbEpoch: the host's duplicate check of a write call's joint ids
	DevArray<float4> jbOut;
	std::vector<uint32_t> jbSeen;
	uint32_t jbEpoch = 0;
	ScanFlags qScan = {};
	void* qPinned = nullptr;
	size_t qPinnedBytes = 0;
	void* shardComm = nullptr;   // ncclComm_t of a connected sharded world (b2hip_shard_connect)
	DevArray<int> shardSend, shardRecv; // this rank's slab / all ranks' slabs
	size_t shardExchangeBytes = 0;
	bool shardLoopback = false;  // B2HIP_SHARD_LOOPBACK=1: a communicator of ONE rank still runs export -> ncclAllGather -> import (self-test on a one-GPU box)
	// spatial ownership (b2d_kernels_spatial.h; b2hip_shard_spatial)
	bool spatial = false;
	bool spFullRows = false;       // B2HIP_SHARD_FULL_ROWS=1 / b2hip_shard_full_rows: every rank holds every body's current row
	int spRowCap = 1024, spProxyCap = 4096;
	int spIdle[6] = {0, 0, 0, 0, 0, 0}; // exchanges in a row in which a capacity was four times what any rank needed (spCapDecay) // lean E1: records per rank (grown alike on every rank when a header says so)
	DevArray<int> spSend, spRecv;
	std::vector<uint8_t> spOwners; // the owner table as the host last knew it (assignment; refreshed after every resolution)
	bool spOwnersDirty = false;    // owners assigned / bodies created since the table was uploaded
	float spBounds[SHARD_MAX_RANKS + 1] = {0}; // strips along x the owners were dealt by (bodies created later fall into them)
	b2hip_all_gather_fn gatherFn = nullptr; // the caller's all-gather (gloo, tests); null with a connected RCCL communicator
	void* gatherUser = nullptr;
	PinnedBuf<int> spHost;          // staging of the caller's all-gather
	const int* spSendWiped = nullptr; // == spSend.p: its header has been wiped by the last import launch (spPrepareSend)
	PinnedBuf<int> spHdrHost;       // mapped: [0] sequence number, [1] extra word, [2..] the headers of all ranks' slabs (spReadHeaders)
	int spHdrSeq = 0;
	PinnedBuf<int> spOwnHost;       // mapped: the packed rows of this rank's bodies (id + b2hip_body_state), written by k_end_step
	size_t spOwnCapRows = 0;
	size_t spHostWords = 0;
	int spPairCap = 2048, spToiBodyCap = 256, spToiProxyCap = 512; // (records per rank; grown alike on every rank when a header says so)
	int spOwned[SHARD_MAX_RANKS] = {0}, spOwnedProxies[SHARD_MAX_RANKS] = {0};
	long long spMigratedTotal = 0, spResolves = 0, spPairsSent = 0;
	size_t spBytesStep = 0;         // bytes this rank received in the exchanges of the last step
	int spContactsBeforeToi = 0, spToiOrderBefore = 0, spTailCap = 64;
	int spToiUnsafe = 0;            // this rank's Counters::toiUnsafe as its E4 header showed it
	bool spToiSettled = false;      // this step's phase has been through its fallback already
	// measurement hook (b2hip_shard_tape): the results of this rank's collectives kept in device memory / taken from another
	// world's tape instead of a collective - one rank of a sharded world stepped alone on one GPU (tools/gpu_spatial_share.py)
	bool spTapeRecord = false;
	std::vector<std::pair<int*, size_t> > spTape;
	b2hip_world* spTapeFrom = nullptr;
	size_t spTapeCursor = 0;
	long long spToiRedos = 0;
	size_t spUp = 0;                // bodies the device's owner table covers
	ScanFlags scanCtx = {};      // scanFlags with their epoch and the abort word (refreshed by ensureCapacity)
	RadixStatus radixCtx = {};   // radixCounts / radixGroups / radixGlobalHist with their tag (refreshed by ensureCapacity)
	bool sortOnepass = true;     // B2HIP_SORT_ONEPASS=0: every radix pass as three launches (histogram, scan, scatter)
	long long statSorts = 0, statSortsOnepass = 0; // radix sorts queued since the world was created / of them in the one-launch form (b2hip_debug_read 22)
	int dfEpoch = 0;
	bool noSideStream = false, profileDetail = false;
	int collideStage = -1;       // B2HIP_COLLIDE_STAGE=0 / 1: never / always stage the shape records through LDS (default: by the record count)
	int solidRoundsEnv = 0;      // B2HIP_SOLID_ROUNDS=1 / 2 / 4 / 8: the tile of the island build's passes over the contacts (x 256 contacts), else by the contact count
	int collideSplitEnv = -1;    // B2HIP_COLLIDE_SPLIT=0 / 1: k_collide with the TOI-order replay inside / as a launch of its own (four waves per SIMD), else by the contact count
	// k_collide<0, false, true> (b2d_kernels_collide.h): the narrow phase stores the compacted contact array itself
	bool collideCompactOn = true;  // B2HIP_COLLIDE_COMPACT=0: never (the scan of the keep flags and k_compact_contacts behind every narrow phase)
	int collideChunk = 256;        // contacts per workgroup of that form (B2HIP_TEST_COLLIDE_CHUNK: fewer, so that a small world has many chunks and groups of chunks)
	bool contactsKnown = false;    // h_dstate holds the contact count and the TOI slot count as they are on the device: true behind a step's last read-back and behind applyEditOps', false once a narrow phase or a pair update is queued
	unsigned collideEpoch = 0;     // tag of its last launch (16 bits, never 0; the status words: collideCounts, collideGroups)
	long long statCollideCompact = 0; // narrow phases that took that form since the world was created (b2hip_debug_read 24)
	// k_collide<0, false, true, true>: that form with the island build's union pass as its tail (b2d_kernels_collide.h, b2d_kernels_island.h)
	bool collideUnionOn = true;    // B2HIP_COLLIDE_UNION=0: never (k_island_union in every island build)
	bool forestUnited = false;     // this step's narrow phase seeded the forest and united the contacts, and nothing has been queued since that changes the contact array or the forest: set by phaseCollide, consumed by buildIslands, dropped by forestDrop()
	bool forestVoided = false;     // ... and stored the colours as k_color_check's first loop leaves them
	long long statUnionSkipped = 0; // island builds that ran no union pass over the contacts since the world was created (b2hip_debug_read 31)
	bool collideUniOff = false;  // B2HIP_COLLIDE_UNI=0: k_collide reads every shape record from memory (no staged pair of records)
	int collideSortEnv = -1;     // B2HIP_COLLIDE_SORT=0 / 1: k_collide never / always sorts the contacts of a tile by shape-pair class in LDS
	hipStream_t stream2 = nullptr; // small-island solver beside the large-island one
	hipEvent_t evFork = nullptr, evJoin = nullptr;
	DevArray<unsigned long long> filterPairs; // sorted body-pair keys of the joints created / destroyed since the last step
	std::vector<int> nonStatic;       // the reference's m_nonStaticBodies: body ids in its order (island seed order)
	bool orderDirty = false;
	// edits of existing fixtures / contacts between steps (b2d_kernels_edit.h)
	std::vector<int2> editOps;        // queued contact-array ops, in call order
	std::vector<int> proxyEdits;      // fixtures whose device proxy row (filter words, body) must be rewritten
	std::vector<int> fatEdits;        // ... and the ones among them whose fat AABB the host has moved (SetTransform)
	bool proxyListsStale = false;     // a fixture was destroyed: b_proxyHead / p_next need a rebuild
	DevArray<int2> d_editOps;
	// listener / filter bridge: user callbacks in the middle of a step (include/b2hip.h)
	b2hip_should_collide_fn filterFn = nullptr;
	void* filterUser = nullptr;
	bool refilterPending = false;   // some contact may carry CF_FILTER (joint created / destroyed, fixture re-filtered)
	b2hip_pre_solve_fn preSolveFn = nullptr;
	b2hip_pre_solve_batch_fn preSolveBatchFn = nullptr;
	b2hip_should_collide_batch_fn filterBatchFn = nullptr;
	void* preSolveUser = nullptr;
	bool postSolveOn = false;
	std::vector<b2hip_contact_impulse> postSolve; // of the last step, in delivery order
	// block partition of the large islands (b2d_kernels_solve_blocks.h)
	int blocksMaxWG = 0;         // co-resident workgroups of k_solve_blocks on this device (0 = do not use it)
	int sweepMaxWG[3] = { 0, 0, 0 }; // ... of k_blocks_sweep<256 / 512 / 1024>
	int hubWaves = 8;            // waves of k_large_hub (B2HIP_HUB_WAVES=1: one)
	bool sweepEnd = true;        // k_sweep_end closes every sweep of the launch-per-colour solver (B2HIP_NO_SWEEP_END=1: round 4's launches)
	bool sweepTail = true;       // ... and takes the small colours (B2HIP_NO_TAIL=1: a launch per colour)
	int tailRowsMax = 1024;      // a colour with at most this many rows in the step's census is a tail colour (B2HIP_TAIL_ROWS): one
	                             // round of the workgroup. Measured on the settled Tumbler (profiles/r05_b): a round costs the
	                             // workgroup ~4.5 us - the same chain of dependent loads a launch pays - so a colour of 8 000
	                             // rows is 9 rounds = 40 us against 5.8 us as a launch of its own (tail colours up to 8 192 rows:
	                             // 4.94 ms per step; none: 3.87; round 4's launches: 4.57)
	int freshColors = 0;         // colours the last colouring from scratch of a partition-less world needed (0: none yet); in the snapshot's hints
	bool freshColorsPending = false;
	bool forceOnDevice = true;   // some body's force / torque row on the device may be non-zero (set by uploads, reset by a clearing read-back): the
	                             // read-back of a large world skips untouched tiles only when there is nothing to clear in them
	int rowMarks = 1;            // the read-back behind an early launch looks at marked tiles only (DW::b_rowDirty; B2HIP_NO_ROW_MARKS=1: compares every row; B2HIP_ROW_MARKS_CHECK=1: compares every row AND fails the step if an unmarked one differs)
	bool rowsWentEarly = false;  // this step's rows left behind SynchronizeFixtures (startEarlyRows): the shadow is that state
	bool sweepStamps = false;    // B2HIP_SWEEP_STAMPS=1: k_sweep_end<1> leaves its phase stamps where the block solver's go (diagnostics)
	bool bodyWarm = true;        // the warm start of a launch-per-colour solve body by body in one launch (k_large_warm; B2HIP_NO_BODY_WARM=1: a sweep of launches)
	bool restFlow = true;        // the small colours of a sweep as data flow per body in one launch (k_large_rest; B2HIP_NO_REST=1: launches / tail)
	bool noHubBuild = false;     // B2HIP_NO_HUB_BUILD=1: the hub list by k_hub_flag + scan + k_hub_fill + k_hub_order (four launches) always
	bool noHubOrder = false;     // B2HIP_NO_HUB_ORDER=1: the hub rows in contact order (round 5)
	bool hubOrderAll = false;    // B2HIP_HUB_ORDER=1: ... ordered also where every hub row is swept lane after lane (B2HIP_HUB_WIDE=0 / B2HIP_HUB_SERIAL=1: comparison runs)
	bool recoverOn = true;       // a timed-out wait between workgroups of the large-island solver is recovered from (saved state back, the
	                             // solve once more launch by launch; B2HIP_NO_RECOVER=1: the step fails as in round 5)
	PinnedBuf<int> h_solverWord; // mapped, 16 words: [0] the overflow word behind the solver, [1] the publication's number (k_solver_status)
	int solverSeq = 0;
	int colorRecoveries = 0;     // steps whose colouring ran out of colours / of rounds and went on (swept in order / finished by the grid-wide rounds)
	int solverRecoveries = 0;    // solves run a second time so far (b2hip_get_counters: solver_recoveries)
	int sweepRowsMax = 60000;    // islands with joints / hubs above this many constraints run launch per colour, not k_blocks_sweep (B2HIP_SWEEP_ROWS_MAX)
	int restHub = 2;             // k_large_rest + k_sweep_end of a sweep as ONE launch (k_rest_hub; B2HIP_REST_HUB=0: two launches, 1: the velocity sweeps only)
	int restHubMaxWG = 0;        // co-resident workgroups of k_rest_hub (0: do not use it)
	int restMaxWG = 0;           // ... of k_large_rest (0: unknown)
	int restArrived = 0;         // workgroups of this step's fused launches that sweep rest rows (what the verdict of a position iteration waits for: bar[5])
	int restRowsMax = 65536;     // ... the highest colours that hold at most this many rows together (B2HIP_REST_ROWS). Measured on the
	                             // settled Tumbler (profiles/r05_i_rest_rows_sweep.txt: the solver family per step, 21 colours): none 2.06 ms /
	                             // 260 launches per step; 16 384 rows 2.01 / 236; 50 000 1.89 / 188; 80 000 1.86 / 164; 180 000 1.88 / 116 -
	                             // a hop costs more the more lanes poll
	long long launchCount = 0;   // kernels launched on the main stream so far (LAUNCH)
	long long familyLaunchesAtStart = 0; int familyLaunches = 0; // ... by the large-island solver family in the last step (timing mode 5)
	int largeHintSteps = 120;    // > 0: the world has had large islands lately (k_color_check / k_block_census run with the island build)
	int serialOrphansNext = 0;   // DW::serialOrphans of the next step
	int adoptSticky = 0;
	bool adoptPasses = false;    // the last step had orphan constraints (or made a partition): run k_block_adopt this step
	bool traceLaunches = false;  // B2HIP_TRACE_LAUNCHES=1 (with B2HIP_DEBUG): every kernel's name before the stream is drained behind it
	bool tracePartition = false; // B2HIP_TRACE_PARTITION=1: why a partition was made, on stderr
	bool traceRecovery = false;  // B2HIP_TRACE_RECOVERY=1: every recovery, on stderr
	bool handoverWhy = false;    // B2HIP_HANDOVER_WHY: the post mortem of a timed-out wait inside a block solver, on stderr
	bool shardTrace = false;     // B2HIP_SHARD_TRACE=1: the size of every all-gather of a spatially sharded world (rank 0), on stderr
	double stepDeadlineS = 300.0; // B2HIP_STEP_DEADLINE_S: a poll of the host gives up on a stream that stays busy this long
	int pollDelayUs = 0;         // B2HIP_TEST_POLL_DELAY_US: the host comes late to its census poll (tests)
	bool gridHalf = false;       // the hash grid's cell is half the limit: chosen from the candidates per moved proxy of the last pair update
	bool gridForced = false;     // B2HIP_GRID_HALF=0 / 1 fixes it
	int pairsLargeSticky = 0;    // steps for which the pair update still reads its pair count back before it sorts
	int recolorCountdown = 0;    // ... and steps until such islands are coloured afresh (phaseSolve)
	bool blocksTooBig = false;   // the large islands hold more constraints than any block solver takes: no partition (phaseSolve)
	bool noSweepBlocks = false;  // B2HIP_NO_SWEEP_BLOCKS=1: jointed / hub islands stay on the launch-per-colour kernels
	int dfWipedAt = 0;           // dfEpoch >> 14 at the last wipe of the hand-over rows
	int sweepSteps = 0;          // steps whose large islands went through k_blocks_sweep
	int blockLanes = 0;          // forced workgroup size of k_solve_blocks (B2HIP_BLOCK_LANES), 0 = chosen per partition
	bool noBlocks = false;       // B2HIP_NO_BLOCKS=1: no block partition (large islands through the launch-per-colour kernels)
	int blockSteps = 0;          // steps solved by k_solve_blocks (diagnostics)
	// What the last pass of the large-island solve decided before its first launch (LargePass: its LargePlan and the solver
	// choice it ran under), kept for b2hip_debug_read 27 - tests/plan_ref.py checks the device's tables against it.
	struct PlanRecord
	{
		long long passes = 0;      // passes run since the world was created (a recovered step runs two)
		int solver = -1;           // 0 a launch per colour, 1 k_solve_blocks, 2 k_blocks_sweep, 3 exact order (levels as colours); -1 none yet
		int safe = 0, restFirst = 0x7fffffff, tailFirst = 0, bigEnd = 0, useRest = 0, fuseHub = 0, blockSort = 0, hubWide = 0, serialOrphans = 0;
		int nColors = 0, hasHubs = 0, hasJoints = 0, hubBuildOne = 0, useSweepEnd = 0, leftoverApart = 0;
	} planRecord;

	// pinned host buffers (mapped and coherent where a kernel writes what the host polls: PinnedBuf::dev is the kernel's address)
	PinnedBuf<float> h_state;    // mapped: k_end_step writes the read-back into it
	int stateSeq = 0;            // sequence number of the last read-back asked for (awaitState)
	size_t h_stateCap = 0;
	PinnedBuf<DState> h_dstate;
	PinnedBuf<DState> h_pub2;    // ... and where k_color_small publishes the state behind the colouring (a buffer and a count of its own: pubSeq2)
	int pubSeq2 = 0;
	PinnedBuf<DState> h_pub;     // mapped: where k_block_census publishes the island census; polled by awaitCensus
	int pubSeq = 0;
	bool noCensusPoll = false;   // B2HIP_NO_CENSUS_POLL=1: copy + stream synchronisation instead (for comparison)
	bool noStatePoll = false;    // B2HIP_NO_STATE_POLL=1: the same for the read-back at the end of the step
	// b2hip_set_lazy_readback: a step ends with the counters only; the 40 B per body stay on the device until a body's state
	// is asked for (rowsPending: h_state's rows are older than the device's; fetched once, by whoever asks first)
	bool lazyReadback = false;
	std::atomic<bool> rowsPending{false};
	// The rows travel only where they differ from what the host's buffer holds: stateOut is the device's copy of h_state's rows
	// (k_end_step, rowMode), valid while these three are what they were when it was last written in full.
	const float* shadowDev = nullptr;
	const float* shadowHost = nullptr;
	size_t shadowRows = 0;
	// ... which lets most of a large world's rows leave early, behind SynchronizeFixtures, on a stream of their own while the
	// pair update and the TOI phase run (startEarlyRows); the launch at the end of the step sends what changed since.
	hipStream_t rowStream = nullptr;
	hipEvent_t rowFork = nullptr, rowJoin = nullptr;
	bool rowsForked = false, rowsEarlyPending = false;
	int earlyRowsMin = 65536;       // bodies from which the early launch pays (B2HIP_EARLY_ROWS_MIN; 0 = never)
	std::mutex rowsMutex;
	bool blocksThisStep = false; // the large islands of this step went through k_solve_blocks

	Counters last = {};   // counters of the last completed step
	int lastContacts = 0;
	float profile[13] = {};
	hipEvent_t ev[13] = {};
	float solverMs = 0.0f;
	double solverBytes = 0.0;
	int solverConstraints = 0, solverBodies = 0;
	int forceLarge = 0;
	// optional per-launch timing of the dominant solver kernel
	size_t pairCapHint = 0; // pair-buffer size asked for after an overflow (growPairBuffers)
	int constsUploaded[2] = { -1, -1 };
	int* constsUploadedAt = nullptr;
	// the host side of b2World::SolveTOI (b2hip_host_toi.h), by what kind of thing it is
	ToiSwitches toiSw;
	ToiHints toiHints;
	ToiStep toiStep;
	ToiStats toiStats;
	// b2World::SetSubStepping (b2World.h:183; b2World.cpp:1082-1086, 1668): with the flag on a step call solves one TOI event
	// and leaves the step open; the calls that follow run Collide and the next event but no island solve, until no event is left
	bool stepComplete = true;  // b2World::m_stepComplete
	bool stepSolves = true;    // this call runs Solve (it started from a complete step)
	bool kernelTimingLaunches = false, colorSmallPending = false;
	int hubSteps = 0;
	bool debugTrace = false;                           // B2HIP_TRACE=1: hash the body state after every solver stage
	std::vector<std::pair<std::string, uint64_t> > trace;
	DevArray<float4> dbgPreVel, dbgVel;
	DevArray<int> dbgLi;
	int kernelTiming = 0;
	long long ktUnitsA = 0, ktUnitsB = 0; // units behind the bandwidth kernels' byte counts (set by b2hip_set_kernel_timing_units)
	std::vector<hipEvent_t> ktEvents;
	int ktUsed = 0;      // events recorded this step (pairs)
	int ktKind = 0;      // 0 none, 1 k_large_velocity, 2 k_solve_small, 4 k_solve_blocks, 5 - 7 (ktBracket), 8 the solver family
	float ktMs = 0.0f;
	int ktLaunches = 0;
	double ktBytes = 0.0;
};

// Every entry point that touches the device runs with the world's device current and puts the caller's device back
// afterwards: two worlds on different GPUs in one process, or a step from another thread, stay on their own device.
struct DeviceGuard
{
	int prev = -1;
	bool switched = false;
	explicit DeviceGuard(int device)
	{
		if (device < 0 || hipGetDevice(&prev) != hipSuccess || prev == device) return;
		switched = hipSetDevice(device) == hipSuccess;
	}
	~DeviceGuard()
	{
		if (switched) (void)hipSetDevice(prev);
	}
	DeviceGuard(const DeviceGuard&) = delete;
	DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DEVICE_GUARD(w) DeviceGuard _deviceGuard((w)->device)

// ------------------------------------------------------------------------------------------------
static int nextPow2(size_t n)
{
	size_t p = 64;
	while (p < n) p <<= 1;
	return (int)p;
}

// The read-back buffer h_state IS the host mirror of the dynamic state; a HostBody is refreshed from it only
// when the host is about to edit that body (no O(bodies) host loop per step).
static void ensureRows(b2hip_world* w);

// The read-back row carries no forces: HostBody::fx, fy, torque are their only host copy, and the next upload of the body
// overwrites b_force from them. Behind a batched write (b2hip_api_body_writes.h) the device's row is the newer one - whatever
// it holds by now - and this brings it home, 16 bytes, when the host is about to edit the body. In an auto-clear world a step
// since the batch has cleared the row: the mark is dropped, and the zeros pullBody has just written are the truth.
static void pullForce(b2hip_world* w, int i)
{
	HostBody& b = w->bodies[i];
	const bool live = !w->def.auto_clear_forces || b.forceDev == w->stepEpoch;
	b.forceDev = 0u;
	{
		std::lock_guard<std::mutex> lock(w->dirtyMutex);
		w->forceDevCount -= 1;
	}
	if (!live) return;
	float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	DeviceGuard guard(w->device);
	hipError_t e = hipMemcpyAsync(&f, w->b_force.p + i, sizeof(float4), hipMemcpyDeviceToHost, w->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
	if (e != hipSuccess)
	{
		// (the force cannot be had: the world is as good as lost - every later call says why, as with ensureRows)
		w->failed = true;
		w->failedWhy = std::string("reading a body's force row: ") + hipGetErrorString(e);
		return;
	}
	b.fx = f.x; b.fy = f.y; b.torque = f.z;
}

static void pullBody(b2hip_world* w, int i)
{
	if ((size_t)i >= w->stateCount || w->h_state == nullptr) return;
	HostBody& b = w->bodies[i];
	if (b.pullEpoch != w->mirrorEpoch) ensureRows(w);
	// once pulled, the host row is the newer one until the next read-back (an upload in between - a contact read flushes
	// the edits made so far - does not make h_state any fresher)
	if (b.pullEpoch == w->mirrorEpoch) return;
	b.pullEpoch = w->mirrorEpoch;
	const float* o = w->h_state + 10 * (size_t)i;
	b.px = o[0]; b.py = o[1]; b.a = o[2];
	b.vx = o[3]; b.vy = o[4]; b.w = o[5];
	b.cx = o[6]; b.cy = o[7];
	uint32_t f;
	memcpy(&f, o + 8, 4);
	b.flags = (b.flags & ~0x7fu) | (f & 0x7fu);
	b.sleepTime = o[9];
	b.c0x = b.cx; b.c0y = b.cy; b.a0 = b.a;
	b.qs = sinf(b.a);
	b.qc = cosf(b.a);
	if (w->def.auto_clear_forces && b.forceEpoch != w->stepEpoch) { b.fx = b.fy = b.torque = 0.0f; }
	b.forceEpoch = w->stepEpoch;
	if (b.forceDev != 0u) pullForce(w, i);
}

// Whoever copies the HostBody rows out as they are (the snapshot) pulls the bodies whose forces live on the device first.
static void pullDeviceForces(b2hip_world* w)
{
	for (size_t i = 0; i < w->bodies.size() && w->forceDevCount > 0; ++i)
		if (w->bodies[i].forceDev != 0u && !w->bodies[i].dirty) pullBody(w, (int)i);
}

static void markDirty(b2hip_world* w, int i)
{
	HostBody& b = w->bodies[i];
	if (b.dirty) return;
	pullBody(w, i);
	b.dirty = true;
	std::lock_guard<std::mutex> lock(w->dirtyMutex);
	w->dirtyList.push_back(i);
}

// b2Body::SetAwake(true) (b2Body.h:690-718): the flag is set and the sleep timer restarts whether the body was asleep or not
// (a slowly dragged mouse joint keeps its body awake this way). A static body's timer is never read: only its flag matters.
static void setAwake(b2hip_world* w, int i)
{
	if (w->bodies[i].type == B2HIP_STATIC_BODY && (w->bodies[i].flags & BF_AWAKE) != 0) return;
	markDirty(w, i);
	HostBody& b = w->bodies[i];
	b.flags |= BF_AWAKE;
	b.sleepTime = 0.0f;
}

// The host's row of a body that is about to be edited: current, and queued for the next upload.
static HostBody& editBody(b2hip_world* w, int i)
{
	markDirty(w, i);
	return w->bodies[i];
}

static void queueJointEdit(b2hip_world* w, int joint, int kind)
{
	w->jointEdits.push_back(JointEdit{ joint, kind });
}

// The ids the reference's b2DynamicTree hands out (AllocateNode / FreeNode, b2DynamicTree.cpp:53-99): a LIFO free list of
// node ids in front of a growing pool. CreateProxy takes one node for the leaf and - unless the tree is empty - InsertLeaf
// one more for the new internal parent; DestroyProxy gives back the parent RemoveLeaf drops (unless the leaf was the root)
// and then the leaf, so the next CreateProxy reuses exactly that leaf id. Which id the internal node had is never
// observable (only leaves are proxies): it sits in the list as a marker (-1).
static int allocProxyKey(b2hip_world* w)
{
	int key;
	if (!w->freeUnits.empty())
	{
		key = w->freeUnits.back().leaf;
		if (key < 0) return -1; // an internal node's id would become a leaf id (the tree was emptied and refilled): not modelled
		w->freeUnits.pop_back();
		if (w->leafCount > 0)
		{
			// InsertLeaf's parent node comes off the free list as well, or from the pool
			if (!w->freeUnits.empty()) w->freeUnits.pop_back();
			else w->nextNode++;
		}
	}
	else
	{
		key = w->nextNode++;
		if (w->leafCount > 0) w->nextNode++; // the internal parent node InsertLeaf allocates
	}
	w->leafCount++;
	return key;
}

// b2DynamicTree::DestroyProxy (b2DynamicTree.cpp:121-128): RemoveLeaf frees the parent (if the leaf is not the root), then the leaf
static void freeProxyKey(b2hip_world* w, int key)
{
	FreeUnit u;
	if (w->leafCount > 1)
	{
		u.leaf = -1;
		w->freeUnits.push_back(u);
	}
	u.leaf = key;
	w->freeUnits.push_back(u);
	w->leafCount--;
}

static int internShape(b2hip_world* w, const ShapeRec& s)
{
	std::string bytes((const char*)&s, sizeof(ShapeRec));
	std::map<std::string, int>::iterator it = w->shapeIndex.find(bytes);
	if (it != w->shapeIndex.end()) return it->second;
	int idx = (int)w->shapes.size();
	w->shapes.push_back(s);
	w->shapeIndex[bytes] = idx;
	return idx;
}

// Host evaluation of shape AABB / mass uses the same header the kernels use (b2d_collide.h), built
// for the host by hipcc; host libm sinf/cosf == b2dSin/b2dCos bit for bit (see b2d_math.h).
static Xf hostXf(const HostBody& b)
{
	Xf xf;
	xf.p = v2(b.px, b.py);
	xf.q.s = b.qs;
	xf.q.c = b.qc;
	return xf;
}

// fixture mass: the shared geometry module (b2d_shape_geom.h), the same routine the drop-in host shape classes call
static void shapeMass(const ShapeRec& s, float density, float* massOut, V2* centerOut, float* IOut)
{
	const MassProps mp = b2dShapeMass(&s, density);
	*massOut = mp.mass;
	*centerOut = mp.center;
	*IOut = mp.inertia;
}

// The mass data of a body: what b2Body::ResetMassData and SetMassData compute before they move the centre. The single calls and
// the batched ones (b2hip_api_body_props.h) both get theirs here.
struct BodyMass
{
	float mass, I, invMass, invI;
	V2 localCenter;
};

// b2Body::ResetMassData (b2Body.cpp:310-355): from the body's type, its fixtures' shapes and densities and its fixed-rotation flag
static BodyMass massFromFixtures(const b2hip_world* w, const HostBody& b)
{
	BodyMass m;
	m.mass = 0.0f;
	m.invMass = 0.0f;
	m.I = 0.0f;
	m.invI = 0.0f;
	m.localCenter = v2(0.0f, 0.0f);
	if (b.type == B2HIP_STATIC_BODY || b.type == B2HIP_KINEMATIC_BODY) return m;
	// the reference walks its fixture list newest first
	for (int k = (int)b.fixtures.size() - 1; k >= 0; --k)
	{
		const HostFixture& f = w->fixtures[b.fixtures[k]];
		if (f.density == 0.0f) continue;
		float mass, I;
		V2 center;
		shapeMass(w->shapes[f.shape], f.density, &mass, &center, &I);
		m.mass += mass;
		m.localCenter += mass * center;
		m.I += I;
	}
	if (m.mass > 0.0f)
	{
		m.invMass = 1.0f / m.mass;
		m.localCenter *= m.invMass;
	}
	else
	{
		m.mass = 1.0f;
		m.invMass = 1.0f;
	}
	if (m.I > 0.0f && (b.flags & BF_FIXEDROT) == 0)
	{
		m.I -= m.mass * b2dDot(m.localCenter, m.localCenter);
		m.invI = 1.0f / m.I;
	}
	else
	{
		m.I = 0.0f;
		m.invI = 0.0f;
	}
	return m;
}

// b2Body::SetMassData (b2Body.cpp:398-413) for a dynamic body: a mass that is not positive becomes 1, the inertia is taken only
// if it is positive and the rotation is not fixed
static BodyMass massFromData(const HostBody& b, const b2hip_mass_data* md)
{
	BodyMass m;
	m.I = 0.0f;
	m.invI = 0.0f;
	m.mass = md->mass;
	if (m.mass <= 0.0f) m.mass = 1.0f;
	m.invMass = 1.0f / m.mass;
	m.localCenter = v2(md->local_center[0], md->local_center[1]);
	if (md->inertia > 0.0f && (b.flags & BF_FIXEDROT) == 0)
	{
		m.I = md->inertia - m.mass * b2dDot(m.localCenter, m.localCenter);
		m.invI = 1.0f / m.I;
	}
	return m;
}

// the host-only part of a body's mass data (the device keeps invMass, invI and the local centre in b_mass)
static void storeMass(HostBody& b, const BodyMass& m)
{
	b.mass = m.mass;
	b.I = m.I;
	b.invMass = m.invMass;
	b.invI = m.invI;
	b.lcx = m.localCenter.x;
	b.lcy = m.localCenter.y;
}

// ... and what follows on a current host row: the centre moves with the local centre, and the velocity of the centre with it
// (b2Body.cpp:374-384, 415-423); a static or kinematic body's centre is its origin (:325-331)
static void moveCenter(HostBody& b)
{
	if (b.type == B2HIP_STATIC_BODY || b.type == B2HIP_KINEMATIC_BODY)
	{
		b.c0x = b.cx = b.px;
		b.c0y = b.cy = b.py;
		b.a0 = b.a;
		return;
	}
	V2 oldCenter = v2(b.cx, b.cy);
	V2 c = b2dMulXV(hostXf(b), v2(b.lcx, b.lcy));
	b.c0x = b.cx = c.x;
	b.c0y = b.cy = c.y;
	V2 dv = b2dCrossSV(b.w, c - oldCenter);
	b.vx += dv.x;
	b.vy += dv.y;
}

// b2Body::ResetMassData (b2Body.cpp:310-385)
static void resetMassData(b2hip_world* w, HostBody& b)
{
	storeMass(b, massFromFixtures(w, b));
	moveCenter(b);
}

// ------------------------------------------------------------------------------------------------
static int syncCheck(b2hip_world* w, const char* what)
{
	if (!w->debugSync) return 0;
	if (w->traceLaunches) { fprintf(stderr, "[b2hip] %s\n", what); fflush(stderr); } // (B2HIP_TRACE_LAUNCHES=1: which launch hangs?)
	hipError_t e = hipStreamSynchronize(w->stream);
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return setError(B2HIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
	return 0;
}

// b2Profile without events: stampPhase(w, k) asks the NEXT kernel launched on the main stream to note the device clock in
// DState::phaseClock[k] as it starts (b2dPhaseStamp, first statement of every kernel that takes the DW block).
static inline void stampPhase(b2hip_world* w, int slot)
{
	if (w->profileDetail) w->dw.stampMask |= 1u << slot;
}

template <typename A, typename... R>
static inline void stampsTaken(b2hip_world* w, const A&, const R&...)
{
	if (std::is_same<typename std::decay<A>::type, DW>::value) w->dw.stampMask = 0u;
}

// A launch that the runtime refuses (bad configuration, wrong device current, lost context) is reported at once:
// hipGetLastError needs no synchronisation. With B2HIP_DEBUG the stream is drained after every launch as well.
#define LAUNCH(w, kernel, grid, block, ...)                                                   \
	do                                                                                        \
	{                                                                                         \
		hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (w)->stream, __VA_ARGS__);     \
		(w)->launchCount += 1;                                                                \
		stampsTaken((w), __VA_ARGS__);                                                        \
		hipError_t _le = hipGetLastError();                                                   \
		if (_le != hipSuccess) return setError(B2HIP_ERR_HIP, std::string(#kernel) + " launch: " + hipGetErrorString(_le)); \
		int _rc = syncCheck((w), #kernel);                                                    \
		if (_rc) return _rc;                                                                  \
	} while (0)

// Same on an explicit stream (the small-island side stream, see phaseSolve).
#define LAUNCH_ON(w, strm, kernel, grid, block, ...)                                          \
	do                                                                                        \
	{                                                                                         \
		const uint32_t _sm = (w)->dw.stampMask;                                               \
		if ((strm) != (w)->stream) (w)->dw.stampMask = 0u; /* phase stamps belong to the main stream */ \
		hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (strm), __VA_ARGS__);          \
		if ((strm) != (w)->stream) (w)->dw.stampMask = _sm; else stampsTaken((w), __VA_ARGS__); \
		hipError_t _le = hipGetLastError();                                                   \
		if (_le != hipSuccess) return setError(B2HIP_ERR_HIP, std::string(#kernel) + " launch: " + hipGetErrorString(_le)); \
		if ((w)->debugSync)                                                                   \
		{                                                                                     \
			hipError_t _e = hipStreamSynchronize(strm);                                       \
			if (_e == hipSuccess) _e = hipGetLastError();                                     \
			if (_e != hipSuccess) return setError(B2HIP_ERR_HIP, std::string(#kernel) + ": " + hipGetErrorString(_e)); \
		}                                                                                     \
	} while (0)

static inline bool hasFilter(const b2hip_world* w) { return w->filterFn != nullptr || w->filterBatchFn != nullptr; }
static inline bool hasPreSolve(const b2hip_world* w) { return w->preSolveFn != nullptr || w->preSolveBatchFn != nullptr; }
// any listener callback switched on: the TOI sub-steps log their calls (b2hip_get_toi_callbacks) and run in serial order
static inline bool listenerOn(const b2hip_world* w) { return w->eventsOn || hasPreSolve(w) || w->postSolveOn; }

// a manifold as the listener records carry it (PreSolveRec, ToiLogRec), for the callbacks
static void toManifold(b2hip_manifold* m, float4 m0, float4 m1, float4 imp, int4 m3)
{
	m->type = m3.z;
	m->point_count = m3.w;
	m->local_normal[0] = m0.x; m->local_normal[1] = m0.y;
	m->local_point[0] = m0.z; m->local_point[1] = m0.w;
	m->point_local[0][0] = m1.x; m->point_local[0][1] = m1.y;
	m->point_local[1][0] = m1.z; m->point_local[1][1] = m1.w;
	m->normal_impulse[0] = imp.x; m->tangent_impulse[0] = imp.y;
	m->normal_impulse[1] = imp.z; m->tangent_impulse[1] = imp.w;
	m->id_key[0] = (uint32_t)m3.x;
	m->id_key[1] = (uint32_t)m3.y;
}

static int ktRecord(b2hip_world* w)
{
	if (!w->kernelTiming) return 0;
	if ((size_t)w->ktUsed >= w->ktEvents.size())
	{
		hipEvent_t e;
		HIP_TRY(hipEventCreate(&e));
		w->ktEvents.push_back(e);
	}
	HIP_TRY(hipEventRecord(w->ktEvents[w->ktUsed++], w->stream));
	return 0;
}

// The record that this step's narrow phase united the contacts (b2hip_world::forestUnited) is dropped by whatever queues a
// narrow phase, a pair update, a compaction or any other change of the contact array or of parent / deg behind it - and by
// the start of a step: an island build never finds a forest that is not its own contacts'.
static void forestDrop(b2hip_world* w)
{
	w->forestUnited = false;
	w->forestVoided = false;
}

// b2hip_set_kernel_timing modes 2 / 3 / 4: an event pair around k_collide / k_sync_fixtures / k_find_pairs_small
static int ktBracket(b2hip_world* w, int mode, int kind)
{
	if (w->kernelTiming != mode) return 0;
	w->ktKind = kind;
	return ktRecord(w);
}

static int gridFor(size_t n, int block = 256, int maxBlocks = 2048)
{
	size_t g = (n + block - 1) / block;
	if (g < 1) g = 1;
	if (g > (size_t)maxBlocks) g = maxBlocks;
	return (int)g;
}

static int readState(b2hip_world* w)
{
	HIP_TRY(hipMemcpyAsync(w->h_dstate, w->d_state.p, sizeof(DState), hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	return 0;
}

// The island census as k_block_census published it under sequence number w->pubSeq (straight into pinned host memory):
// the host polls the number instead of queueing a copy and synchronising the stream - which also lets the stream run on
// (k_color_small, queued behind the census) while the host sizes the solver launches.
// The polling loop of awaitCensus / awaitState: until *seq == want. Like hipStreamSynchronize it waits as long as the stream
// is busy (a step of a pathological world can take a minute); it gives up only if the stream reports an error, or has
// drained and the number still is not there two seconds later (the publishing kernel did not run: a bug, not a wait).
static int pollPublished(b2hip_world* w, volatile const int* seq, int want, const char* what)
{
	bool drained = false;
	std::chrono::steady_clock::time_point drainedAt;
	// ... and, as a backstop, after a generous wall-clock deadline (B2HIP_STEP_DEADLINE_S, default 300 s): every device-side
	// wait is bounded (PERSIST_SPIN_MAX, SCAN_SPIN_MAX), so a stream that stays busy that long is lost, and the caller gets an
	// error and a failed world instead of a Step() that never returns.
	const auto startedAt = std::chrono::steady_clock::now();
	for (unsigned spins = 1; *seq != want; ++spins)
	{
		if ((spins & 0x3fff) == 0)
		{
			const hipError_t q = hipStreamQuery(w->stream);
			if (q != hipSuccess && q != hipErrorNotReady) return setError(B2HIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(q));
			if (q == hipSuccess)
			{
				const auto now = std::chrono::steady_clock::now();
				if (!drained) { drained = true; drainedAt = now; }
				else if (now - drainedAt > std::chrono::seconds(2)) return setError(B2HIP_ERR_HIP, std::string(what) + " was not published (the stream has drained)");
			}
			else drained = false;
			if (std::chrono::duration<double>(std::chrono::steady_clock::now() - startedAt).count() > w->stepDeadlineS)
				return setError(B2HIP_ERR_HIP, std::string(what) + ": the device did not finish the step within the deadline (B2HIP_STEP_DEADLINE_S)");
		}
#if defined(__x86_64__)
		__builtin_ia32_pause();
#endif
	}
	std::atomic_thread_fence(std::memory_order_acquire);
	return 0;
}

// The state behind k_color_small (published into the second buffer with the number the host gave it).
static int awaitColors(b2hip_world* w)
{
	if (int rc = pollPublished(w, (volatile const int*)&w->h_pub2->pubSeq, w->pubSeq2, "colour state")) return rc;
	memcpy(w->h_dstate, w->h_pub2, offsetof(DState, pubSeq));
	return 0;
}

static int awaitCensus(b2hip_world* w)
{
	// (B2HIP_TEST_POLL_DELAY_US: the host comes late to its poll - what a descheduled thread does to it now and then;
	// tests/test_gpu_recovery.py: a second publication must not have overwritten the first by then)
	if (w->pollDelayUs > 0) std::this_thread::sleep_for(std::chrono::microseconds(w->pollDelayUs));
	if (int rc = pollPublished(w, (volatile const int*)&w->h_pub->pubSeq, w->pubSeq, "island census")) return rc;
	memcpy(w->h_dstate, w->h_pub, offsetof(DState, pubSeq));
	return 0;
}

// ---- the environment switches, read once per world by b2hip_world_create -------------------------------
static bool envSet(const char* k) { return getenv(k) != nullptr; } // any value
static bool envOn(const char* k) { const char* e = getenv(k); return e && atoi(e); } // a non-zero number
static int envInt(const char* k, int unset) { const char* e = getenv(k); return e ? atoi(e) : unset; }

static void readSwitches(b2hip_world* w)
{
	DW& d = w->dw;
	w->debugSync = envSet("B2HIP_DEBUG");
	w->traceLaunches = envSet("B2HIP_TRACE_LAUNCHES");
	w->debugTrace = envSet("B2HIP_TRACE");
	w->forceLarge = envInt("B2HIP_FORCE_LARGE", 0);
	w->kernelTimingLaunches = envSet("B2HIP_SOLVER_LAUNCHES"); // force the launch-per-colour solver
	w->noSideStream = envSet("B2HIP_NO_SIDE_STREAM");
	w->profileDetail = envInt("B2HIP_PROFILE_DETAIL", 1) != 0;
	if (const char* e = getenv("B2HIP_SOLID_ROUNDS")) { const int v = atoi(e); w->solidRoundsEnv = (v == 1 || v == 2 || v == 4 || v == 8) ? v : 0; }
	w->collideSplitEnv = envInt("B2HIP_COLLIDE_SPLIT", -1);
	w->collideCompactOn = envInt("B2HIP_COLLIDE_COMPACT", 1) != 0;
	w->collideUnionOn = envInt("B2HIP_COLLIDE_UNION", 1) != 0;
	w->collideChunk = std::min(std::max(envInt("B2HIP_TEST_COLLIDE_CHUNK", 256), 1), 256);
	w->lifecycleSortMax = std::min(std::max(envInt("B2HIP_TEST_LIFECYCLE_SORT_MAX", LIFECYCLE_SORT_MAX), 0), LIFECYCLE_SORT_MAX);
	w->fixtureListRoom = std::max(envInt("B2HIP_TEST_FIXTURE_LIST_ROOM", -1), -1);
	w->collideUniOff = envInt("B2HIP_COLLIDE_UNI", 1) == 0;
	w->collideSortEnv = envInt("B2HIP_COLLIDE_SORT", -1);
	w->sortOnepass = envInt("B2HIP_SORT_ONEPASS", 1) != 0;
	d.keysetKeep = envInt("B2HIP_KEYSET_KEEP", 1) != 0 ? 1 : 0;
	d.keysetMaxFill = std::min(std::max(envInt("B2HIP_KEYSET_MAX_FILL", 37), 1), 90); // (per cent; below 100 so that a probe always meets an empty slot)
	w->collideStage = envInt("B2HIP_COLLIDE_STAGE", -1);
	w->noSweepBlocks = envSet("B2HIP_NO_SWEEP_BLOCKS");
	w->tracePartition = envSet("B2HIP_TRACE_PARTITION");
	w->traceRecovery = envSet("B2HIP_TRACE_RECOVERY");
	if (const char* e = getenv("B2HIP_GRID_HALF")) { w->gridForced = true; w->gridHalf = atoi(e) != 0; d.gridHalf = w->gridHalf ? 1 : 0; }
	d.noChainCreate = envSet("B2HIP_TOI_NO_CHAIN_CREATE") ? 1 : 0;
	d.noOwnIdBlocks = envSet("B2HIP_NO_OWN_ID_BLOCKS") ? 1 : envSet("B2HIP_OWN_ID_BLOCKS_ALL") ? -1 : 0;
	w->noBlocks = envSet("B2HIP_NO_BLOCKS"); // no block partition at all (colours as before it existed)
	w->blockLanes = 0; // chosen per partition (see phaseSolve); B2HIP_BLOCK_LANES = 256 | 512 | 1024 forces one size
	if (const char* e = getenv("B2HIP_BLOCK_LANES")) w->blockLanes = atoi(e) == 512 ? 512 : (atoi(e) == 256 ? 256 : (atoi(e) == 1024 ? 1024 : 0));
	w->toiSw.serialOnly = envSet("B2HIP_TOI_SERIAL");
	w->toiSw.syncOnly = envSet("B2HIP_TOI_SYNC");
	w->toiSw.domWideOnly = envSet("B2HIP_TOI_DOM_WIDE");
	w->toiSw.noSpecDomains = envSet("B2HIP_TOI_NO_SPEC_DOMAINS");
	w->toiSw.assumeFreshGrid = envSet("B2HIP_DEBUG_ASSUME_FRESH_GRID");
	w->toiSw.noDomains = envSet("B2HIP_TOI_NO_DOMAINS");
	w->toiSw.why = envSet("B2HIP_TOI_WHY");
	w->handoverWhy = envSet("B2HIP_HANDOVER_WHY");
	w->shardTrace = envOn("B2HIP_SHARD_TRACE");
	w->recoverOn = !envOn("B2HIP_NO_RECOVER");
	w->noCensusPoll = envOn("B2HIP_NO_CENSUS_POLL");
	w->noStatePoll = envOn("B2HIP_NO_STATE_POLL");
	w->lazyReadback = envOn("B2HIP_LAZY_READBACK");
	w->earlyRowsMin = envInt("B2HIP_EARLY_ROWS_MIN", w->earlyRowsMin);
	w->stepDeadlineS = getenv("B2HIP_STEP_DEADLINE_S") ? atof(getenv("B2HIP_STEP_DEADLINE_S")) : 300.0;
	w->pollDelayUs = envInt("B2HIP_TEST_POLL_DELAY_US", 0);
	d.bigChunks = envSet("B2HIP_BIG_CHUNKS") ? 1 : 0;
	// Exact order costs ~1 us per DEPENDENT constraint (a GPU lane against a CPU core on a chain): a 210-box pyramid is
	// ~300 levels x 12 sweeps = 3.9 ms in k_solve_small, ~0.1 ms as one block of k_solve_blocks. Islands up to 128 (bodies
	// or contacts) are walked in the reference's order, bit-exact; B2HIP_SMALL_MAX_W (<= 512) moves the line.
	d.smallMaxW = TINY_ISLAND_MAX_W;
	if (const char* e = getenv("B2HIP_SMALL_MAX_W")) d.smallMaxW = std::max(1, std::min((int)SMALL_ISLAND_MAX_W, atoi(e)));
	d.noFreeBodies = envOn("B2HIP_NO_FREE_BODIES") ? 1 : 0;
	d.testMaxColors = envInt("B2HIP_TEST_MAX_COLORS", 0);
	d.testColorRounds = envInt("B2HIP_TEST_COLOR_ROUNDS", 0);
	d.testSpinMax = std::max(0, envInt("B2HIP_TEST_SPIN_MAX", 0));
	d.restPoll = getenv("B2HIP_REST_POLL") ? std::max(1, std::min(16, atoi(getenv("B2HIP_REST_POLL")))) : 1;
	d.hubSerial = envOn("B2HIP_HUB_SERIAL") ? 1 : 0;
	w->hubWaves = envInt("B2HIP_HUB_WAVES", 0) == 1 ? 1 : 8; // (1: the one-wave form, for comparison)
	// The end of a sweep over islands that run launch per colour - tail colours, hub rows, joints, the verdict of a position
	// iteration - in one single-workgroup launch (k_sweep_end). B2HIP_NO_SWEEP_END=1: the launches of round 4 (k_large_hub,
	// k_large_joints, k_large_pos_end); B2HIP_NO_TAIL=1: every colour a launch of its own; B2HIP_HUB_WIDE=0: the hub rows in
	// k_large_hub's order and scheme (chunks of 64) inside k_sweep_end - what the comparisons in tests/ use. Asking for a
	// number of hub waves or the serial hub sweep means k_large_hub.
	w->sweepEnd = !envOn("B2HIP_NO_SWEEP_END") && !envSet("B2HIP_HUB_WAVES");
	w->sweepTail = w->sweepEnd && !envOn("B2HIP_NO_TAIL");
	w->sweepStamps = envSet("B2HIP_SWEEP_STAMPS");
	w->rowMarks = envOn("B2HIP_ROW_MARKS_CHECK") ? 2 : envOn("B2HIP_NO_ROW_MARKS") ? 0 : 1;
	w->bodyWarm = !envOn("B2HIP_NO_BODY_WARM");
	w->restFlow = w->sweepEnd && !envOn("B2HIP_NO_REST");
	w->noHubBuild = envOn("B2HIP_NO_HUB_BUILD");
	w->noHubOrder = envOn("B2HIP_NO_HUB_ORDER");
	w->hubOrderAll = envOn("B2HIP_HUB_ORDER");
	if (getenv("B2HIP_SWEEP_ROWS_MAX")) w->sweepRowsMax = std::max(1, atoi(getenv("B2HIP_SWEEP_ROWS_MAX")));
	w->restHub = getenv("B2HIP_REST_HUB") ? std::max(0, std::min(2, atoi(getenv("B2HIP_REST_HUB")))) : 2;
	w->restRowsMax = getenv("B2HIP_REST_ROWS") ? std::min(atoi(getenv("B2HIP_REST_ROWS")), REST_ROWS_MAX - COLOR_SMALL_MAX) : 65536;
	w->tailRowsMax = envInt("B2HIP_TAIL_ROWS", SWEEP_END_LANES);
	d.hubWide = (w->sweepEnd && !d.hubSerial && envInt("B2HIP_HUB_WIDE", 1) != 0) ? 1 : 0;
}

// What ensureCapacity's counts are made of, worked out once per call: WorldSizes z = { w, needContacts }.
struct WorldSizes
{
	const b2hip_world* w;
	size_t needContacts;
	size_t nb = std::max<size_t>(w->bodies.size(), 1), np = std::max<size_t>(w->fixtures.size(), 1);
	size_t nj = std::max<size_t>(w->joints.size(), 1), ng = std::max<size_t>(w->gears.size(), 1);
	size_t capPairs = std::max<size_t>(std::max<size_t>(8 * np + 4096, w->pairKey.cap), w->pairCapHint);
	size_t capContacts = std::max<size_t>(needContacts + capPairs, 1024); // the contact arrays' room asked for ...
	size_t cc = w->c_ids[0].capFor(capContacts);                          // ... and the (power of two) capacity they get
	size_t gridSize = (size_t)nextPow2(2 * np);
	size_t maxScanN = std::max(std::max(nb + 2, gridSize + 2), std::max(cc + 2, capPairs + 2));
	size_t radixTiles = capPairs / RADIX_TILE + 2;
	// tiles / chunks the one-launch radix passes / k_collide<0, false, true> have status words for (0: switched off)
	size_t onepassTiles = w->sortOnepass ? std::min<size_t>(radixTiles, RADIX_ONEPASS_MAX_TILES) : 0;
	size_t collideChunks = w->collideCompactOn ? cc / (size_t)w->collideChunk + 2 : 0;
	// the listener arrays: contact-sized only while the callback that needs them is installed
	size_t nPre = hasPreSolve(w) ? cc : 1, nPost = w->postSolveOn ? cc : 1, nFil = hasFilter(w) ? cc : 1;
};

// Size every buffer for the current topology and a contact / pair budget; refresh the kernarg block.
static int ensureCapacity(b2hip_world* w, size_t needContacts)
{
	hipStream_t s = w->stream;
	const WorldSizes z = { w, needContacts };
	const size_t nb = z.nb;
	DW& d = w->dw;
	int rc = 0;
#define ENS(arr, n) do { rc = w->arr.ensure((n), s); if (rc) return rc; } while (0)
	ENS(d_state, 1);
	ENS(d_shapes, std::max<size_t>(w->shapes.size(), 1));
	ENS(d_joints, z.nj);
	ENS(d_gears, z.ng);
	d.shapes = w->d_shapes.p; d.joints = w->d_joints.p; d.gears = w->d_gears.p;
	for (int k = 0; k < 2; ++k)
	{
		ENS(c_ids[k], z.capContacts); ENS(c_key[k], z.capContacts); ENS(c_flags[k], z.capContacts); ENS(c_mat[k], z.capContacts);
		ENS(c_man0[k], z.capContacts); ENS(c_man1[k], z.capContacts); ENS(c_imp[k], z.capContacts); ENS(c_man3[k], z.capContacts);
		ENS(c_color[k], z.capContacts); ENS(c_mgr[k], z.capContacts);
		d.ca[k].ids = w->c_ids[k].p; d.ca[k].key = w->c_key[k].p; d.ca[k].flags = w->c_flags[k].p; d.ca[k].mat = w->c_mat[k].p;
		d.ca[k].man0 = w->c_man0[k].p; d.ca[k].man1 = w->c_man1[k].p; d.ca[k].imp = w->c_imp[k].p; d.ca[k].man3 = w->c_man3[k].p;
		d.ca[k].color = w->c_color[k].p; d.ca[k].mgr = w->c_mgr[k].p;
	}
#undef ENS
	// hash set: at most 50 % load
	{
		size_t want = (size_t)nextPow2(2 * z.cc);
		if (w->ht_keys.cap < want)
		{
			const bool had = w->ht_keys.cap != 0;
			rc = w->ht_keys.ensure(want, s, false);
			if (rc) return rc;
			// (the new table does not keep the old one's keys: a kept set is rebuilt by the next pair update)
			static const int one = 1;
			if (had) HIP_TRY(hipMemcpyAsync(&w->d_state.p->c.ksStale, &one, sizeof(int), hipMemcpyHostToDevice, s));
		}
	}
	d.ht_keys = w->ht_keys.p;
	// the two tables: every array sized, then DW's pointers set from the arrays
#define X(T, name, count, keep, zeroNew) if ((rc = w->name.ensure((count), s, (keep), (zeroNew)))) return rc;
	WORLD_ARRAYS_DW(X)
	WORLD_ARRAYS_HOST(X)
#undef X
#define X(T, name, count, keep, zeroNew) d.name = w->name.p;
	WORLD_ARRAYS_DW(X)
#undef X
	w->scanCtx.words = w->scanFlags.p;
	w->scanCtx.count = w->scanFlags.cap;
	w->scanCtx.abortWord = &w->d_state.p->c.overflow;
	w->radixCtx.counts = w->radixCounts.p; w->radixCtx.countsCap = w->radixCounts.cap;
	w->radixCtx.groups = w->radixGroups.p; w->radixCtx.groupsCap = w->radixGroups.cap;
	w->radixCtx.hist = w->radixGlobalHist.p;
	w->radixCtx.maxTiles = !w->sortOnepass ? 0 : (int)std::min<size_t>(
		std::min<size_t>(w->radixCounts.cap / RADIX_DIGITS, (w->radixGroups.cap / RADIX_DIGITS) * RADIX_GROUP), RADIX_ONEPASS_MAX_TILES);
	w->radixCtx.abortWord = &w->d_state.p->c.overflow;
	if (w->h_stateCap < 12 * nb + sizeof(DState) / sizeof(float) + 4)
	{
		// (the rows of the last read-back are the host's mirror of every body it has not edited: they move along)
		ensureRows(w);
		const size_t cap = 12 * nb * 2 + sizeof(DState) / sizeof(float) + 4;
		PinnedBuf<float> grown;
		rc = grown.alloc(cap, hipHostMallocMapped | hipHostMallocCoherent);
		if (rc) return rc;
		if (w->h_state) memcpy(grown, w->h_state, w->stateCount * 10 * sizeof(float));
		w->h_state.swap(grown); // (which takes the old buffer away with it)
		w->h_stateCap = cap;
	}

	d.st = w->d_state.p;
	d.nBodies = (int)w->bodies.size();
	d.nProxies = (int)w->fixtures.size();
	d.nJoints = (int)w->joints.size();
	d.nShapes = (int)w->shapes.size();
	d.capContacts = (int)z.cc;
	d.capPairs = (int)w->pairKey.cap;
	d.capMoves = (int)w->moveBuf.cap;
	d.htMask = (uint32_t)(w->ht_keys.cap - 1);
	d.gridMask = (uint32_t)(z.gridSize - 1);
	d.dfRank = nullptr; d.dfInbox = nullptr; d.eventsOn = w->eventsOn ? 1 : 0;
	d.spatial = w->spatial ? 1 : 0; d.spFullRows = w->spFullRows ? 1 : 0; d.capStraddle = (int)w->spStraddle.cap;
	if (w->spatial && w->spOwnCapRows < nb)
	{
		if (w->spOwnHost) HIP_TRY(hipStreamSynchronize(s));
		w->spOwnHost.free();
		w->spOwnCapRows = 2 * nb;
		rc = w->spOwnHost.alloc(w->spOwnCapRows * 11, hipHostMallocMapped | hipHostMallocCoherent);
		if (rc) return rc;
	}
	d.spOwnOut = w->spatial ? w->spOwnHost.dev : nullptr; d.spOwnCap = (int)w->spOwnCapRows;
	d.userFilter = hasFilter(w) ? 1 : 0; d.preSolveOn = hasPreSolve(w) ? 1 : 0; d.postSolveOn = w->postSolveOn ? 1 : 0;
	d.toiLog = listenerOn(w) && w->def.continuous ? w->toiLog.p : nullptr;
	d.capToiLog = (int)std::min<size_t>(w->toiLog.cap, 0x7fffff);
	d.toiVerdict = hasPreSolve(w) && w->def.continuous ? w->toiVerdict.p : nullptr;
	d.nToiVerdict = std::min((int)w->toiStep.verdicts.size(), (int)std::min<size_t>(w->toiVerdict.cap, 0x7fffff));
	return 0;
}

