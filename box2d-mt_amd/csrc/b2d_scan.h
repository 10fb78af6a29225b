// b2d_scan.h - device-wide exclusive scan and stable LSD radix sort, hand-written for wave64.
// Element counts live in device memory (the host never learns them mid-step), so every launch is
// sized by a capacity and blocks beyond the live count exit immediately.
#ifndef B2D_SCAN_H
#define B2D_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define SCAN_THREADS 256
#define SCAN_ITEMS 4
#define SCAN_TILE (SCAN_THREADS * SCAN_ITEMS)
#define SCAN_CHAIN_MAX_TILES 256 // single-pass scan up to 256 tiles: 256 K elements in tiles of 1 024, 1 M in tiles of 4 096; three kernels beyond
#define SCAN_ITEMS_WIDE 16
#define SCAN_TILE_WIDE (SCAN_THREADS * SCAN_ITEMS_WIDE)

__device__ __forceinline__ int scanAdd(int a, int b) { return a + b; }
__device__ __forceinline__ int4 scanAdd(int4 a, int4 b) { return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ void scanZero(int& a) { a = 0; }
__device__ __forceinline__ void scanZero(int4& a) { a = make_int4(0, 0, 0, 0); }
// Tile aggregates / prefixes handed from workgroup to workgroup of one launch: stores and loads that go past the XCD's L2
// (sc1), so the status words need no release / acquire (an agent-scope release writes the whole L2 back, an acquire
// invalidates it - per tile, and per spin of the look-back).
__device__ __forceinline__ void scanStoreAgent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int scanLoadAgent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void scanStoreAgent(int4* p, int4 v)
{
	typedef int i4 __attribute__((ext_vector_type(4)));
	i4 q;
	q.x = v.x; q.y = v.y; q.z = v.z; q.w = v.w;
	// (s_nop 1: the store's data registers must not be written by the next two instructions - see stRow in b2d_handover.h)
	asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(q) : "memory");
}
__device__ __forceinline__ int4 scanLoadAgent(const int4* p)
{
	typedef int i4 __attribute__((ext_vector_type(4)));
	i4 r;
	asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
	return make_int4(r.x, r.y, r.z, r.w);
}

// Exclusive scan of one value per thread across a 256-thread block (Hillis-Steele through LDS).
template <typename T>
__device__ __forceinline__ T blockExclusiveScan(T val, T* total, T* lds /* [2 * SCAN_THREADS] */)
{
	int tid = threadIdx.x;
	int pin = 0;
	lds[tid] = val;
	__syncthreads();
	for (int off = 1; off < SCAN_THREADS; off <<= 1)
	{
		T v = lds[pin * SCAN_THREADS + tid];
		if (tid >= off) v = scanAdd(v, lds[pin * SCAN_THREADS + tid - off]);
		lds[(1 - pin) * SCAN_THREADS + tid] = v;
		pin = 1 - pin;
		__syncthreads();
	}
	T incl = lds[pin * SCAN_THREADS + tid];
	*total = lds[pin * SCAN_THREADS + SCAN_THREADS - 1];
	T excl;
	scanZero(excl);
	if (tid > 0) excl = lds[pin * SCAN_THREADS + tid - 1];
	__syncthreads();
	(void)incl;
	return excl;
}

template <typename T>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_reduce(const T* __restrict__ in, T* __restrict__ blockSums, const int* nPtr)
{
	__shared__ T lds[2 * SCAN_THREADS];
	int n = *nPtr;
	int base = blockIdx.x * SCAN_TILE;
	if (base >= n) return;
	T sum;
	scanZero(sum);
	for (int k = 0; k < SCAN_ITEMS; ++k)
	{
		int i = base + threadIdx.x * SCAN_ITEMS + k;
		if (i < n) sum = scanAdd(sum, in[i]);
	}
	T total;
	blockExclusiveScan(sum, &total, lds);
	if (threadIdx.x == 0) blockSums[blockIdx.x] = total;
}

template <typename T>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_blocksums(T* __restrict__ blockSums, const int* nPtr, T* totalOut)
{
	__shared__ T lds[2 * SCAN_THREADS];
	int n = *nPtr;
	int numBlocks = (n + SCAN_TILE - 1) / SCAN_TILE;
	T carry;
	scanZero(carry);
	for (int base = 0; base < numBlocks; base += SCAN_THREADS)
	{
		int i = base + threadIdx.x;
		T v;
		scanZero(v);
		if (i < numBlocks) v = blockSums[i];
		T total;
		T excl = blockExclusiveScan(v, &total, lds);
		if (i < numBlocks) blockSums[i] = scanAdd(carry, excl);
		carry = scanAdd(carry, total);
	}
	if (threadIdx.x == 0 && totalOut) *totalOut = carry;
}

// out[i] = sum of in[0..i) ; out[n] = total (out must hold n + 1 entries)
template <typename T>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_final(const T* __restrict__ in, T* __restrict__ out, const T* __restrict__ blockSums, const int* nPtr)
{
	__shared__ T lds[2 * SCAN_THREADS];
	int n = *nPtr;
	int base = blockIdx.x * SCAN_TILE;
	if (n == 0)
	{
		if (blockIdx.x == 0 && threadIdx.x == 0)
		{
			T z;
			scanZero(z);
			out[0] = z;
		}
		return;
	}
	if (base >= n) return;
	T v[SCAN_ITEMS];
	T sum;
	scanZero(sum);
	for (int k = 0; k < SCAN_ITEMS; ++k)
	{
		int i = base + threadIdx.x * SCAN_ITEMS + k;
		scanZero(v[k]);
		if (i < n) v[k] = in[i];
		sum = scanAdd(sum, v[k]);
	}
	T total;
	T excl = blockExclusiveScan(sum, &total, lds);
	T run = scanAdd(blockSums[blockIdx.x], excl);
	for (int k = 0; k < SCAN_ITEMS; ++k)
	{
		int i = base + threadIdx.x * SCAN_ITEMS + k;
		if (i < n) out[i] = run;
		run = scanAdd(run, v[k]);
		if (i == n - 1) out[n] = run;
	}
}

// ---- single-pass scan (decoupled look-back) ---------------------------------------------------------------------------------
// One launch instead of three: every tile publishes its aggregate, then walks back over its predecessors' status words
// until it meets one whose inclusive prefix is known, and publishes its own. Status per tile in `work`:
//   work[t]     aggregate of tile t          work[cap + t]   inclusive prefix up to and including tile t
//   flags[t]    (epoch << 2) | state, state 1 = aggregate published, 2 = prefix published
// `epoch` is unique per launch (the host counts them), so the flag words are never reset (they live in an array of their
// own that only ever holds flag words: zeroed when allocated). Progress: workgroups are dispatched in
// index order on every XCD, so the lowest unfinished tile is always running.
__device__ __forceinline__ int scanWaveSum(int v)
{
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
	return v;
}
__device__ __forceinline__ int4 scanWaveSum(int4 v)
{
	return make_int4(scanWaveSum(v.x), scanWaveSum(v.y), scanWaveSum(v.z), scanWaveSum(v.w));
}

// The look-back spins on status words other workgroups publish: bounded. A tile that has waited SCAN_SPIN_MAX polls (seconds:
// a poll is a memory round trip, ~1 us) for one word gives up, raises SCAN_ABORT_BIT in *abortWord and publishes a zero
// prefix so that its successors end too; every other waiting lane leaves as soon as it sees the bit. The host finds the bit
// with the step's read-back and fails the step (B2HIP_ERR_HIP) instead of hanging in it.
#define SCAN_SPIN_MAX (1u << 23)
#define SCAN_ABORT_BIT 256

// ITEMS per thread: 4 (tiles of 1 024 elements) up to 256 K elements; 16 (tiles of 4 096) up to 1 M - the look-back is a chain
// over the TILES, so a million-element scan (the body and grid tables of BASELINE config 5, the tables of a rank of a sharded
// world) is as short a chain as a 256 K one and still one launch instead of three.
template <typename T, int ITEMS>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_chain(const T* __restrict__ in, T* __restrict__ out, T* work, int* flags, int cap, const int* nPtr, unsigned epoch,
	int* abortWord)
{
	constexpr int TILE = SCAN_THREADS * ITEMS;
	__shared__ T lds[2 * SCAN_THREADS];
	__shared__ T s_prefix;
	const int n = *nPtr;
	const int tile = blockIdx.x;
	const int base = tile * TILE;
	if (n == 0)
	{
		if (tile == 0 && threadIdx.x == 0)
		{
			T z;
			scanZero(z);
			out[0] = z;
		}
		return;
	}
	if (base >= n) return;
	T v[ITEMS];
	T sum;
	scanZero(sum);
	for (int k = 0; k < ITEMS; ++k)
	{
		const int i = base + threadIdx.x * ITEMS + k;
		scanZero(v[k]);
		if (i < n) v[k] = in[i];
		sum = scanAdd(sum, v[k]);
	}
	T total;
	const T excl = blockExclusiveScan(sum, &total, lds);
	if (threadIdx.x < 64)
	{
		// the first wave looks back over 64 predecessors at a time (one status word per lane)
		const int lane = threadIdx.x;
		T* agg = work;
		T* pre = work + cap;
		T running;
		scanZero(running);
		if (tile > 0)
		{
			if (lane == 0)
			{
				scanStoreAgent(&agg[tile], total);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__hip_atomic_store(flags + tile, (int)((epoch << 2) | 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
			int hi = tile - 1; // nearest predecessor not yet accounted for
			while (true)
			{
				const int t = hi - lane;
				unsigned state = 2u; // (lanes before tile 0 count as "prefix known, zero")
				T val;
				scanZero(val);
				if (t >= 0)
				{
					unsigned word;
					unsigned polls = 0;
					bool gaveUp = false;
					do
					{
						word = (unsigned)__hip_atomic_load(flags + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						if ((++polls & 0xfffu) == 0u)
						{
							if (polls >= SCAN_SPIN_MAX) atomicOr(abortWord, SCAN_ABORT_BIT);
							gaveUp = (__hip_atomic_load(abortWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & SCAN_ABORT_BIT) != 0;
						}
					} while (!gaveUp && ((word >> 2) != epoch || (word & 3u) == 0u));
					state = gaveUp ? 2u : (word & 3u); // (aborted: pretend a zero prefix so that the walk ends)
					if (!gaveUp) val = scanLoadAgent(state == 2u ? &pre[t] : &agg[t]);
				}
				// the nearest tile whose inclusive prefix is known ends the walk
				const unsigned long long known = __ballot(state == 2u);
				const int stop = known ? __ffsll((long long)known) - 1 : 64;
				if (lane > stop) scanZero(val);
				running = scanAdd(running, scanWaveSum(val));
				if (stop < 64) break;
				hi -= 64;
			}
		}
		if (lane == 0)
		{
			scanStoreAgent(&pre[tile], scanAdd(running, total));
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__hip_atomic_store(flags + tile, (int)((epoch << 2) | 2u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			s_prefix = running;
		}
	}
	__syncthreads();
	T run = scanAdd(s_prefix, excl);
	for (int k = 0; k < ITEMS; ++k)
	{
		const int i = base + threadIdx.x * ITEMS + k;
		if (i < n) out[i] = run;
		run = scanAdd(run, v[k]);
		if (i == n - 1) out[n] = run;
	}
}

// Host helper: ONE launch on `stream`. capN bounds the grid; nPtr is the live count in device memory; `work` holds
// 2 * (capN / SCAN_TILE + 4) elements, `flags` capN / SCAN_TILE + 4 ints (zeroed when allocated).
// The epoch belongs to the flag array (ScanFlags: one per world): it tags the array's status words, 30 bits wide, and when it
// wraps the array is zeroed on the stream before the next scan, so that no word left behind by a scan 2^30 launches ago can
// read as "published" (a process-wide counter over per-world arrays could alias in a rarely used tile).
struct ScanFlags
{
	int* words = nullptr;   // device
	size_t count = 0;
	unsigned epoch = 0;     // of the last launch over `words`
	int* abortWord = nullptr; // device: SCAN_ABORT_BIT is raised here when a look-back gives up
};
template <typename T>
static inline void deviceExclusiveScan(hipStream_t stream, const T* in, T* out, T* work, ScanFlags& sf, const int* nPtr, int capN)
{
	int* flags = sf.words;
	int blocks = (capN + SCAN_TILE - 1) / SCAN_TILE;
	if (blocks < 1) blocks = 1;
	const int blocksWide = (capN + SCAN_TILE_WIDE - 1) / SCAN_TILE_WIDE;
	hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
	(void)hipStreamIsCapturing(stream, &capturing);
	if (capturing != hipStreamCaptureStatusNone || blocksWide > SCAN_CHAIN_MAX_TILES)
	{
		// a captured launch would replay its epoch, and past a few hundred tiles the look-back chain costs more than the two
		// launches it saves (1.4 M elements: 25 us against 15): the three-kernel form (reduce, scan of the tile sums, final)
		hipLaunchKernelGGL(k_scan_reduce<T>, dim3(blocks), dim3(SCAN_THREADS), 0, stream, in, work, nPtr);
		hipLaunchKernelGGL(k_scan_blocksums<T>, dim3(1), dim3(SCAN_THREADS), 0, stream, work, nPtr, (T*)nullptr);
		hipLaunchKernelGGL(k_scan_final<T>, dim3(blocks), dim3(SCAN_THREADS), 0, stream, in, out, work, nPtr);
		return;
	}
	if (sf.epoch >= 0x3fffffffu)
	{
		(void)hipMemsetAsync(flags, 0, sf.count * sizeof(int), stream);
		sf.epoch = 0u;
	}
	const unsigned epoch = ++sf.epoch;
	if (blocks <= SCAN_CHAIN_MAX_TILES)
		hipLaunchKernelGGL((k_scan_chain<T, SCAN_ITEMS>), dim3(blocks), dim3(SCAN_THREADS), 0, stream, in, out, work, flags, blocks + 4, nPtr, epoch, sf.abortWord);
	else
		hipLaunchKernelGGL((k_scan_chain<T, SCAN_ITEMS_WIDE>), dim3(blocksWide), dim3(SCAN_THREADS), 0, stream, in, out, work, flags, blocksWide + 4, nPtr, epoch, sf.abortWord);
}

// ---------------------------------------------------------------------------------------------
// Stable LSD radix sort of (uint64 key, int2 payload), up to RADIX_BITS = 11 bits per pass (round 5; 8 before: the pair
// update's keys are two proxy keys of 17 - 21 bits - six passes of three launches each, every one a dependent launch of a
// step that is priced by those; now four).
// Per pass: (1) per-tile digit histogram, (2) scan of the digit-major histogram matrix,
// (3) stable scatter using wave64 ballots to rank equal digits inside a wave.
#define RADIX_THREADS 256
#define RADIX_ITEMS 8
#define RADIX_TILE (RADIX_THREADS * RADIX_ITEMS)
#define RADIX_BITS 11
#define RADIX_DIGITS (1 << RADIX_BITS)

// `width` <= RADIX_BITS: the bits this pass looks at (the digit is (key >> shift) & ((1 << width) - 1); all RADIX_DIGITS rows of
// the matrix are written, the unused ones with zeros)
__global__ __launch_bounds__(RADIX_THREADS) void k_radix_hist(const uint64_t* __restrict__ keys, int* __restrict__ hist,
	const int* nPtr, int minN, int shift, int width, int numTilesCap)
{
	__shared__ int lh[RADIX_DIGITS];
	int n = *nPtr;
	if (n <= minN) return;
	int numTiles = (n + RADIX_TILE - 1) / RADIX_TILE;
	if (numTiles > (int)gridDim.x) numTiles = (int)gridDim.x; // (a sort sized for fewer keys than there are: k_radix_count has flagged it)
	int tile = blockIdx.x;
	if (tile >= numTiles) return;
	for (int q = threadIdx.x; q < RADIX_DIGITS; q += RADIX_THREADS) lh[q] = 0;
	__syncthreads();
	const uint32_t mask = (1u << width) - 1u;
	int base = tile * RADIX_TILE;
	for (int k = 0; k < RADIX_ITEMS; ++k)
	{
		int i = base + k * RADIX_THREADS + threadIdx.x;
		if (i < n)
		{
			int d = (int)((uint32_t)(keys[i] >> shift) & mask);
			atomicAdd(&lh[d], 1);
		}
	}
	__syncthreads();
	// digit-major so that a plain scan yields global offsets
	for (int q = threadIdx.x; q < RADIX_DIGITS; q += RADIX_THREADS) hist[q * numTiles + tile] = lh[q];
	(void)numTilesCap;
}

// histCount = RADIX_DIGITS * numTiles, written to device memory for the scan utility
// tilesCap: the tiles the launches of this sort were sized for. A sort that was queued without the host having seen the count
// (the pair update of a world that has been sorting with the radix passes lately) may meet more: the passes then cover a part
// only and `overflow` gets `overflowBit` - whoever consumes the result looks at it (createBlocked).
__global__ void k_radix_count(const int* nPtr, int minN, int* histCount, int tilesCap, int* overflow, int overflowBit)
{
	int n = *nPtr;
	int numTiles = (n + RADIX_TILE - 1) / RADIX_TILE;
	if (numTiles > tilesCap)
	{
		if (overflow != nullptr) atomicOr(overflow, overflowBit);
		numTiles = tilesCap;
	}
	*histCount = (n <= minN) ? 0 : RADIX_DIGITS * numTiles;
}

__global__ __launch_bounds__(RADIX_THREADS) void k_radix_scatter(const uint64_t* __restrict__ keysIn, const int2* __restrict__ valsIn,
	uint64_t* __restrict__ keysOut, int2* __restrict__ valsOut, const int* __restrict__ histScan, const int* nPtr, int minN, int shift, int width)
{
	// per wave: how many of the current round's keys of the three waves before it carry a digit - only the digits that OCCUR in
	// the round are touched (a round is 256 keys: at most 256 of the 2 048 counters), set by the first lane of a digit group
	// and taken back by it after the round
	__shared__ int waveCount[4][RADIX_DIGITS];
	__shared__ int digitBase[RADIX_DIGITS]; // running global offset per digit for this tile
	int n = *nPtr;
	if (n <= minN) return;
	int numTiles = (n + RADIX_TILE - 1) / RADIX_TILE;
	if (numTiles > (int)gridDim.x) { numTiles = (int)gridDim.x; n = numTiles * RADIX_TILE; } // (see k_radix_hist)
	int tile = blockIdx.x;
	if (tile >= numTiles) return;
	int tid = threadIdx.x;
	int lane = tid & 63;
	int wave = tid >> 6;
	for (int q = tid; q < RADIX_DIGITS; q += RADIX_THREADS)
	{
		digitBase[q] = histScan[q * numTiles + tile];
		waveCount[0][q] = 0; waveCount[1][q] = 0; waveCount[2][q] = 0; waveCount[3][q] = 0;
	}
	__syncthreads();
	const uint32_t mask = (1u << width) - 1u;
	int base = tile * RADIX_TILE;
	// (all of the tile's keys and payloads first: eight independent loads in flight, not one load's latency in front of every
	// round - the kernel moves 2 MB and was 16 us of dependent steps)
	uint64_t keyR[RADIX_ITEMS];
	int2 valR[RADIX_ITEMS];
#pragma unroll
	for (int k = 0; k < RADIX_ITEMS; ++k)
	{
		const int i = base + k * RADIX_THREADS + tid;
		keyR[k] = i < n ? keysIn[i] : 0;
		valR[k] = i < n ? valsIn[i] : make_int2(0, 0);
	}
#pragma unroll
	for (int k = 0; k < RADIX_ITEMS; ++k)
	{
		int i = base + k * RADIX_THREADS + tid;
		bool valid = i < n;
		uint64_t key = keyR[k];
		int d = valid ? (int)((uint32_t)(key >> shift) & mask) : -1;
		// lanes of this wave holding the same digit
		unsigned long long peers = __ballot(valid);
		for (int b = 0; b < RADIX_BITS; ++b)
		{
			unsigned long long m = __ballot(valid && ((d >> b) & 1));
			peers &= ((d >> b) & 1) ? m : ~m;
		}
		if (!valid) peers = 0;
		unsigned long long lower = peers & ((1ull << lane) - 1ull);
		int rankInWave = __popcll(lower);
		const bool first = valid && lower == 0; // first lane of each digit group
		const int groupSize = __popcll(peers);
		if (first) waveCount[wave][d] = groupSize;
		__syncthreads();
		int total = 0;
		if (valid)
		{
			int off = digitBase[d];
			for (int w = 0; w < wave; ++w) off += waveCount[w][d];
			int dst = off + rankInWave;
			keysOut[dst] = key;
			valsOut[dst] = valR[k];
			if (first) total = waveCount[0][d] + waveCount[1][d] + waveCount[2][d] + waveCount[3][d];
		}
		__syncthreads();
		// the digit's running offset moves on by the round's keys with that digit: added once per digit - by the first lane of
		// the digit's group in the LOWEST wave that has the digit - and the round's counters go back to zero
		if (first)
		{
			bool lowest = true;
			for (int w = 0; w < wave; ++w) lowest = lowest && waveCount[w][d] == 0;
			if (lowest) digitBase[d] += total;
		}
		__syncthreads();
		if (first) waveCount[wave][d] = 0;
		__syncthreads();
	}
}

// ---- one launch per pass ----------------------------------------------------------------------------------------------------
// The three launches of a pass (histogram, scan of the tiles x digits matrix, scatter) as ONE: at 260 tiles each of them sits
// at its latency floor, so a pass costs its launch boundaries, not its data. One launch in front of the sort
// (k_radix_prepare) reads the keys once and leaves the GLOBAL digit histogram of every pass; a pass kernel then
//   1. turns its pass's histogram into the global base of every digit (a block scan of <= 2 048 counters),
//   2. ranks the tile's keys with the ballots k_radix_scatter uses, each wave a quarter of the tile on counters of its own (one
//      barrier per tile, not four per round) - the ranks stay in registers, the tile's per-digit counts fall out of the ranking,
//   3. publishes the counts, one tagged word per digit,
//   4. looks back: per digit, the keys of that digit in the tiles before it,
//   5. scatters: global base + keys in earlier tiles + rank inside the tile. Same places as the three-launch form, bit for bit.
// The look-back has two levels so that no tile reads more than 15 + tiles / 16 words per digit and nothing forms a chain:
//   counts[t][q]   (tag << 16) | keys of digit q in tile t (<= 2 048), published by every tile BEFORE it waits for anything
//   groups[g][q]   (tag << 16) | keys of digit q in tiles [16 g, 16 g + 16) (<= 32 768), published by the group's last tile as
//                  soon as it has read the 15 counts before its own
// Tile t reads counts[16 g .. t) of its own group g = t / 16, then groups[0 .. g). (The running inclusive prefix of the
// classic decoupled look-back never helps here: up to a thousand tiles of 50 KB LDS are resident at once and start together,
// so no predecessor is ever a whole look-back ahead - a tile would walk all the way down, 260 words per digit, or wait on a
// chain of 260 tiles. A count depends on nothing, a group sum on counts only: two memory round trips.)
// `tag` is unique per pass (RadixStatus::epoch, 16 bits; the host zeroes both arrays on the stream before it wraps), so the
// words are never reset and value and tag arrive in one store. Progress: a tile waits for words of LOWER tiles only, and
// workgroups are dispatched in index order (the tile index IS blockIdx.x) - the argument of k_scan_chain. Every wait is bounded
// the same way: SCAN_SPIN_MAX polls, SCAN_ABORT_BIT in *abortWord, a waiter that gives up takes zero for the word and goes on
// (it still publishes its group's sum, so nobody waits for it; partial sums only ever point below the true place, and the
// scatter checks the bound anyway). The host finds the bit in the step's read-back and fails the step.
#define RADIX_MAX_PASSES 6             // one-launch form: the passes one k_radix_prepare counts for (48 KB of LDS)
#define RADIX_GROUP 16
#define RADIX_ONEPASS_MAX_TILES 1024   // 2 M keys: 64 group words per digit at most
#define RADIX_PREPARE_TILES 2          // tiles per workgroup of k_radix_prepare (fewer flushes into the global histograms)

struct RadixLayout
{
	int passes;
	int shift[RADIX_MAX_PASSES];
	int width[RADIX_MAX_PASSES];
};

// The global digit histograms of all passes: hist[p * RADIX_DIGITS + digit], zero when the kernel starts (the prepare launch of
// the sort before this one zeroed it: `histNext` is the other of two buffers), and k_radix_count's job - the tile clamp and the
// overflow bit.
__global__ __launch_bounds__(RADIX_THREADS) void k_radix_prepare(const uint64_t* __restrict__ keys, const int* nPtr, int tilesCap, RadixLayout lay,
	int* __restrict__ hist, int* __restrict__ histNext, int* overflow, int overflowBit)
{
	__shared__ int lh[RADIX_MAX_PASSES][RADIX_DIGITS];
	for (int q = blockIdx.x * RADIX_THREADS + threadIdx.x; q < RADIX_MAX_PASSES * RADIX_DIGITS; q += gridDim.x * RADIX_THREADS) histNext[q] = 0;
	int n = *nPtr;
	if (n <= 0) return;
	int numTiles = (n + RADIX_TILE - 1) / RADIX_TILE;
	if (numTiles > tilesCap)
	{
		if (overflow != nullptr && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(overflow, overflowBit);
		numTiles = tilesCap;
		n = numTiles * RADIX_TILE;
	}
	const int base = blockIdx.x * (RADIX_PREPARE_TILES * RADIX_TILE);
	if (base >= n) return;
	for (int p = 0; p < lay.passes; ++p)
		for (int q = threadIdx.x; q < (1 << lay.width[p]); q += RADIX_THREADS) lh[p][q] = 0;
	__syncthreads();
	// (neighbouring keys often share a digit - the pair search emits a proxy's pairs in a row, so the high digits of a wave's 64 keys
	// are a handful of runs - and 64 adds to one LDS word are served one after the other: the first lane of a run adds its length)
	const int lane = threadIdx.x & 63;
	for (int k = 0; k < RADIX_PREPARE_TILES * RADIX_ITEMS; ++k)
	{
		const int i = base + k * RADIX_THREADS + threadIdx.x;
		const bool valid = i < n;
		const uint64_t key = valid ? keys[i] : 0;
		const int nValid = __popcll(__ballot(valid)); // (the valid lanes of a wave are its first ones)
		for (int p = 0; p < lay.passes; ++p)
		{
			const int d = valid ? (int)((uint32_t)(key >> lay.shift[p]) & ((1u << lay.width[p]) - 1u)) : -1;
			const int prev = __shfl_up(d, 1);
			const bool head = valid && (lane == 0 || prev != d);
			const unsigned long long heads = __ballot(head);
			if (head)
			{
				const unsigned long long rest = lane < 63 ? heads >> (lane + 1) : 0ull;
				const int end = rest ? lane + __ffsll((long long)rest) : nValid;
				atomicAdd(&lh[p][d], end - lane);
			}
		}
	}
	__syncthreads();
	for (int p = 0; p < lay.passes; ++p)
		for (int q = threadIdx.x; q < (1 << lay.width[p]); q += RADIX_THREADS)
		{
			const int v = lh[p][q];
			if (v) atomicAdd(&hist[p * RADIX_DIGITS + q], v);
		}
}

// One status word of another tile: `word` is what a first load saw; polls until the word carries `tag` (bounded, see above).
__device__ __forceinline__ int radixAwait(const unsigned* p, unsigned word, unsigned tag, int* abortWord, bool& gaveUp)
{
	unsigned polls = 0;
	while (!gaveUp && (word >> 16) != tag)
	{
		word = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if ((++polls & 0xfffu) == 0u)
		{
			if (polls >= SCAN_SPIN_MAX) atomicOr(abortWord, SCAN_ABORT_BIT);
			gaveUp = (__hip_atomic_load(abortWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & SCAN_ABORT_BIT) != 0;
		}
	}
	return (word >> 16) == tag ? (int)(word & 0xffffu) : 0;
}

__global__ __launch_bounds__(RADIX_THREADS) void k_radix_onepass(const uint64_t* __restrict__ keysIn, const int2* __restrict__ valsIn,
	uint64_t* __restrict__ keysOut, int2* __restrict__ valsOut, const int* __restrict__ passHist, unsigned* counts, unsigned* groups,
	const int* nPtr, int shift, int width, unsigned tag, int* abortWord)
{
	__shared__ int waveCount[4][RADIX_DIGITS]; // per wave: keys of the digit in its quarter so far; after the ranking: in the quarters before it
	__shared__ int digitBase[RADIX_DIGITS];    // keys of the digit in the tile
	__shared__ int digitOff[RADIX_DIGITS];     // where the tile's first key of the digit goes
	__shared__ int scanLds[2 * SCAN_THREADS];
	int n = *nPtr;
	if (n <= 0) return;
	int numTiles = (n + RADIX_TILE - 1) / RADIX_TILE;
	if (numTiles > (int)gridDim.x) { numTiles = (int)gridDim.x; n = numTiles * RADIX_TILE; } // (k_radix_prepare has flagged it)
	const int tile = blockIdx.x;
	if (tile >= numTiles) return;
	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int wave = tid >> 6;
	const int D = 1 << width;
	const uint32_t mask = (uint32_t)D - 1u;
	const int base = tile * RADIX_TILE;
	uint64_t keyR[RADIX_ITEMS];
	int2 valR[RADIX_ITEMS];
	int rank[RADIX_ITEMS];
	// (a wave takes a quarter of the tile, 64 keys in a row per round: the ranking below then needs no barrier between rounds)
	const int first0 = base + wave * (RADIX_TILE / 4) + lane;
#pragma unroll
	for (int k = 0; k < RADIX_ITEMS; ++k)
	{
		const int i = first0 + k * 64;
		keyR[k] = i < n ? keysIn[i] : 0;
		valR[k] = i < n ? valsIn[i] : make_int2(0, 0);
	}
	for (int q = tid; q < D; q += RADIX_THREADS)
	{
		waveCount[0][q] = 0; waveCount[1][q] = 0; waveCount[2][q] = 0; waveCount[3][q] = 0;
	}
	{
		// 1. global base of every digit: exclusive scan of the pass's histogram (eight consecutive digits per thread)
		constexpr int PER = RADIX_DIGITS / RADIX_THREADS;
		int h[PER];
		int sum = 0;
#pragma unroll
		for (int k = 0; k < PER; ++k)
		{
			const int q = tid * PER + k;
			h[k] = q < D ? passHist[q] : 0;
			sum += h[k];
		}
		int total;
		int run = blockExclusiveScan(sum, &total, scanLds);
#pragma unroll
		for (int k = 0; k < PER; ++k)
		{
			const int q = tid * PER + k;
			if (q < D) digitOff[q] = run;
			run += h[k];
		}
	}
	__syncthreads();
	// 2. the ballot ranking of k_radix_scatter, wave by wave: rank[k] = keys of the same digit before this one in the wave's
	// quarter. The wave's own row of counters runs along from round to round (written by the first lane of a digit's group and
	// handed to the group by a shuffle: LDS serves a wave's accesses in program order), so nothing waits for another wave.
	int* const myCount = waveCount[wave];
#pragma unroll
	for (int k = 0; k < RADIX_ITEMS; ++k)
	{
		const bool valid = first0 + k * 64 < n;
		const int d = valid ? (int)((uint32_t)(keyR[k] >> shift) & mask) : -1;
		unsigned long long peers = __ballot(valid);
		for (int b = 0; b < width; ++b)
		{
			const unsigned long long m = __ballot(valid && ((d >> b) & 1));
			peers &= ((d >> b) & 1) ? m : ~m;
		}
		if (!valid) peers = 0;
		const unsigned long long lower = peers & ((1ull << lane) - 1ull);
		const bool first = valid && lower == 0;
		int before = 0;
		if (first)
		{
			before = myCount[d];
			myCount[d] = before + __popcll(peers);
		}
		before = __shfl(before, valid ? __ffsll((long long)peers) - 1 : lane);
		rank[k] = before + __popcll(lower);
	}
	__syncthreads();
	// per digit: the waves' counts become the keys of the digit in the waves before, their sum the tile's count
	for (int q = tid; q < D; q += RADIX_THREADS)
	{
		const int c0 = waveCount[0][q], c1 = waveCount[1][q], c2 = waveCount[2][q], c3 = waveCount[3][q];
		waveCount[0][q] = 0; waveCount[1][q] = c0; waveCount[2][q] = c0 + c1; waveCount[3][q] = c0 + c1 + c2;
		digitBase[q] = c0 + c1 + c2 + c3;
	}
	// 3. the tile's counts (thread tid owns the digits tid, tid + 256, ...: neighbouring lanes, neighbouring words)
	for (int q = tid; q < D; q += RADIX_THREADS)
		__hip_atomic_store(counts + (size_t)tile * D + q, (tag << 16) | (unsigned)digitBase[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	// 4. look back (a thread owns the digits tid, tid + 256, ...; two of them at a time so that their loads are in flight together)
	bool gaveUp = false;
	const int group = tile / RADIX_GROUP;
	const int inGroup = tile - group * RADIX_GROUP; // tiles of the own group before this one
	for (int q0 = tid; q0 < D; q0 += 2 * RADIX_THREADS)
	{
		const bool two = q0 + RADIX_THREADS < D;
		const unsigned* srcA = counts + (size_t)(group * RADIX_GROUP) * D + q0;
		const unsigned* srcB = srcA + RADIX_THREADS;
		unsigned wordA[RADIX_GROUP - 1], wordB[RADIX_GROUP - 1];
#pragma unroll
		for (int j = 0; j < RADIX_GROUP - 1; ++j)
		{
			wordA[j] = j < inGroup ? __hip_atomic_load(srcA + (size_t)j * D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
			wordB[j] = (two && j < inGroup) ? __hip_atomic_load(srcB + (size_t)j * D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
		}
		int beforeA = 0, beforeB = 0;
#pragma unroll
		for (int j = 0; j < RADIX_GROUP - 1; ++j)
			if (j < inGroup)
			{
				beforeA += radixAwait(srcA + (size_t)j * D, wordA[j], tag, abortWord, gaveUp);
				if (two) beforeB += radixAwait(srcB + (size_t)j * D, wordB[j], tag, abortWord, gaveUp);
			}
		if (inGroup == RADIX_GROUP - 1)
		{
			unsigned* dstA = groups + (size_t)group * D + q0;
			__hip_atomic_store(dstA, (tag << 16) | (unsigned)(beforeA + digitBase[q0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (two) __hip_atomic_store(dstA + RADIX_THREADS, (tag << 16) | (unsigned)(beforeB + digitBase[q0 + RADIX_THREADS]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		digitOff[q0] += beforeA;
		if (two) digitOff[q0 + RADIX_THREADS] += beforeB;
	}
	for (int q0 = tid; q0 < D; q0 += 2 * RADIX_THREADS)
	{
		const bool two = q0 + RADIX_THREADS < D;
		int beforeA = 0, beforeB = 0;
		for (int g0 = 0; g0 < group; g0 += 16)
		{
			const unsigned* srcA = groups + (size_t)g0 * D + q0;
			const unsigned* srcB = srcA + RADIX_THREADS;
			const int m = group - g0; // (the first 16 of them in this round)
			unsigned wordA[16], wordB[16];
#pragma unroll
			for (int j = 0; j < 16; ++j)
			{
				wordA[j] = j < m ? __hip_atomic_load(srcA + (size_t)j * D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
				wordB[j] = (two && j < m) ? __hip_atomic_load(srcB + (size_t)j * D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
			}
#pragma unroll
			for (int j = 0; j < 16; ++j)
				if (j < m)
				{
					beforeA += radixAwait(srcA + (size_t)j * D, wordA[j], tag, abortWord, gaveUp);
					if (two) beforeB += radixAwait(srcB + (size_t)j * D, wordB[j], tag, abortWord, gaveUp);
				}
		}
		digitOff[q0] += beforeA;
		if (two) digitOff[q0 + RADIX_THREADS] += beforeB;
	}
	__syncthreads();
	// 5. scatter
#pragma unroll
	for (int k = 0; k < RADIX_ITEMS; ++k)
	{
		if (first0 + k * 64 < n)
		{
			const int d = (int)((uint32_t)(keyR[k] >> shift) & mask);
			const int dst = digitOff[d] + myCount[d] + rank[k];
			if ((unsigned)dst < (unsigned)n) // (always, unless a look-back gave up)
			{
				keysOut[dst] = keyR[k];
				valsOut[dst] = valR[k];
			}
		}
	}
}

// The status words of the one-launch passes, one set per world. `counts` holds maxTiles * RADIX_DIGITS words, `groups`
// (maxTiles / RADIX_GROUP + 1) * RADIX_DIGITS, `hist` two buffers of RADIX_MAX_PASSES * RADIX_DIGITS ints; all zeroed when allocated.
struct RadixStatus
{
	unsigned* counts = nullptr;
	unsigned* groups = nullptr;
	size_t countsCap = 0, groupsCap = 0; // words
	int* hist = nullptr;
	int maxTiles = 0;        // the tiles `counts` / `groups` are sized for (<= RADIX_ONEPASS_MAX_TILES); 0: three-launch passes only
	unsigned epoch = 0;      // tag of the last pass (16 bits, never 0)
	unsigned parity = 0;     // which half of `hist` the next sort counts into
	int* abortWord = nullptr;
};

// Whether a sort can take the one-launch form.
static inline bool radixOnepassFits(hipStream_t stream, const RadixStatus& rs, int tilesCap, size_t passes)
{
	if (rs.maxTiles <= 0 || tilesCap > rs.maxTiles || passes == 0 || passes > RADIX_MAX_PASSES) return false;
	// (a captured launch would replay its tags and its histogram parity: the three-launch form, as deviceExclusiveScan)
	hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
	(void)hipStreamIsCapturing(stream, &capturing);
	return capturing == hipStreamCaptureStatusNone;
}

#endif
