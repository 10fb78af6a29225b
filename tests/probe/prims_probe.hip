// GPU probe of the integer primitives everything else stands on: the device-wide exclusive scan of box2d-mt_amd/csrc/b2d_scan.h
// (deviceExclusiveScan<int> and <int4>, called exactly as the product calls it, on a ScanFlags that lives across calls as a
// world's does) and the wave / workgroup aggregation helpers of box2d-mt_amd/csrc/b2d_wave.h, one kernel per helper, fed
// per-thread keys, values and valid flags from the host. Built with the product's own flags (box2d-mt_amd/Makefile:
// $(HIPFLAGS)); checked against numpy references (tests/prims_ref.py) by tests/test_gpu_scan.py and tests/test_gpu_wave.py.
// TEST INFRASTRUCTURE: nothing in the product links this file and it links no product library; the headers are included unchanged.
//
// Every entry checks its arguments on the host and returns hipErrorInvalidValue for bad ones (n > capN, a block size that is
// no multiple of 64 in 64..1024, a key outside the counter array): a bad call never becomes an out-of-bounds access on the
// device. Entries return 0 or the failing hipError_t; pprobe_scan_run returns PPROBE_SCAN_ABORTED when it finds SCAN_ABORT_BIT.
#include "b2d_scan.h"
#include "b2d_wave.h"

#include <new>

#define PPROBE_SCAN_ABORTED (-1000)
#define PPROBE_FILL_BYTE 0x5A
#define PPROBE_MAX_CAP (1 << 24)
#define PPROBE_MAX_GUARD (1 << 16)
#define PPROBE_MAX_GRID 4096
#define PPROBE_MAX_ROUNDS 64

namespace
{

struct ScanHandle
{
	ScanFlags sf;
	hipStream_t stream = nullptr;
	int4* work = nullptr; // 2 * (maxCap / SCAN_TILE + 4) elements of int4 (b2d_scan.h: "Host helper"); the int scans use its front
	int* dN = nullptr;    // the live count, in device memory as the product keeps it
	int maxCap = 0;
};

void scanFree(ScanHandle* h)
{
	if (h->stream) (void)hipStreamDestroy(h->stream);
	if (h->sf.words) (void)hipFree(h->sf.words);
	if (h->sf.abortWord) (void)hipFree(h->sf.abortWord);
	if (h->work) (void)hipFree(h->work);
	if (h->dN) (void)hipFree(h->dN);
	delete h;
}

template <typename T>
int scanRun(ScanHandle* h, int capN, int n, const void* in, void* out, int guard)
{
	const size_t outCount = (size_t)capN + 1 + (size_t)guard;
	T* dIn = nullptr;
	T* dOut = nullptr;
	int abortWord = 0;
	hipError_t err = hipMalloc((void**)&dIn, (size_t)capN * sizeof(T));
	if (err == hipSuccess) err = hipMalloc((void**)&dOut, outCount * sizeof(T));
	// (the part of `in` beyond the live count is never read; it holds the fill byte so that a read of it would show)
	if (err == hipSuccess) err = hipMemsetAsync(dIn, PPROBE_FILL_BYTE, (size_t)capN * sizeof(T), h->stream);
	if (err == hipSuccess && n > 0) err = hipMemcpyAsync(dIn, in, (size_t)n * sizeof(T), hipMemcpyHostToDevice, h->stream);
	if (err == hipSuccess) err = hipMemcpyAsync(h->dN, &n, sizeof(int), hipMemcpyHostToDevice, h->stream);
	if (err == hipSuccess) err = hipMemsetAsync(dOut, PPROBE_FILL_BYTE, outCount * sizeof(T), h->stream);
	if (err == hipSuccess) err = hipStreamSynchronize(h->stream); // (`n` is a stack variable: uploaded before it goes)
	if (err == hipSuccess)
	{
		deviceExclusiveScan<T>(h->stream, dIn, dOut, (T*)h->work, h->sf, h->dN, capN);
		err = hipGetLastError();
	}
	if (err == hipSuccess) err = hipMemcpyAsync(out, dOut, outCount * sizeof(T), hipMemcpyDeviceToHost, h->stream);
	if (err == hipSuccess) err = hipMemcpyAsync(&abortWord, h->sf.abortWord, sizeof(int), hipMemcpyDeviceToHost, h->stream);
	if (err == hipSuccess) err = hipStreamSynchronize(h->stream);
	if (dIn) (void)hipFree(dIn);
	if (dOut) (void)hipFree(dOut);
	if (err != hipSuccess) return (int)err;
	return (abortWord & SCAN_ABORT_BIT) ? PPROBE_SCAN_ABORTED : 0;
}

// ---- the helpers of b2d_wave.h, one kernel each ---------------------------------------------------------------------------
// Thread i of the launch reads element r * n + i of key / val / valid in round r; threads with i >= n still call the helper,
// with valid = false (the wave-uniform contract of the header). A slot a helper returns is stored to `slots` and never used
// as an address.
struct WaveIn
{
	int n, rounds;
	const int* key;
	const uint32_t* val;
	const int* valid;
	int* slots;
	int p0, p1;
};

struct Offer
{
	int key;
	uint32_t val;
	bool valid;
	size_t at;
	bool live; // i < n: the thread owns an element of the arrays
};

__device__ __forceinline__ Offer offerOf(const WaveIn& a, int r)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	Offer o;
	o.live = i < (size_t)a.n;
	o.at = (size_t)r * (size_t)a.n + i;
	o.key = o.live ? a.key[o.at] : 0;
	o.val = o.live ? a.val[o.at] : 0u;
	o.valid = o.live && a.valid[o.at] != 0;
	return o;
}

#define PPROBE_WAVE_ATOMIC_KERNEL(KERNEL, HELPER, T)                                     \
	__global__ void KERNEL(WaveIn a, T* base)                                            \
	{                                                                                    \
		for (int r = 0; r < a.rounds; ++r)                                               \
		{                                                                                \
			const Offer o = offerOf(a, r);                                               \
			HELPER(base, o.key, (T)o.val, o.valid);                                      \
		}                                                                                \
	}
PPROBE_WAVE_ATOMIC_KERNEL(k_wave_add_int, waveAtomicAddInt, int)
PPROBE_WAVE_ATOMIC_KERNEL(k_wave_min_int, waveAtomicMinInt, int)
PPROBE_WAVE_ATOMIC_KERNEL(k_wave_max_u32, waveAtomicMaxU32, uint32_t)
PPROBE_WAVE_ATOMIC_KERNEL(k_wave_max_u32_guarded, waveAtomicMaxU32Guarded, uint32_t)
PPROBE_WAVE_ATOMIC_KERNEL(k_wave_min_u32, waveAtomicMinU32, uint32_t)
#undef PPROBE_WAVE_ATOMIC_KERNEL

__global__ void k_block_max_u32(WaveIn a, uint32_t* base)
{
	BlockMaxU32 run;
	run.key = -1;
	run.val = 0u;
	for (int r = 0; r < a.rounds; ++r)
	{
		const Offer o = offerOf(a, r);
		blockMaxU32Offer(run, base, o.key, o.val, o.valid);
	}
	blockMaxU32Flush(run, base);
}

__global__ void k_block_max_if_above(WaveIn a, int* base)
{
	for (int r = 0; r < a.rounds; ++r)
	{
		const Offer o = offerOf(a, r);
		blockAtomicMaxIfAbove(base, o.valid ? (int)o.val : 0); // (values <= 0 are no offer)
	}
}

__global__ void k_block_hot(WaveIn a, int* base)
{
	__shared__ BlockHot hot;
	blockHotInit(&hot);
	for (int r = 0; r < a.rounds; ++r)
	{
		const Offer o = offerOf(a, r);
		blockHotAddInt(&hot, base, o.key, (int)o.val, o.valid);
	}
	blockHotFlush(&hot, base);
}

__global__ void k_block_alloc(WaveIn a, int* base)
{
	for (int r = 0; r < a.rounds; ++r)
	{
		const Offer o = offerOf(a, r);
		const int slot = blockAlloc(base, o.valid);
		if (o.live) a.slots[o.at] = slot;
	}
}

__global__ void k_wave_keyed_alloc(WaveIn a, int* base)
{
	for (int r = 0; r < a.rounds; ++r)
	{
		const Offer o = offerOf(a, r);
		const int slot = waveKeyedAlloc(base, o.key, o.valid);
		if (o.live) a.slots[o.at] = slot;
	}
}

__global__ void k_wave_run_alloc(WaveIn a, int* base)
{
	for (int r = 0; r < a.rounds; ++r)
	{
		const Offer o = offerOf(a, r);
		const int slot = waveRunAlloc(base, o.key, o.valid);
		if (o.live) a.slots[o.at] = slot;
	}
}

__global__ void k_wave_keyed_alloc_once(WaveIn a, int* base)
{
	for (int r = 0; r < a.rounds; ++r)
	{
		const Offer o = offerOf(a, r);
		const int slot = waveKeyedAllocOnce(base, o.key, o.valid, a.p0, a.p1);
		if (o.live) a.slots[o.at] = slot;
	}
}

__global__ void k_block_keyed_alloc65(WaveIn a, int* base)
{
	for (int r = 0; r < a.rounds; ++r)
	{
		const Offer o = offerOf(a, r);
		const int slot = blockKeyedAlloc65(base, o.key, o.valid, a.p0 != 0, a.p1 != 0);
		if (o.live) a.slots[o.at] = slot;
	}
}

enum WaveOp
{
	OP_WAVE_ADD_INT = 0,
	OP_WAVE_MIN_INT = 1,
	OP_WAVE_MAX_U32 = 2,
	OP_WAVE_MAX_U32_GUARDED = 3,
	OP_WAVE_MIN_U32 = 4,
	OP_BLOCK_MAX_U32 = 5,
	OP_BLOCK_MAX_IF_ABOVE = 6,
	OP_BLOCK_HOT = 7,
	OP_BLOCK_ALLOC = 8,
	OP_WAVE_KEYED_ALLOC = 9,
	OP_WAVE_RUN_ALLOC = 10,
	OP_WAVE_KEYED_ALLOC_ONCE = 11,
	OP_BLOCK_KEYED_ALLOC65 = 12,
	OP_COUNT = 13
};

bool opAllocates(int op) { return op >= OP_BLOCK_ALLOC; }

// The words of `base` a key may address, or -1 for a key the helper must not be given. Every element's key is checked, valid or
// not: no helper reads base[key] of an invalid lane, and no test needs such a key out of range.
long wordOfKey(int op, int key, int p0, int p1)
{
	switch (op)
	{
	case OP_BLOCK_MAX_IF_ABOVE:
	case OP_BLOCK_ALLOC:
		return 0; // one word; the key is not looked at
	case OP_WAVE_KEYED_ALLOC_ONCE:
		if (key < 0 || (p0 < 31 && key >= (1 << p0))) return -1;
		return (long)key * p1;
	case OP_BLOCK_KEYED_ALLOC65:
		if (key < 0 || key > 64) return -1;
		return p1 ? colorSlot(key) : key;
	default:
		return key < 0 ? -1 : key;
	}
}

} // namespace

extern "C"
{

int pprobe_scan_aborted_code() { return PPROBE_SCAN_ABORTED; }

// A scan context for capacities up to maxCap: zeroed flag words, a zeroed abort word, a stream, `work` for int4.
int pprobe_scan_open(int maxCap, void** handleOut)
{
	if (!handleOut || maxCap < 1 || maxCap > PPROBE_MAX_CAP) return (int)hipErrorInvalidValue;
	*handleOut = nullptr;
	ScanHandle* h = new (std::nothrow) ScanHandle;
	if (!h) return (int)hipErrorOutOfMemory;
	h->maxCap = maxCap;
	h->sf.count = (size_t)maxCap / SCAN_TILE + 8;
	const size_t workCount = 2 * ((size_t)maxCap / SCAN_TILE + 4);
	hipError_t err = hipStreamCreate(&h->stream);
	if (err == hipSuccess) err = hipMalloc((void**)&h->sf.words, h->sf.count * sizeof(int));
	if (err == hipSuccess) err = hipMemset(h->sf.words, 0, h->sf.count * sizeof(int));
	if (err == hipSuccess) err = hipMalloc((void**)&h->sf.abortWord, sizeof(int));
	if (err == hipSuccess) err = hipMemset(h->sf.abortWord, 0, sizeof(int));
	if (err == hipSuccess) err = hipMalloc((void**)&h->work, workCount * sizeof(int4));
	if (err == hipSuccess) err = hipMemset(h->work, 0, workCount * sizeof(int4));
	if (err == hipSuccess) err = hipMalloc((void**)&h->dN, sizeof(int));
	if (err == hipSuccess) err = hipDeviceSynchronize();
	if (err != hipSuccess) { scanFree(h); return (int)err; }
	*handleOut = h;
	return 0;
}

// One deviceExclusiveScan over in[0 .. n) with capacity capN; elemInts 1 = int, 4 = int4. `out` receives all
// capN + 1 + guard elements of the device's output array, which held the byte 0x5A everywhere before the scan.
int pprobe_scan_run(void* handle, int elemInts, int capN, int n, const void* in, void* out, int guard)
{
	ScanHandle* h = (ScanHandle*)handle;
	if (!h || !out || (elemInts != 1 && elemInts != 4)) return (int)hipErrorInvalidValue;
	if (capN < 1 || capN > h->maxCap || n < 0 || n > capN || guard < 0 || guard > PPROBE_MAX_GUARD) return (int)hipErrorInvalidValue;
	if (n > 0 && !in) return (int)hipErrorInvalidValue;
	return elemInts == 1 ? scanRun<int>(h, capN, n, in, out, guard) : scanRun<int4>(h, capN, n, in, out, guard);
}

// ScanFlags::epoch of the host struct, nothing else
unsigned pprobe_scan_epoch(void* handle) { return handle ? ((ScanHandle*)handle)->sf.epoch : 0u; }

int pprobe_scan_set_epoch(void* handle, unsigned value)
{
	if (!handle) return (int)hipErrorInvalidValue;
	((ScanHandle*)handle)->sf.epoch = value;
	return 0;
}

int pprobe_scan_close(void* handle)
{
	if (!handle) return (int)hipErrorInvalidValue;
	ScanHandle* h = (ScanHandle*)handle;
	const hipError_t err = hipStreamSynchronize(h->stream);
	scanFree(h);
	return (int)err;
}

// One helper of b2d_wave.h (op: WaveOp above) in a launch of `grid` workgroups of `block` threads, `rounds` calls per thread.
// key / val / valid: rounds * n elements (val: the 32 bits of an int or a uint32_t). base: baseLen words, initial contents in,
// final contents out. slots: rounds * n, the value each call returned (allocators only; may be null otherwise).
// p0, p1: keyBits and stride of waveKeyedAllocOnce; fetch and slotted of blockKeyedAlloc65; 0 otherwise.
int pprobe_wave(int op, int block, int grid, int rounds, int n, const int* key, const uint32_t* val, const int* valid,
	uint32_t* base, int baseLen, int* slots, int p0, int p1)
{
	if (op < 0 || op >= OP_COUNT || block < 64 || block > 1024 || block % 64 != 0 || grid < 1 || grid > PPROBE_MAX_GRID)
		return (int)hipErrorInvalidValue;
	if (rounds < 1 || rounds > PPROBE_MAX_ROUNDS || n < 0 || (long)n > (long)block * grid || baseLen < 1 || !base) return (int)hipErrorInvalidValue;
	if (n > 0 && (!key || !val || !valid)) return (int)hipErrorInvalidValue;
	if (opAllocates(op) && !slots) return (int)hipErrorInvalidValue;
	if (op == OP_BLOCK_KEYED_ALLOC65 && block < 128) return (int)hipErrorInvalidValue; // (its first 65 threads clear the LDS counters)
	if (op == OP_WAVE_KEYED_ALLOC_ONCE && (p0 < 0 || p0 > 31 || p1 < 1)) return (int)hipErrorInvalidValue;
	if (op != OP_WAVE_KEYED_ALLOC_ONCE && op != OP_BLOCK_KEYED_ALLOC65 && (p0 != 0 || p1 != 0)) return (int)hipErrorInvalidValue;
	const size_t total = (size_t)rounds * (size_t)n;
	for (size_t q = 0; q < total; ++q)
	{
		const long word = wordOfKey(op, key[q], p0, p1);
		if (word < 0 || word >= (long)baseLen) return (int)hipErrorInvalidValue;
	}
	const size_t count = total ? total : 1;
	int* dKey = nullptr;
	uint32_t* dVal = nullptr;
	int* dValid = nullptr;
	int* dSlots = nullptr;
	uint32_t* dBase = nullptr;
	hipError_t err = hipMalloc((void**)&dKey, count * sizeof(int));
	if (err == hipSuccess) err = hipMalloc((void**)&dVal, count * sizeof(uint32_t));
	if (err == hipSuccess) err = hipMalloc((void**)&dValid, count * sizeof(int));
	if (err == hipSuccess) err = hipMalloc((void**)&dSlots, count * sizeof(int));
	if (err == hipSuccess) err = hipMalloc((void**)&dBase, (size_t)baseLen * sizeof(uint32_t));
	if (err == hipSuccess && total) err = hipMemcpy(dKey, key, total * sizeof(int), hipMemcpyHostToDevice);
	if (err == hipSuccess && total) err = hipMemcpy(dVal, val, total * sizeof(uint32_t), hipMemcpyHostToDevice);
	if (err == hipSuccess && total) err = hipMemcpy(dValid, valid, total * sizeof(int), hipMemcpyHostToDevice);
	if (err == hipSuccess) err = hipMemset(dSlots, PPROBE_FILL_BYTE, count * sizeof(int));
	if (err == hipSuccess) err = hipMemcpy(dBase, base, (size_t)baseLen * sizeof(uint32_t), hipMemcpyHostToDevice);
	if (err == hipSuccess)
	{
		WaveIn a;
		a.n = n; a.rounds = rounds; a.key = dKey; a.val = dVal; a.valid = dValid; a.slots = dSlots; a.p0 = p0; a.p1 = p1;
		const dim3 g((unsigned)grid), b((unsigned)block);
		switch (op)
		{
		case OP_WAVE_ADD_INT: k_wave_add_int<<<g, b>>>(a, (int*)dBase); break;
		case OP_WAVE_MIN_INT: k_wave_min_int<<<g, b>>>(a, (int*)dBase); break;
		case OP_WAVE_MAX_U32: k_wave_max_u32<<<g, b>>>(a, dBase); break;
		case OP_WAVE_MAX_U32_GUARDED: k_wave_max_u32_guarded<<<g, b>>>(a, dBase); break;
		case OP_WAVE_MIN_U32: k_wave_min_u32<<<g, b>>>(a, dBase); break;
		case OP_BLOCK_MAX_U32: k_block_max_u32<<<g, b>>>(a, dBase); break;
		case OP_BLOCK_MAX_IF_ABOVE: k_block_max_if_above<<<g, b>>>(a, (int*)dBase); break;
		case OP_BLOCK_HOT: k_block_hot<<<g, b>>>(a, (int*)dBase); break;
		case OP_BLOCK_ALLOC: k_block_alloc<<<g, b>>>(a, (int*)dBase); break;
		case OP_WAVE_KEYED_ALLOC: k_wave_keyed_alloc<<<g, b>>>(a, (int*)dBase); break;
		case OP_WAVE_RUN_ALLOC: k_wave_run_alloc<<<g, b>>>(a, (int*)dBase); break;
		case OP_WAVE_KEYED_ALLOC_ONCE: k_wave_keyed_alloc_once<<<g, b>>>(a, (int*)dBase); break;
		default: k_block_keyed_alloc65<<<g, b>>>(a, (int*)dBase); break;
		}
		err = hipGetLastError();
		if (err == hipSuccess) err = hipDeviceSynchronize();
	}
	if (err == hipSuccess) err = hipMemcpy(base, dBase, (size_t)baseLen * sizeof(uint32_t), hipMemcpyDeviceToHost);
	if (err == hipSuccess && slots && total) err = hipMemcpy(slots, dSlots, total * sizeof(int), hipMemcpyDeviceToHost);
	void* all[5] = { dKey, dVal, dValid, dSlots, dBase };
	for (void* p : all)
		if (p)
		{
			const hipError_t e = hipFree(p);
			if (err == hipSuccess) err = e;
		}
	return (int)err;
}

} // extern "C"
