// clo_hip_setop.hip — union, intersection, difference and symmetric difference of two sorted arrays as multisets
// (CloSetOp, include/clo_setop.h; not upstream), with values carried along or the indices written.
//
// The result is the subsequence of the stable merge of A and B that a KEEP rule selects. Pair the r-th element of a
// run of equal keys in A with the r-th element of the same run in B: an element with a partner is MATCHED. Then
//   union = all of A + the unmatched of B      intersection = the matched of A
//   difference = the unmatched of A            symmetric difference = the unmatched of A + the unmatched of B.
// A[i] with key x is matched iff i - lbA(x) < ubB(x) - lbB(x), B[j] iff j - lbB(x) < ubA(x) - lbA(x), lb and ub being
// the lower and upper bounds of x in the whole arrays.
//
// Four launches, none of which waits for another work-group and none of which uses an atomic:
//   PARTITION  the merge's diagonal search, one thread per tile boundary of the MERGED sequence -> split[tiles + 1];
//   COUNT      one work-group per tile: clamps its splits as the merge does, stages its range of A and of B in LDS,
//              merges, decides keep for every merged element and writes the tile's kept count -> count[tiles];
//   SCAN       one work-group turns the counts into exclusive offsets in place and writes num_out = min(total, capacity);
//   APPLY      the same merge and the same keep function; the kept elements are compacted in LDS in merge order and
//              stored at the tile's offset, every store index below the capacity.
// The bounds of x inside the tile come from the staged ranges. While the serial merge stands at (ai, bi), everything
// consumed lies before everything not consumed, so lbB(x) = bi for an element taken from A and ubA(y) = ai for one taken
// from B; the other bounds are one compare with the neighbouring key, which the merge carries in registers, and a binary
// search in LDS only where that neighbour is equal, once per distinct key of a thread. Only the runs of the tile's FIRST and LAST key can reach outside the tile: four lanes
// find lbA and lbB of the first key and ubA and ubB of the last one in global memory — one load of the element next to
// the tile, requested before the tile is staged, and a clamped binary search only if it is equal.
// Unsorted inputs: whatever the searches find only changes which elements are kept. Splits are clamped, every search
// reads inside [0, na) or [0, nb) or the staged range, COUNT and APPLY run the same code on the same data and so agree,
// and APPLY clamps what it stores to the capacity.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

constexpr int SETOP_THREADS = 256;
static_assert(SETOP_THREADS == CLO_OP_THREADS, "the shared helpers stride by CLO_OP_THREADS");
constexpr int SETOP_WAVES = SETOP_THREADS / 64;
constexpr int setop_items(int key_size) { return key_size <= 2 ? 17 : 9; }
constexpr size_t setop_tile(int key_size) { return (size_t) SETOP_THREADS * setop_items(key_size); }
constexpr size_t SETOP_MIN_TILE = setop_tile(8);   // sizes the workspace, whose getter does not know the key size
constexpr unsigned SETOP_SCAN_ITEMS = 8;           // the scan sweeps SETOP_THREADS * SETOP_SCAN_ITEMS counts at a time

// the modes CLO_OP_KEYS, V4, V8 and ARG (clo_hip_op_device.h); the table keeps a name of its own here because the
// kernels' symbols spell it
template <int MODE> struct setop_val : clo_op_val<MODE> {};

// The keep rule. matched: the element has a partner of the same rank in the other array's run of its key.
__device__ __forceinline__ bool setop_keep(int op, bool from_a, bool matched) {
	switch (op) {
		case CLO_HIP_SETOP_UNION: return from_a || !matched;
		case CLO_HIP_SETOP_INTERSECTION: return from_a && matched;
		case CLO_HIP_SETOP_DIFFERENCE: return from_a && !matched;
		default: return !matched;
	}
}

// The first index in [lo, hi) whose key is not below x (UPPER: is above x), hi if there is none. Reads k[lo, hi) only.
template <typename TK, bool XF, bool UPPER>
__device__ __forceinline__ unsigned setop_bound(const TK* k, unsigned lo, unsigned hi, TK x, const clo_keyx& kx) {
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		TK y = k[mid];
		if constexpr (XF) y = clo_keyx_fwd<TK>(y, kx);
		if (UPPER ? y <= x : y < x) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

template <typename TK>
__global__ __launch_bounds__(SETOP_THREADS)
void clo_setop_partition_kernel(const TK* __restrict__ ka, const TK* __restrict__ kb, unsigned na, unsigned nb, unsigned tiles,
	clo_keyx kx, unsigned* __restrict__ split) {
	clo_op_partition<TK, setop_tile((int) sizeof(TK))>(ka, kb, na, nb, tiles, kx, split);
}

// The exclusive sum of v over the work-group's threads and the sum of all. One barrier; s_wave must not be written
// again before every thread has left. (Not clo_op_block_scan: the waves are scanned with __shfl_up here, which is
// another sequence of instructions.)
__device__ __forceinline__ unsigned setop_block_scan(unsigned v, unsigned* s_wave, unsigned tid, unsigned& total) {
	const unsigned lane = tid & 63u;
	unsigned inc = v;
	#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned t = __shfl_up(inc, d, 64);
		if (lane >= (unsigned) d) inc += t;
	}
	if (lane == 63u) s_wave[tid >> 6] = inc;
	__syncthreads();
	unsigned before = 0;
	total = 0;
	#pragma unroll
	for (unsigned w = 0; w < (unsigned) SETOP_WAVES; ++w) {
		const unsigned s = s_wave[w];
		if (w < (tid >> 6)) before += s;
		total += s;
	}
	return before + inc - v;
}

// Lane 0 of wave w loads the key next to the tile that decides whether a run reaches outside it: w = 0 A[a0 - 1], 1 B[b0 -
// 1], 2 A[a1], 3 B[b1] (unsigned order; ok: there is one). Requested before the tile is staged, looked at after it.
template <typename TK>
__device__ __forceinline__ TK setop_neighbour(const TK* __restrict__ ka, const TK* __restrict__ kb, unsigned na, unsigned nb,
	const clo_op_range& r, const clo_keyx& kx, unsigned tid, bool& ok) {
	ok = false;
	if ((tid & 63u) != 0) return (TK) 0;
	const unsigned w = tid >> 6, a1 = r.a0 + r.na_t, b1 = r.b0 + r.nb_t;
	const TK* k = (w & 1u) ? kb : ka;
	const unsigned i = w == 0 ? r.a0 - 1u : w == 1 ? r.b0 - 1u : w == 2 ? a1 : b1;
	ok = w == 0 ? r.a0 > 0 : w == 1 ? r.b0 > 0 : w == 2 ? a1 < na : b1 < nb;
	return ok ? clo_keyx_fwd<TK>(k[i], kx) : (TK) 0;
}

// After the tile's keys are staged (A at s_keys[0, na_t), B behind it, unsigned order) and a barrier: merges this
// thread's ITEMS outputs and decides keep for each. Returns the keep bits; out[i] is the key (unsigned order) and
// slot[i] the LDS slot of output tid * ITEMS + i. One barrier inside. s_g: four words of LDS.
template <typename TK, int ITEMS>
__device__ __forceinline__ unsigned setop_decide(const TK* __restrict__ ka, const TK* __restrict__ kb, unsigned na, unsigned nb,
	const clo_op_range& r, const TK* s_keys, unsigned* s_g, TK nbr, bool nbr_ok, int op, const clo_keyx& kx, unsigned tid,
	TK (&out)[ITEMS], unsigned (&slot)[ITEMS]) {
	constexpr unsigned TILE = (unsigned) SETOP_THREADS * ITEMS;
	const unsigned na_t = r.na_t, nb_t = r.nb_t, cnt = r.cnt, a0 = r.a0, b0 = r.b0;
	const TK* sa = s_keys;
	const TK* sb = s_keys + na_t;
	// the tile's first and last key (cnt > 0): only their runs can begin before the tile or end after it
	const TK a_lo = s_keys[0], a_hi = s_keys[na_t > 0 ? na_t - 1u : 0u], b_lo = s_keys[clo_op_min(na_t, TILE - 1u)], b_hi = s_keys[cnt - 1u];
	const TK kfirst = na_t == 0 ? b_lo : nb_t == 0 ? a_lo : (a_lo < b_lo ? a_lo : b_lo);
	const TK klast = na_t == 0 ? b_hi : nb_t == 0 ? a_hi : (a_hi > b_hi ? a_hi : b_hi);
	if ((tid & 63u) == 0) {
		const unsigned w = tid >> 6, a1 = a0 + na_t, b1 = b0 + nb_t;
		unsigned g;
		if (w == 0) { g = a0; if (nbr_ok && nbr == kfirst) g = setop_bound<TK, true, false>(ka, 0u, a0 - 1u, kfirst, kx); }
		else if (w == 1) { g = b0; if (nbr_ok && nbr == kfirst) g = setop_bound<TK, true, false>(kb, 0u, b0 - 1u, kfirst, kx); }
		else if (w == 2) { g = a1; if (nbr_ok && nbr == klast) g = setop_bound<TK, true, true>(ka, a1 + 1u, na, klast, kx); }
		else { g = b1; if (nbr_ok && nbr == klast) g = setop_bound<TK, true, true>(kb, b1 + 1u, nb, klast, kx); }
		s_g[w] = g;
	}
	// this thread's ITEMS outputs start at diagonal tid * ITEMS of the tile; past cnt nothing is valid
	const unsigned diag = clo_op_min(tid * ITEMS, cnt);
	unsigned ai = clo_op_path<TK, false>(sa, sb, na_t, nb_t, diag, kx);
	unsigned bi = diag - ai;
	__syncthreads();
	const unsigned g_lba = s_g[0], g_lbb = s_g[1], g_uba = s_g[2], g_ubb = s_g[3];

	TK x = s_keys[clo_op_min(ai, TILE - 1u)], y = s_keys[clo_op_min(na_t + bi, TILE - 1u)];
	// the keys just before them, pa = A[ai - 1] and pb = B[bi - 1] where there are such: carried along in registers
	bool has_pa = ai > 0, has_pb = bi > 0;
	TK pa = s_keys[has_pa ? ai - 1u : 0u], pb = s_keys[has_pb ? na_t + bi - 1u : 0u];
	unsigned keep = 0;
	bool c_valid = false, c_ub_valid = false;   // the bounds of c_key inside the tile, found once per distinct key
	TK c_key = 0;
	unsigned c_lba = 0, c_lbb = 0, c_ubb = 0;
	#pragma unroll
	for (int i = 0; i < ITEMS; ++i) {
		// x is looked at only while ai < na_t, y only while bi < nb_t
		const bool from_a = bi >= nb_t || (ai < na_t && x <= y);
		const TK key = from_a ? x : y;
		out[i] = key;
		slot[i] = from_a ? ai : na_t + bi;
		if (tid * ITEMS + i < cnt) {
			if (!c_valid || key != c_key) {
				// everything of A below ai is <= key, everything of B below bi is <= key (< key for an element of A)
				c_lba = (has_pa && pa == key) ? setop_bound<TK, false, false>(sa, 0u, ai - 1u, key, kx) : ai;
				c_lbb = (has_pb && pb == key) ? setop_bound<TK, false, false>(sb, 0u, bi - 1u, key, kx) : bi;
				c_key = key;
				c_valid = true;
				c_ub_valid = false;
			}
			const bool is_first = key == kfirst, is_last = key == klast;
			const unsigned lba = is_first ? g_lba : a0 + c_lba, lbb = is_first ? g_lbb : b0 + c_lbb;
			bool matched;
			if (from_a) {
				if (!c_ub_valid) {   // B[bi] is the first key of B not below this one
					c_ubb = (bi < nb_t && y == key) ? setop_bound<TK, false, true>(sb, bi + 1u, nb_t, key, kx) : bi;
					c_ub_valid = true;
				}
				const unsigned ubb = is_last ? g_ubb : b0 + c_ubb;
				matched = (a0 + ai - lba) < (ubb - lbb);
			} else {             // A[ai] is the first key of A above this one
				const unsigned uba = is_last ? g_uba : a0 + ai;
				matched = (b0 + bi - lbb) < (uba - lba);
			}
			if (setop_keep(op, from_a, matched)) keep |= 1u << i;
		}
		if (from_a) { pa = x; has_pa = true; ++ai; } else { pb = y; has_pb = true; ++bi; }
		const TK next = s_keys[clo_op_min(from_a ? ai : na_t + bi, TILE - 1u)];
		if (from_a) x = next; else y = next;
	}
	return keep;
}

template <typename TK>
__global__ __launch_bounds__(SETOP_THREADS)
void clo_setop_count_kernel(const TK* __restrict__ ka, unsigned na, const TK* __restrict__ kb, unsigned nb,
	const unsigned* __restrict__ split, unsigned* __restrict__ count, int op, clo_keyx kx) {
	constexpr int ITEMS = setop_items((int) sizeof(TK));
	constexpr unsigned TILE = (unsigned) setop_tile((int) sizeof(TK));
	__shared__ __attribute__((aligned(16))) TK s_keys[TILE];
	__shared__ unsigned s_g[4], s_wave[SETOP_WAVES];
	const unsigned tid = threadIdx.x;
	const clo_op_range r = clo_op_tile_range<TILE>(split, na, nb);
	bool nbr_ok;
	const TK nbr = setop_neighbour<TK>(ka, kb, na, nb, r, kx, tid, nbr_ok);
	clo_op_stage<TK, true>(ka + r.a0, r.na_t, s_keys, kx, tid);
	clo_op_stage<TK, true>(kb + r.b0, r.nb_t, s_keys + r.na_t, kx, tid);
	__syncthreads();
	TK out[ITEMS];
	unsigned slot[ITEMS];
	const unsigned keep = setop_decide<TK, ITEMS>(ka, kb, na, nb, r, s_keys, s_g, nbr, nbr_ok, op, kx, tid, out, slot);
	unsigned total;
	setop_block_scan((unsigned) __popc(keep), s_wave, tid, total);
	if (tid == 0) count[blockIdx.x] = total;
}

// count[0, tiles) -> its exclusive sums in place; *num_out = min(sum of all, cap). One work-group; the next sweep's
// counts are requested before this sweep's are summed. tiles 0: only num_out is written.
__global__ __launch_bounds__(SETOP_THREADS)
void clo_setop_scan_kernel(unsigned* __restrict__ count, unsigned tiles, unsigned long long cap, unsigned long long* __restrict__ num_out) {
	constexpr unsigned SWEEP = SETOP_THREADS * SETOP_SCAN_ITEMS;
	__shared__ unsigned s_wave[SETOP_WAVES];
	const unsigned tid = threadIdx.x;
	unsigned carry = 0;   // the sum of all counts is at most numel_a + numel_b < 2^32
	unsigned v[SETOP_SCAN_ITEMS], ahead[SETOP_SCAN_ITEMS];
	#pragma unroll
	for (unsigned c = 0; c < SETOP_SCAN_ITEMS; ++c) {
		const unsigned i = tid * SETOP_SCAN_ITEMS + c;
		ahead[c] = i < tiles ? count[i] : 0u;
	}
	for (unsigned base = 0; base < tiles; base += SWEEP) {
		unsigned sum = 0;
		#pragma unroll
		for (unsigned c = 0; c < SETOP_SCAN_ITEMS; ++c) {
			v[c] = ahead[c];
			sum += v[c];
			const unsigned long long i = (unsigned long long) base + SWEEP + tid * SETOP_SCAN_ITEMS + c;
			ahead[c] = i < tiles ? count[i] : 0u;
		}
		unsigned total;
		unsigned at = carry + setop_block_scan(sum, s_wave, tid, total);
		#pragma unroll
		for (unsigned c = 0; c < SETOP_SCAN_ITEMS; ++c) {
			const unsigned i = base + tid * SETOP_SCAN_ITEMS + c;   // < tiles + SWEEP: no wrap, tiles < 2^21
			if (i < tiles) count[i] = at;
			at += v[c];
		}
		carry += total;
		__syncthreads();   // s_wave is written again
	}
	if (tid == 0) *num_out = carry < cap ? carry : cap;
}

template <typename TK, int MODE>
__global__ __launch_bounds__(SETOP_THREADS)
void clo_setop_apply_kernel(const TK* __restrict__ ka, const typename setop_val<MODE>::T* __restrict__ va, unsigned na,
	const TK* __restrict__ kb, const typename setop_val<MODE>::T* __restrict__ vb, unsigned nb,
	TK* __restrict__ kout, typename setop_val<MODE>::T* __restrict__ vout, const unsigned* __restrict__ split,
	const unsigned* __restrict__ offset, unsigned cap, int op, clo_keyx kx) {
	typedef typename setop_val<MODE>::T TV;
	constexpr int ITEMS = setop_items((int) sizeof(TK));
	constexpr unsigned TILE = (unsigned) setop_tile((int) sizeof(TK));
	constexpr bool VALS = MODE == CLO_OP_V4 || MODE == CLO_OP_V8;
	static_assert(TILE <= 65536u, "slots are 16-bit");
	__shared__ __attribute__((aligned(16))) TK s_keys[TILE];
	__shared__ unsigned short s_slot[MODE == CLO_OP_KEYS ? 1 : TILE];
	__shared__ __attribute__((aligned(16))) TV s_vals[VALS ? TILE : 1];
	__shared__ unsigned s_g[4], s_wave[SETOP_WAVES];
	const unsigned tid = threadIdx.x;
	const clo_op_range r = clo_op_tile_range<TILE>(split, na, nb);
	const bool keeps_b = op == CLO_HIP_SETOP_UNION || op == CLO_HIP_SETOP_SYMMETRIC_DIFFERENCE;
	bool nbr_ok;
	const TK nbr = setop_neighbour<TK>(ka, kb, na, nb, r, kx, tid, nbr_ok);

	clo_op_stage<TK, true>(ka + r.a0, r.na_t, s_keys, kx, tid);
	clo_op_stage<TK, true>(kb + r.b0, r.nb_t, s_keys + r.na_t, kx, tid);
	if constexpr (VALS) {   // requested now, needed after the merge; no element of B leaves an intersection or a difference
		clo_op_stage<TV, false>(va + r.a0, r.na_t, s_vals, kx, tid);
		if (keeps_b) clo_op_stage<TV, false>(vb + r.b0, r.nb_t, s_vals + r.na_t, kx, tid);
	}
	__syncthreads();
	TK out[ITEMS];
	unsigned slot[ITEMS];
	const unsigned keep = setop_decide<TK, ITEMS>(ka, kb, na, nb, r, s_keys, s_g, nbr, nbr_ok, op, kx, tid, out, slot);
	unsigned kept;
	unsigned at = setop_block_scan((unsigned) __popc(keep), s_wave, tid, kept);
	// (the scan's barrier: every thread has read its keys, s_keys becomes the compacted output)
	#pragma unroll
	for (int i = 0; i < ITEMS; ++i) {
		if (keep >> i & 1u) {   // at < kept <= cnt
			s_keys[at] = clo_keyx_inv<TK>(out[i], kx);
			if constexpr (MODE != CLO_OP_KEYS) s_slot[at] = (unsigned short) slot[i];
			++at;
		}
	}
	__syncthreads();
	// the tile's rows land at [off, off + kept) of the outputs; nothing is stored at or above the capacity
	const unsigned off = offset[blockIdx.x];
	const unsigned rows = off < cap ? clo_op_min(kept, cap - off) : 0u;
	if (kout) clo_op_store<TK>(kout + off, rows, tid, [&](unsigned j) { return s_keys[j]; });
	if constexpr (VALS) clo_op_store<TV>(vout + off, rows, tid, [&](unsigned j) { return s_vals[s_slot[j]]; });
	if constexpr (MODE == CLO_OP_ARG) {
		const unsigned base_b = na + r.b0 - r.na_t;   // slot s >= na_t is B[b0 + s - na_t], index na + b0 + s - na_t of A || B (mod 2^32: exact)
		clo_op_store<TV>(vout + off, rows, tid, [&](unsigned j) { const unsigned s = s_slot[j]; return s < r.na_t ? r.a0 + s : base_b + s; });
	}
}

struct setop_args {
	const void* ka; const void* va; const void* kb; const void* vb; void* kout; void* vout;
	unsigned na, nb, cap; int op; clo_keyx kx; unsigned* ws; unsigned long long* num_out; hipStream_t s;
};

inline int setop_scan_launch(unsigned* count, unsigned tiles, unsigned cap, unsigned long long* num_out, hipStream_t s) {
	clo_timing_scope timing("setop_scan", s);
	hipLaunchKernelGGL(clo_setop_scan_kernel, dim3(1), dim3(SETOP_THREADS), 0, s, count, tiles, (unsigned long long) cap, num_out);
	return (int) hipGetLastError();
}

template <typename TK, int MODE>
int setop_launch(const setop_args& a) {
	typedef typename setop_val<MODE>::T TV;
	const size_t tile = setop_tile((int) sizeof(TK));
	const unsigned tiles = (unsigned) (((size_t) a.na + a.nb + tile - 1) / tile);
	unsigned* split = a.ws;                  // tiles + 1 words
	unsigned* count = a.ws + tiles + 1u;     // tiles words: the counts, then the offsets
	{
		clo_timing_scope timing("setop_partition", a.s);
		hipLaunchKernelGGL((clo_setop_partition_kernel<TK>), dim3(tiles / SETOP_THREADS + 1u), dim3(SETOP_THREADS), 0, a.s,
			(const TK*) a.ka, (const TK*) a.kb, a.na, a.nb, tiles, a.kx, split);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("setop_count", a.s);
		hipLaunchKernelGGL((clo_setop_count_kernel<TK>), dim3(tiles), dim3(SETOP_THREADS), 0, a.s,
			(const TK*) a.ka, a.na, (const TK*) a.kb, a.nb, (const unsigned*) split, count, a.op, a.kx);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	const int st = setop_scan_launch(count, tiles, a.cap, a.num_out, a.s);
	if (st != 0) return st;
	clo_timing_scope timing("setop_apply", a.s);
	hipLaunchKernelGGL((clo_setop_apply_kernel<TK, MODE>), dim3(tiles), dim3(SETOP_THREADS), 0, a.s,
		(const TK*) a.ka, (const TV*) a.va, a.na, (const TK*) a.kb, (const TV*) a.vb, a.nb, (TK*) a.kout, (TV*) a.vout,
		(const unsigned*) split, (const unsigned*) count, a.cap, a.op, a.kx);
	return (int) hipGetLastError();
}

template <typename TK>
int setop_dispatch(const setop_args& a, int mode) {
	switch (mode) {
		case CLO_OP_KEYS: return setop_launch<TK, CLO_OP_KEYS>(a);
		case CLO_OP_V4: return setop_launch<TK, CLO_OP_V4>(a);
		case CLO_OP_V8: return setop_launch<TK, CLO_OP_V8>(a);
		default: return setop_launch<TK, CLO_OP_ARG>(a);
	}
}

}  // namespace

extern "C" {

size_t clo_hip_setop_tile(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return setop_tile(key_size);
}

size_t clo_hip_setop_workspace_bytes(size_t numel_a, size_t numel_b) {
	const size_t n = numel_a + numel_b;
	if (n == 0 || n < numel_a) return 0;
	// tiles + 1 split points and tiles counts of 4 bytes for the smallest tile, in whole CLO_HIP_WORKSPACE_ALIGN units
	return clo_op_ws_align((2 * ((n + SETOP_MIN_TILE - 1) / SETOP_MIN_TILE) + 1) * sizeof(unsigned));
}

int clo_hip_setop(int op, const void* keys_a, const void* values_a, size_t numel_a, const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, uint64_t* num_out, int key_size, int key_kind, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (op < CLO_HIP_SETOP_UNION || op > CLO_HIP_SETOP_SYMMETRIC_DIFFERENCE) return CLO_HIP_EARGS;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull) return CLO_HIP_EARGS;
	if ((numel_a > 0 && !keys_a) || (numel_b > 0 && !keys_b)) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8)) return CLO_HIP_EARGS;
	if (!keys_out && !values_out) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_a || values_b || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	// the values of an empty input are not looked at, nor are those of B where no element of B is kept; those of the
	// others are all given, or all NULL (the arg form)
	const bool keeps_b = op == CLO_HIP_SETOP_UNION || op == CLO_HIP_SETOP_SYMMETRIC_DIFFERENCE;
	const bool given_a = numel_a > 0 && values_a, given_b = keeps_b && numel_b > 0 && values_b;
	const bool absent_a = numel_a > 0 && !values_a, absent_b = keeps_b && numel_b > 0 && !values_b;
	if ((given_a && absent_b) || (given_b && absent_a)) return CLO_HIP_EARGS;
	const bool arg = value_size > 0 && (absent_a || absent_b);
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	if (clo_misaligned(keys_a, (size_t) key_size) || clo_misaligned(keys_b, (size_t) key_size) || clo_misaligned(keys_out, (size_t) key_size))
		return CLO_HIP_EARGS;
	if (value_size > 0 && (clo_misaligned(values_a, (size_t) value_size) || clo_misaligned(values_b, (size_t) value_size)
		|| clo_misaligned(values_out, (size_t) value_size))) return CLO_HIP_EARGS;
	const size_t n = numel_a + numel_b;
	if (n > 0) {
		if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
		if (workspace_bytes < clo_hip_setop_workspace_bytes(numel_a, numel_b)) return CLO_HIP_EWORKSPACE;
	}
	const size_t cap = keeps_b ? n : op == CLO_HIP_SETOP_DIFFERENCE ? numel_a : (numel_a < numel_b ? numel_a : numel_b);
	if (n == 0) return setop_scan_launch(nullptr, 0u, 0u, (unsigned long long*) num_out, (hipStream_t) stream);   // num_out = 0

	setop_args a;
	a.ka = keys_a; a.va = arg ? nullptr : values_a; a.kb = keys_b; a.vb = arg ? nullptr : values_b;
	a.kout = keys_out; a.vout = values_out;
	a.na = (unsigned) numel_a; a.nb = (unsigned) numel_b; a.cap = (unsigned) cap; a.op = op;
	a.kx = clo_keyx_make(key_kind, 0, 8 * key_size);
	a.ws = (unsigned*) workspace; a.num_out = (unsigned long long*) num_out; a.s = (hipStream_t) stream;
	const int mode = clo_op_mode(value_size, arg);
	return clo_op_by_key_size(key_size, [&](auto tk) { return setop_dispatch<decltype(tk)>(a, mode); });
}

}  // extern "C"
