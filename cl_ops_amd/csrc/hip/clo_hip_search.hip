// clo_hip_search.hip — lower and upper bounds of many keys (the needles) in a sorted array (the haystack): CloSearch,
// include/clo_search.h; not upstream. pos_out[i] = how many haystack keys are < (lower) or <= (upper)
// needles[i], in the order of the sorts and the merge (clo_keyx_fwd, then unsigned).
//
// GENERAL (any needles), one launch: a grid-stride loop over tiles of TILE needles. A work-group first stages in LDS,
//   in unsigned order, the whole haystack if it has at most LDS_KEYS keys, else PIVOTS evenly spaced keys
//   hay[k * numel_h / PIVOTS] (64-bit arithmetic). A needle's search then runs in LDS entirely, or its first
//   log2 PIVOTS steps do and the remaining log2(numel_h / PIVOTS) steps are dependent global loads.
// SORTED NEEDLES (the caller's promise), two launches, neither of which waits for another work-group:
//   PARTITION  one thread per tile searches the haystack for the lower bound of the tile's first needle and the upper
//              bound of its last and writes both to the workspace (8 bytes per tile);
//   SEARCH     one work-group per tile CLAMPS the two to what numel_h allows, stages that range of the haystack in LDS
//              if it has at most LDS_KEYS keys and searches there; a longer range is searched in global memory.
// Every search is the branch-free halving of a range [base, base + n) that is set before its first load: every load
// index is additionally the minimum with the range's last index, every result is at most base + n <= numel_h.
// Whatever the arrays hold (an unsorted haystack, unsorted needles under the promise) reads stay inside the inputs,
// positions written are <= numel_h and the trip counts depend on the sizes alone. A thread carries ITEMS needles
// through the steps together, so that their loads are in flight at once.
// Needles come in and positions go out through LDS: 16-byte vectors from the first 16-byte boundary on, single
// elements before it and after the last whole vector (clo_op_stage, clo_hip_op_device.h).
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

constexpr int SEARCH_THREADS = 256;
static_assert(SEARCH_THREADS == CLO_OP_THREADS, "the shared helpers stride by CLO_OP_THREADS");
constexpr int SEARCH_ITEMS = 4;
constexpr unsigned SEARCH_TILE = SEARCH_THREADS * SEARCH_ITEMS;
constexpr unsigned SEARCH_LDS_KEYS = 4096;
constexpr unsigned SEARCH_PIVOTS_LOG2 = 10;
constexpr unsigned SEARCH_PIVOTS = 1u << SEARCH_PIVOTS_LOG2;
constexpr unsigned SEARCH_GROUPS = 256 * 8;   // the general path's grid when the caller sets no bound
static_assert(SEARCH_PIVOTS <= SEARCH_LDS_KEYS, "the pivots live where a staged haystack would");

// For each of N needles x[k]: base[k] + how many keys of h[base[k], base[k] + n[k]) are < x[k] (upper: <= x[k]), the
// keys ascending. nmax >= every n[k] sets the number of steps. Loads are of h[<= last] only; the callers pass a last
// that is the last index of a non-empty array containing every range. Whatever h holds the result lies in
// [base[k], base[k] + n[k]]. XF: h is raw and goes through clo_keyx_fwd first (x already has).
template <typename TK, bool XF, int N>
__device__ __forceinline__ void search_halve(const TK* h, unsigned (&base)[N], unsigned (&n)[N], const TK (&x)[N], unsigned nmax,
	unsigned last, bool upper, const clo_keyx& kx) {
	for (unsigned m = nmax; m > 1u; m -= m >> 1) {
		TK v[N];
		#pragma unroll
		for (int k = 0; k < N; ++k) v[k] = h[clo_op_min(base[k] + (n[k] >> 1) - (n[k] > 1u ? 1u : 0u), last)];
		#pragma unroll
		for (int k = 0; k < N; ++k) {
			const TK y = XF ? clo_keyx_fwd<TK>(v[k], kx) : v[k];
			const unsigned half = n[k] > 1u ? n[k] >> 1 : 0u;
			const bool below = upper ? y <= x[k] : y < x[k];
			base[k] += below ? half : 0u;
			n[k] -= half;
		}
	}
	TK v[N];
	#pragma unroll
	for (int k = 0; k < N; ++k) v[k] = h[clo_op_min(base[k], last)];
	#pragma unroll
	for (int k = 0; k < N; ++k) {
		const TK y = XF ? clo_keyx_fwd<TK>(v[k], kx) : v[k];
		const bool below = upper ? y <= x[k] : y < x[k];
		base[k] += (n[k] == 1u && below) ? 1u : 0u;
	}
}

// One needle, one range [0, n) of the haystack, n > 0: the partition's form of the same search.
template <typename TK>
__device__ __forceinline__ unsigned search_one(const TK* h, unsigned n, TK x, bool upper, const clo_keyx& kx) {
	unsigned base[1] = { 0u }, len[1] = { n };
	const TK xs[1] = { x };
	search_halve<TK, true, 1>(h, base, len, xs, n, n - 1u, upper, kx);
	return base[0];
}

// dst[0, count) = src[0, count) (LDS), clo_op_stage's division: 16-byte vector stores where dst allows them. (Not
// clo_op_store: it copies from an array and calls no functor.)
__device__ __forceinline__ void search_store(unsigned* __restrict__ dst, unsigned count, const unsigned* src, unsigned tid) {
	typedef unsigned vec __attribute__((ext_vector_type(4)));
	const unsigned head = clo_op_min((unsigned) ((16u - ((uintptr_t) dst & 15u)) & 15u) / 4u, count);
	const unsigned nvec = (count - head) / 4u, body_end = head + nvec * 4u;
	for (unsigned v = tid; v < nvec; v += SEARCH_THREADS) {
		const unsigned i0 = head + v * 4u;
		vec x;
		#pragma unroll
		for (unsigned c = 0; c < 4u; ++c) x[c] = src[i0 + c];
		*reinterpret_cast<vec*>(dst + i0) = x;
	}
	const unsigned rest = head + (count - body_end);
	if (tid < rest) {
		const unsigned i = tid < head ? tid : body_end + (tid - head);
		dst[i] = src[i];
	}
}

// k * numel_h / PIVOTS: where pivot k lies, 0 for k = 0 and numel_h for k = PIVOTS
__device__ __forceinline__ unsigned search_pivot_at(unsigned k, unsigned numel_h) {
	return (unsigned) (((unsigned long long) k * numel_h) >> SEARCH_PIVOTS_LOG2);
}

// SORTED: the needles are promised ascending and `part` holds the tiles' ranges.
template <typename TK, bool SORTED>
__global__ __launch_bounds__(SEARCH_THREADS)
void clo_search_kernel(const TK* __restrict__ hay, unsigned numel_h, const TK* __restrict__ ndl, unsigned numel_n, unsigned tiles,
	unsigned upper_, const unsigned* __restrict__ part, unsigned* __restrict__ pos, clo_keyx kx) {
	__shared__ __attribute__((aligned(16))) TK s_hay[SEARCH_LDS_KEYS];
	__shared__ __attribute__((aligned(16))) TK s_ndl[SEARCH_TILE];
	__shared__ __attribute__((aligned(16))) unsigned s_pos[SEARCH_TILE];
	const unsigned tid = threadIdx.x;
	const bool upper = upper_ != 0u;
	const bool whole = numel_h <= SEARCH_LDS_KEYS;   // GENERAL: the haystack itself is staged, else its pivots

	if constexpr (!SORTED) {
		if (whole) {
			clo_op_stage<TK, true>(hay, numel_h, s_hay, kx, tid);
		} else {
			for (unsigned k = tid; k < SEARCH_PIVOTS; k += SEARCH_THREADS)
				s_hay[k] = clo_keyx_fwd<TK>(hay[search_pivot_at(k, numel_h)], kx);   // k numel_h / PIVOTS < numel_h
		}
	}

	for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
		const unsigned n0 = tile * SEARCH_TILE;                         // tiles * TILE < 2^32 + TILE: n0 < numel_n does not wrap
		const unsigned cnt = clo_op_min(SEARCH_TILE, numel_n - n0);     // the clamp of the last partial tile
		clo_op_stage<TK, true>(ndl + n0, cnt, s_ndl, kx, tid);

		// the tile's range [r0, r0 + len) of the haystack: the partition's two results clamped to r0 <= r1 <= numel_h
		unsigned r0 = 0u, len = numel_h;
		if constexpr (SORTED) {
			r0 = clo_op_min(part[2u * tile], numel_h);
			len = clo_op_min(clo_op_max(part[2u * tile + 1u], r0), numel_h) - r0;
			if (len > 0u && len <= SEARCH_LDS_KEYS) clo_op_stage<TK, true>(hay + r0, len, s_hay, kx, tid);
		}
		__syncthreads();   // s_ndl, s_hay; and every thread has left the previous tile's store of s_pos

		TK x[SEARCH_ITEMS];
		unsigned base[SEARCH_ITEMS], n[SEARCH_ITEMS];
		#pragma unroll
		for (int k = 0; k < SEARCH_ITEMS; ++k) x[k] = s_ndl[tid + k * SEARCH_THREADS];   // past cnt: whatever LDS holds, searched in bounds like any key, not stored
		if (len == 0u) {
			#pragma unroll
			for (int k = 0; k < SEARCH_ITEMS; ++k) base[k] = r0;
		} else if (SORTED ? len <= SEARCH_LDS_KEYS : whole) {
			#pragma unroll
			for (int k = 0; k < SEARCH_ITEMS; ++k) { base[k] = 0u; n[k] = len; }
			search_halve<TK, false, SEARCH_ITEMS>(s_hay, base, n, x, len, len - 1u, upper, kx);
			#pragma unroll
			for (int k = 0; k < SEARCH_ITEMS; ++k) base[k] += r0;
		} else if constexpr (SORTED) {
			#pragma unroll
			for (int k = 0; k < SEARCH_ITEMS; ++k) { base[k] = r0; n[k] = len; }
			search_halve<TK, true, SEARCH_ITEMS>(hay, base, n, x, len, r0 + len - 1u, upper, kx);
		} else {
			// c pivots are below the needle: the answer lies in (at(c - 1), at(c)], at(PIVOTS) = numel_h; c = 0: it is 0
			#pragma unroll
			for (int k = 0; k < SEARCH_ITEMS; ++k) { base[k] = 0u; n[k] = SEARCH_PIVOTS; }
			search_halve<TK, false, SEARCH_ITEMS>(s_hay, base, n, x, SEARCH_PIVOTS, SEARCH_PIVOTS - 1u, upper, kx);
			#pragma unroll
			for (int k = 0; k < SEARCH_ITEMS; ++k) {
				const unsigned c = base[k];
				base[k] = c ? search_pivot_at(c - 1u, numel_h) + 1u : 0u;
				n[k] = search_pivot_at(c, numel_h) - base[k];           // at(c) > at(c - 1): numel_h > PIVOTS
			}
			search_halve<TK, true, SEARCH_ITEMS>(hay, base, n, x, (numel_h >> SEARCH_PIVOTS_LOG2) + 1u, numel_h - 1u, upper, kx);
		}
		#pragma unroll
		for (int k = 0; k < SEARCH_ITEMS; ++k) s_pos[tid + k * SEARCH_THREADS] = base[k];
		__syncthreads();   // s_pos; and every thread has read its needles and its part of s_hay
		search_store(pos + n0, cnt, s_pos, tid);
	}
}

template <typename TK>
__global__ __launch_bounds__(SEARCH_THREADS)
void clo_search_partition_kernel(const TK* __restrict__ hay, unsigned numel_h, const TK* __restrict__ ndl, unsigned numel_n, unsigned tiles,
	clo_keyx kx, unsigned* __restrict__ part) {
	const unsigned t = blockIdx.x * SEARCH_THREADS + threadIdx.x;
	if (t >= tiles) return;
	const unsigned n0 = t * SEARCH_TILE, n1 = n0 + clo_op_min(SEARCH_TILE, numel_n - n0);   // n0 < n1 <= numel_n
	part[2u * t] = search_one<TK>(hay, numel_h, clo_keyx_fwd<TK>(ndl[n0], kx), false, kx);
	part[2u * t + 1u] = search_one<TK>(hay, numel_h, clo_keyx_fwd<TK>(ndl[n1 - 1u], kx), true, kx);
}

struct search_args {
	const void* hay; const void* ndl; unsigned* pos; unsigned numel_h, numel_n, upper, max_groups; bool sorted;
	clo_keyx kx; unsigned* part; hipStream_t s;
};

template <typename TK>
int search_launch(const search_args& a) {
	const unsigned tiles = (unsigned) (((size_t) a.numel_n + SEARCH_TILE - 1) / SEARCH_TILE);
	unsigned groups = a.sorted || tiles < SEARCH_GROUPS ? tiles : SEARCH_GROUPS;
	if (a.max_groups != 0 && groups > a.max_groups) groups = a.max_groups;
	if (a.sorted) {
		{
			clo_timing_scope timing("search_partition", a.s);
			hipLaunchKernelGGL((clo_search_partition_kernel<TK>), dim3((tiles + SEARCH_THREADS - 1) / SEARCH_THREADS), dim3(SEARCH_THREADS), 0, a.s,
				(const TK*) a.hay, a.numel_h, (const TK*) a.ndl, a.numel_n, tiles, a.kx, a.part);
			const hipError_t e = hipGetLastError();
			if (e != hipSuccess) return (int) e;
		}
		clo_timing_scope timing("search_sorted", a.s);
		hipLaunchKernelGGL((clo_search_kernel<TK, true>), dim3(groups), dim3(SEARCH_THREADS), 0, a.s,
			(const TK*) a.hay, a.numel_h, (const TK*) a.ndl, a.numel_n, tiles, a.upper, (const unsigned*) a.part, a.pos, a.kx);
		return (int) hipGetLastError();
	}
	clo_timing_scope timing("search", a.s);
	hipLaunchKernelGGL((clo_search_kernel<TK, false>), dim3(groups), dim3(SEARCH_THREADS), 0, a.s,
		(const TK*) a.hay, a.numel_h, (const TK*) a.ndl, a.numel_n, tiles, a.upper, (const unsigned*) nullptr, a.pos, a.kx);
	return (int) hipGetLastError();
}

// the partition is worth its launch only where there is a haystack to partition
inline bool search_partitions(size_t numel_h, size_t numel_n, unsigned flags) {
	return (flags & CLO_HIP_SEARCH_NEEDLES_SORTED) != 0 && numel_h > 0 && numel_n > 0;
}

}  // namespace

extern "C" {

size_t clo_hip_search_tile(int key_size) { return clo_op_key_size_ok(key_size) ? SEARCH_TILE : 0; }
size_t clo_hip_search_lds_keys(int key_size) { return clo_op_key_size_ok(key_size) ? SEARCH_LDS_KEYS : 0; }
size_t clo_hip_search_pivots(int key_size) { return clo_op_key_size_ok(key_size) ? SEARCH_PIVOTS : 0; }

size_t clo_hip_search_workspace_bytes(size_t numel_h, size_t numel_n, unsigned flags) {
	if (!search_partitions(numel_h, numel_n, flags)) return 0;
	// two words per tile, in whole CLO_HIP_WORKSPACE_ALIGN units
	return clo_op_ws_align(((numel_n + SEARCH_TILE - 1) / SEARCH_TILE) * 2 * sizeof(unsigned));
}

int clo_hip_search(const void* haystack, size_t numel_h, const void* needles, size_t numel_n, void* pos_out,
	int key_size, int key_kind, unsigned flags, unsigned max_groups, void* workspace, size_t workspace_bytes, void* stream) {
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (flags & ~(CLO_HIP_SEARCH_UPPER | CLO_HIP_SEARCH_NEEDLES_SORTED)) return CLO_HIP_EARGS;
	if (numel_h > 0xffffffffull || numel_n > 0xffffffffull) return CLO_HIP_EARGS;
	if (numel_h > 0 && !haystack) return CLO_HIP_EARGS;
	if (numel_n > 0 && (!needles || !pos_out)) return CLO_HIP_EARGS;
	if ((numel_h > 0 && clo_misaligned(haystack, (size_t) key_size)) || clo_misaligned(needles, (size_t) key_size)
		|| clo_misaligned(pos_out, sizeof(unsigned))) return CLO_HIP_EARGS;
	if (numel_n == 0) return 0;
	const size_t need = clo_hip_search_workspace_bytes(numel_h, numel_n, flags);
	if (need > 0) {
		if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
		if (workspace_bytes < need) return CLO_HIP_EWORKSPACE;
	}

	search_args a;
	a.hay = haystack; a.ndl = needles; a.pos = (unsigned*) pos_out;
	a.numel_h = (unsigned) numel_h; a.numel_n = (unsigned) numel_n;
	a.upper = (flags & CLO_HIP_SEARCH_UPPER) ? 1u : 0u; a.max_groups = max_groups;
	a.sorted = need > 0;
	a.kx = clo_keyx_make(key_kind, 0, 8 * key_size);
	a.part = (unsigned*) workspace; a.s = (hipStream_t) stream;
	return clo_op_by_key_size(key_size, [&](auto tk) { return search_launch<decltype(tk)>(a); });
}

}  // extern "C"
