// clo_hip_expand.hip — run-length decode and segment ids from counts or from CSR offsets (CloExpand,
// include/clo_expand.h; not upstream). With m = min(numel_in, *num_in) segments whose ends are e_r (the
// running sums of the counts, or offsets[r + 1] - offsets[0]), row j < min(total, capacity) belongs to segment r(j) = the
// number of r < m with e_r <= j: values_out[j] = values_in[r(j)], seg_out[j] = r(j), rank_out[j] = j - e_(r(j) - 1).
//
// None of the launches waits for another work-group, none uses a global atomic:
//   ENDS       the counts form only: the numel_in inclusive ends as uint64 in the workspace, entries at r >= m adding 0.
//              Three launches (CloSelect's count scan, in 64 bits): the tiles' sums, one work-group that turns them into
//              exclusive sums CLO_OP_SUMS_TRIP at a time, and the tiles' write. The offsets form is read where it lies.
//   PARTITION  one thread per output tile boundary t * T: first[t] = the number of r < m with e_r <= t * T, 4 bytes per
//              tile in the workspace; thread 0 writes num_out = total.
//   EXPAND     one work-group per tile of T rows. first[t] and first[t + 1] are CLAMPED to [0, m] and ordered; the
//              n = first[t + 1] - first[t] ends between them are the segment starts inside the tile.
//                n == 0     the tile lies inside one segment: nothing but the outputs.
//                n <= L     every end is loaded once, coalesced, and marks the row it starts in an LDS row array with
//                           (segment << 12 | row) by an LDS max, so that of several segments that start in one row — all
//                           but the last are empty — the highest stays; an inclusive max scan over the T rows then
//                           gives every row its segment and where that began.
//                n > L      (more than L - T empty segments inside one tile) every row runs the bounded halving in
//                           global memory.
//              values_in[r] is gathered once r(j) is known; the outputs leave through clo_op_store.
// Whatever the arrays hold: the one halving routine (exp_halve) takes its trip count from numel_in and loads ends at
// indices <= numel_in - 1 only; what comes out of the workspace is clamped (first[]) or only ever compared and added
// (the ends); a mark is placed only at a row below T; every segment id is clamped to numel_in - 1 before it is written
// or gathered by; and the rows stored are [t * T, min(total, capacity)).
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_seg_device.h"

namespace {

typedef unsigned long long exp_u64;

constexpr int EXP_THREADS = 256;
constexpr int EXP_WAVES = EXP_THREADS / 64;
static_assert(EXP_THREADS == CLO_OP_THREADS, "the shared helpers stride by CLO_OP_THREADS, and clo_op_ends_launch launches groups of it");
constexpr unsigned EXP_TILE_LOG2 = 12;
constexpr unsigned EXP_TILE = 1u << EXP_TILE_LOG2;               // T: output rows per tile, for every value size
constexpr unsigned EXP_PER_THREAD = EXP_TILE / EXP_THREADS;      // 16 consecutive rows of the max scan
constexpr unsigned EXP_LDS_SEGMENTS = 4 * EXP_TILE;              // L: (segment << 12 | row) must fit a word
static_assert(((exp_u64) EXP_LDS_SEGMENTS << EXP_TILE_LOG2) < (1ull << 32), "a mark is one word");
constexpr int EXP_HALVE_ITEMS = 4;                               // rows a thread carries through the halving together

// THE halving, the only search there is. For each of N rows x[k]: base[k] + how many of the ends [base[k], base[k] +
// n[k]) are <= x[k], the ends ascending. nmax >= every n[k] sets the number of trips and comes from numel_in; loads are
// of ends at indices <= last = numel_in - 1 only. Whatever the ends hold the result lies in [base[k], base[k] + n[k]].
template <typename E, int N>
__device__ __forceinline__ void exp_halve(const E& e, unsigned (&base)[N], unsigned (&n)[N], const exp_u64 (&x)[N], unsigned nmax, unsigned last) {
	for (unsigned trips = nmax; trips > 1u; trips -= trips >> 1) {
		exp_u64 v[N];
		#pragma unroll
		for (int k = 0; k < N; ++k) v[k] = e.at(clo_op_min(base[k] + (n[k] >> 1) - (n[k] > 1u ? 1u : 0u), last));
		#pragma unroll
		for (int k = 0; k < N; ++k) {
			const unsigned half = n[k] > 1u ? n[k] >> 1 : 0u;
			base[k] += v[k] <= x[k] ? half : 0u;
			n[k] -= half;
		}
	}
	#pragma unroll
	for (int k = 0; k < N; ++k) {
		const exp_u64 v = e.at(clo_op_min(base[k], last));
		base[k] += (n[k] == 1u && v <= x[k]) ? 1u : 0u;
	}
}

// ---- 1. the ends of the counts form: the three launches of clo_hip_seg_device.h ----

template <typename TC>
__global__ __launch_bounds__(EXP_THREADS)
void clo_expand_sums_kernel(const TC* __restrict__ counts, const exp_u64* __restrict__ num_in, unsigned m_h, int vec_ok, exp_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(EXP_THREADS)
void clo_expand_sums_scan_kernel(exp_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(EXP_THREADS)
void clo_expand_ends_kernel(const TC* __restrict__ counts, const exp_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const exp_u64* __restrict__ tsum, exp_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. partition ----
template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(EXP_THREADS)
void clo_expand_partition_kernel(const TC* __restrict__ src, const exp_u64* __restrict__ ends, const exp_u64* __restrict__ num_in, unsigned m_h,
	unsigned tiles, unsigned* __restrict__ first, exp_u64* __restrict__ num_out) {
	const unsigned t = blockIdx.x * EXP_THREADS + threadIdx.x;
	if (t > tiles) return;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	unsigned base[1] = { 0u }, n[1] = { m };
	const exp_u64 x[1] = { (exp_u64) t << EXP_TILE_LOG2 };
	exp_halve<clo_op_ends<TC, OFFSETS>, 1>(e, base, n, x, m_h, m_h - 1u);
	first[t] = base[0];   // <= m
	if (t == 0) *num_out = m > 0u ? e.at(m - 1u) : 0ull;
}

// numel_in 0: there is nothing to read
__global__ void clo_expand_empty_kernel(exp_u64* __restrict__ num_out) { *num_out = 0ull; }

// ---- 3. expand ----

// inclusive max scan of the 64 lanes of a wave: clo_wave_scan_inclusive's network with max, whose identity is 0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned exp_max_step(unsigned x) { return clo_op_max(x, clo_op_dpp<CTRL, ROW_MASK, unsigned>(0u, x)); }
__device__ __forceinline__ unsigned exp_wave_max_scan(unsigned x) {
	x = exp_max_step<0x111, 0xF>(x);   // row_shr:1
	x = exp_max_step<0x112, 0xF>(x);   // row_shr:2
	x = exp_max_step<0x114, 0xF>(x);   // row_shr:4
	x = exp_max_step<0x118, 0xF>(x);   // row_shr:8
	x = exp_max_step<0x142, 0xA>(x);   // row_bcast:15 into rows 1 and 3
	x = exp_max_step<0x143, 0xC>(x);   // row_bcast:31 into rows 2 and 3
	return x;
}

enum { EXP_FLAT = 0, EXP_LDS = 1, EXP_GLOBAL = 2 };

template <typename TC, bool OFFSETS, typename TV>
__global__ __launch_bounds__(EXP_THREADS)
void clo_expand_kernel(const TC* __restrict__ src, const exp_u64* __restrict__ ends, const exp_u64* __restrict__ num_in, unsigned m_h, unsigned capacity,
	const unsigned* __restrict__ first, const TV* __restrict__ vin, TV* __restrict__ vout, unsigned* __restrict__ seg, unsigned* __restrict__ rank) {
	__shared__ __attribute__((aligned(16))) unsigned s_row[EXP_TILE];
	__shared__ unsigned s_wave[EXP_WAVES];
	typedef unsigned vec4 __attribute__((ext_vector_type(4)));
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);
	if (m == 0u) return;
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	const exp_u64 total = e.at(m - 1u), lim = total < capacity ? total : (exp_u64) capacity;
	const exp_u64 row0 = (exp_u64) blockIdx.x << EXP_TILE_LOG2;
	if (row0 >= lim) return;   // the whole work-group
	const unsigned cnt = lim - row0 < EXP_TILE ? (unsigned) (lim - row0) : EXP_TILE;
	const unsigned last = m_h - 1u;
	// the tile's segments: what the partition found, clamped to [0, m] and ordered
	const unsigned f0 = clo_op_min(first[blockIdx.x], m);
	const unsigned f1 = clo_op_min(clo_op_max(first[blockIdx.x + 1u], f0), m);
	const unsigned n = f1 - f0;   // the ends in (row0, row0 + T]: f0 + k < f1 <= m <= m_h for k < n
	const int mode = n == 0u ? EXP_FLAT : n <= EXP_LDS_SEGMENTS ? EXP_LDS : EXP_GLOBAL;

	if (mode == EXP_LDS) {
		#pragma unroll
		for (unsigned i = 0; i < EXP_PER_THREAD / 4u; ++i) reinterpret_cast<vec4*>(s_row)[tid + i * EXP_THREADS] = vec4(0u);
		__syncthreads();
		for (unsigned k = tid; k < n; k += EXP_THREADS) {
			const exp_u64 at = e.at(f0 + k) - row0;   // an end below row0 wraps to above T
			if (at < EXP_TILE) atomicMax(&s_row[(unsigned) at], ((k + 1u) << EXP_TILE_LOG2) | (unsigned) at);
		}
		__syncthreads();
		// the inclusive max scan over the rows: 16 consecutive rows per thread, the lanes, the waves
		unsigned v[EXP_PER_THREAD];
		#pragma unroll
		for (unsigned i = 0; i < EXP_PER_THREAD / 4u; ++i) {
			const vec4 x = reinterpret_cast<const vec4*>(s_row)[tid * (EXP_PER_THREAD / 4u) + i];
			v[4 * i] = x.x; v[4 * i + 1] = x.y; v[4 * i + 2] = x.z; v[4 * i + 3] = x.w;
		}
		#pragma unroll
		for (unsigned i = 1; i < EXP_PER_THREAD; ++i) v[i] = clo_op_max(v[i], v[i - 1]);
		const unsigned incl = exp_wave_max_scan(v[EXP_PER_THREAD - 1]);
		if (lane == 63u) s_wave[wave] = incl;
		unsigned carry = clo_op_shfl<unsigned>(incl, (int) lane - 1);
		if (lane == 0u) carry = 0u;
		__syncthreads();
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) EXP_WAVES; ++w) {
			const unsigned s = s_wave[w];
			if (w < wave) carry = clo_op_max(carry, s);
		}
		#pragma unroll
		for (unsigned i = 0; i < EXP_PER_THREAD / 4u; ++i) {
			vec4 x;
			x.x = clo_op_max(v[4 * i], carry); x.y = clo_op_max(v[4 * i + 1], carry);
			x.z = clo_op_max(v[4 * i + 2], carry); x.w = clo_op_max(v[4 * i + 3], carry);
			reinterpret_cast<vec4*>(s_row)[tid * (EXP_PER_THREAD / 4u) + i] = x;
		}
		__syncthreads();
	} else if (mode == EXP_GLOBAL) {
		// s_row[j] = the segment itself: n does not fit a mark
		#pragma unroll 1
		for (unsigned i = 0; i < EXP_PER_THREAD / EXP_HALVE_ITEMS; ++i) {
			unsigned base[EXP_HALVE_ITEMS], len[EXP_HALVE_ITEMS];
			exp_u64 x[EXP_HALVE_ITEMS];
			#pragma unroll
			for (int k = 0; k < EXP_HALVE_ITEMS; ++k) {
				base[k] = f0; len[k] = n;
				x[k] = row0 + tid + (i * EXP_HALVE_ITEMS + (unsigned) k) * EXP_THREADS;
			}
			exp_halve<clo_op_ends<TC, OFFSETS>, EXP_HALVE_ITEMS>(e, base, len, x, m_h, last);
			#pragma unroll
			for (int k = 0; k < EXP_HALVE_ITEMS; ++k) s_row[tid + (i * EXP_HALVE_ITEMS + (unsigned) k) * EXP_THREADS] = base[k];
		}
		__syncthreads();
	}

	// where segment f0 began: the rows of the tile before its first mark count from there
	const exp_u64 start0 = f0 > 0u ? e.at(clo_op_min(f0 - 1u, last)) : 0ull;
	// every segment id is clamped to numel_in - 1: nothing else is written to seg_out or gathered by
	auto seg_of = [&](unsigned j) -> unsigned {
		const unsigned r = mode == EXP_FLAT ? f0 : mode == EXP_LDS ? f0 + (s_row[j] >> EXP_TILE_LOG2) : s_row[j];
		return clo_op_min(r, last);
	};
	auto rank_of = [&](unsigned j) -> unsigned {
		if (mode == EXP_GLOBAL) {
			const unsigned r = s_row[j];
			const exp_u64 start = r > 0u ? e.at(clo_op_min(r - 1u, last)) : 0ull;
			return (unsigned) (row0 + j - start);
		}
		const unsigned mark = mode == EXP_FLAT ? 0u : s_row[j];
		return (mark >> EXP_TILE_LOG2) == 0u ? (unsigned) (row0 + j - start0) : j - (mark & (EXP_TILE - 1u));
	};
	if (vout) clo_op_store<TV>(vout + row0, cnt, tid, [&](unsigned j) { return vin[seg_of(j)]; });
	if (seg) clo_op_store<unsigned>(seg + row0, cnt, tid, seg_of);
	if (rank) clo_op_store<unsigned>(rank + row0, cnt, tid, rank_of);
}

struct exp_args {
	const void* src; const exp_u64* num_in; const void* vin; void* vout; unsigned* seg; unsigned* rank; exp_u64* num_out;
	unsigned m_h, capacity; exp_u64* ends; unsigned* first; exp_u64* tsum; hipStream_t s;
};

inline unsigned exp_tiles(size_t capacity) { return (unsigned) ((capacity + EXP_TILE - 1) / EXP_TILE); }

constexpr const char* EXP_ENDS_LABELS[3] = { "expand_sums", "expand_sums_scan", "expand_ends" };

template <typename TC, bool OFFSETS, typename TV>
int exp_launch(const exp_args& a) {
	if constexpr (!OFFSETS) {
		const int st = clo_op_ends_launch<TC>(clo_expand_sums_kernel<TC>, clo_expand_sums_scan_kernel, clo_expand_ends_kernel<TC>, EXP_ENDS_LABELS,
			a.src, a.num_in, a.m_h, a.tsum, a.ends, a.s);
		if (st != 0) return st;
	}
	const unsigned tiles = exp_tiles(a.capacity);
	{
		clo_timing_scope timing("expand_partition", a.s);
		hipLaunchKernelGGL((clo_expand_partition_kernel<TC, OFFSETS>), dim3(tiles / EXP_THREADS + 1u), dim3(EXP_THREADS), 0, a.s,
			(const TC*) a.src, (const exp_u64*) a.ends, a.num_in, a.m_h, tiles, a.first, a.num_out);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	if (tiles == 0u) return 0;   // the size query
	clo_timing_scope timing("expand", a.s);
	hipLaunchKernelGGL((clo_expand_kernel<TC, OFFSETS, TV>), dim3(tiles), dim3(EXP_THREADS), 0, a.s,
		(const TC*) a.src, (const exp_u64*) a.ends, a.num_in, a.m_h, a.capacity, (const unsigned*) a.first, (const TV*) a.vin, (TV*) a.vout, a.seg, a.rank);
	return (int) hipGetLastError();
}

template <typename TC, bool OFFSETS>
int exp_dispatch_value(const exp_args& a, int value_size) {
	// without values the kernel of the 1-byte ones, which looks at neither pointer
	return clo_op_by_key_size(value_size ? value_size : 1, [&](auto tv) { return exp_launch<TC, OFFSETS, decltype(tv)>(a); });
}

template <typename TC>
int exp_dispatch(const exp_args& a, int form, int value_size) {
	return form == CLO_HIP_EXPAND_OFFSETS ? exp_dispatch_value<TC, true>(a, value_size) : exp_dispatch_value<TC, false>(a, value_size);
}

inline bool exp_value_size_ok(int vs) { return vs == 0 || clo_op_key_size_ok(vs); }

}  // namespace

extern "C" {

size_t clo_hip_expand_tile(int value_size) { return exp_value_size_ok(value_size) ? EXP_TILE : 0; }
size_t clo_hip_expand_lds_segments(void) { return EXP_LDS_SEGMENTS; }

size_t clo_hip_expand_workspace_bytes(size_t numel_in, size_t capacity) {
	if (numel_in == 0 && capacity == 0) return 0;
	// the ends of the counts form, one word per tile boundary, the sums of the ends' scan
	return clo_op_ws_align(numel_in * sizeof(exp_u64)) + clo_op_ws_align(((size_t) exp_tiles(capacity) + 1) * sizeof(unsigned))
		+ clo_op_ws_align((clo_op_ends_tiles(numel_in) + 1) * sizeof(exp_u64));
}

int clo_hip_expand(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* values_out, void* seg_out, void* rank_out, uint64_t* num_out, size_t numel_in, size_t capacity, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (form != CLO_HIP_EXPAND_COUNTS && form != CLO_HIP_EXPAND_OFFSETS) return CLO_HIP_EARGS;
	if ((count_size != 4 && count_size != 8) || !exp_value_size_ok(value_size)) return CLO_HIP_EUNSUPPORTED;
	if (numel_in > 0xffffffffull || capacity > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_in > 0 || (form == CLO_HIP_EXPAND_OFFSETS && capacity > 0))) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8) || clo_misaligned(num_in, 8)) return CLO_HIP_EARGS;
	if (!values_out && !seg_out && !rank_out) return CLO_HIP_EARGS;
	if ((values_in != nullptr) != (values_out != nullptr)) return CLO_HIP_EARGS;
	if (values_in && value_size == 0) return CLO_HIP_EARGS;
	if (clo_misaligned(counts_or_offsets, (size_t) count_size) || clo_misaligned(seg_out, 4) || clo_misaligned(rank_out, 4)) return CLO_HIP_EARGS;
	if (values_in && (clo_misaligned(values_in, (size_t) value_size) || clo_misaligned(values_out, (size_t) value_size))) return CLO_HIP_EARGS;
	if (numel_in == 0) {
		hipLaunchKernelGGL(clo_expand_empty_kernel, dim3(1), dim3(1), 0, (hipStream_t) stream, (exp_u64*) num_out);
		return (int) hipGetLastError();
	}
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_expand_workspace_bytes(numel_in, capacity)) return CLO_HIP_EWORKSPACE;

	exp_args a;
	a.src = counts_or_offsets; a.num_in = (const exp_u64*) num_in; a.vin = values_in; a.vout = values_out;
	a.seg = (unsigned*) seg_out; a.rank = (unsigned*) rank_out; a.num_out = (exp_u64*) num_out;
	a.m_h = (unsigned) numel_in; a.capacity = (unsigned) capacity; a.s = (hipStream_t) stream;
	char* ws = (char*) workspace;
	a.ends = (exp_u64*) ws;
	ws += clo_op_ws_align(numel_in * sizeof(exp_u64));
	a.first = (unsigned*) ws;
	ws += clo_op_ws_align(((size_t) exp_tiles(capacity) + 1) * sizeof(unsigned));
	a.tsum = (exp_u64*) ws;
	return count_size == 8 ? exp_dispatch<uint64_t>(a, form, values_in ? value_size : 0) : exp_dispatch<uint32_t>(a, form, values_in ? value_size : 0);
}

}  // extern "C"
