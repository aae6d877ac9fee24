// clo_hip_hist.hip — histogram (CloHistogram, include/clo_histogram.h; not upstream): counts or sums of values
// per bin, bin = (key - lower) >> shift, the keys read ONCE and nothing sorted.
//
// One launch of a FIXED grid (a few work-groups per CU); a group walks tiles grid-stride, adds into counters of its
// own and, at the end, adds what it counted onto hist_out with device-scope atomic adds. hist_out was zeroed by a
// fill on the same stream (unless the caller accumulates). No group waits for another, integer addition commutes:
// the result does not depend on the schedule. Three forms of the same loop:
//   COPIES  few bins (num_bins * 32 counters fit HIST_LDS_SPREAD bytes): 32 copies of every counter in LDS, copy =
//           lane mod 32, bin-major — the 32 lanes an LDS instruction serves together hit 32 different banks and never
//           one address, whatever the keys (the layout of clo_radixw_tilehist_kernel);
//   PEEL    more bins, up to clo_hip_histogram_lds_bins: 16, 8, .. 1 copies in LDS. With fewer copies than lanes equal
//           bins meet on one address, so the wave first PEELS its leader's bin: the lanes whose bin is the first
//           valid lane's are summed on the DPP network and added once (all-equal keys: one add per wave instead of 64
//           serialised ones; a bin with 90 % of the keys: it is the leader's nine times out of ten);
//   GLOBAL  more bins than LDS holds: the same peel, the adds go straight to hist_out.
// A tile is THREADS x UNITS vectors of PER elements; PER elements of the WIDER of key and value are 16 bytes, lanes
// read adjacent vectors. The keys (and values) of a group's next tile are requested before the current one is
// counted, and those of its first tile before the counters are zeroed (see clo_radixw_tilehist_kernel).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

constexpr int HIST_THREADS = 512;
constexpr int HIST_UNITS = 4;              // vectors per thread and tile: 64 bytes of the wider array in flight per thread, twice with the prefetch
constexpr int HIST_LDS_MAX = 64 * 1024;    // per group: two groups (16 waves) per CU inside the 160 KiB
constexpr int HIST_LDS_SPREAD = 32 * 1024; // the copies are spread over this much: four groups (32 waves) per CU
constexpr int HIST_GROUPS_PER_CU = 4;

enum { HIST_COPIES = 0, HIST_PEEL = 1, HIST_GLOBAL = 2 };
// How a value becomes a number of the sum type, `(sum type) x` seen as bits: the pairs of clo_op_cvt in a table of its
// own, because a 64-bit sum is unsigned long long here (atomicAdd's type), not uint64_t:
enum {
	HIST_CVT_ONE32 = 0,   // values absent: every value is 1, 32-bit sum
	HIST_CVT_ONE64 = 1,   // the same, 64-bit sum
	HIST_CVT_32 = 2,      // 32-bit value, 32-bit sum
	HIST_CVT_S64 = 3,     // int value, 64-bit sum (sign extension)
	HIST_CVT_U64 = 4,     // uint value, 64-bit sum
	HIST_CVT_64 = 5       // 64-bit value, 64-bit sum
};
template <int CVT> struct hist_cvt;
template <> struct hist_cvt<HIST_CVT_ONE32> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 0; };
template <> struct hist_cvt<HIST_CVT_ONE64> { typedef uint32_t TV; typedef unsigned long long TS; static constexpr int vs = 0; };
template <> struct hist_cvt<HIST_CVT_32> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 4; };
template <> struct hist_cvt<HIST_CVT_S64> { typedef int32_t TV; typedef unsigned long long TS; static constexpr int vs = 4; };
template <> struct hist_cvt<HIST_CVT_U64> { typedef uint32_t TV; typedef unsigned long long TS; static constexpr int vs = 4; };
template <> struct hist_cvt<HIST_CVT_64> { typedef unsigned long long TV; typedef unsigned long long TS; static constexpr int vs = 8; };

constexpr int hist_per(int key_size, int value_size) { return 16 / (key_size > value_size ? key_size : value_size); }
constexpr size_t hist_tile(int key_size, int value_size) { return (size_t) HIST_THREADS * HIST_UNITS * hist_per(key_size, value_size); }

// PER consecutive elements from element index i0 (a multiple of PER) of an array of n: one vector load where the
// array's start allows it and all of them exist, else one by one; elements past the end read as 0.
template <typename T, int PER>
__device__ __forceinline__ void hist_load(const T* __restrict__ p, size_t i0, size_t n, bool vec_ok, T (&v)[PER]) {
	if (vec_ok && i0 + PER <= n) {
		typedef T vec __attribute__((ext_vector_type(PER)));
		const vec x = *reinterpret_cast<const vec*>(p + i0);
		#pragma unroll
		for (int c = 0; c < PER; ++c) v[c] = x[c];
	} else {
		#pragma unroll
		for (int c = 0; c < PER; ++c) v[c] = i0 + c < n ? p[i0 + c] : (T) 0;
	}
}

template <typename TS>
__device__ __forceinline__ void hist_global_add(TS* p, TS x) {
	(void) __hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One element per lane, the whole wave here together (`valid` says which lanes have one): x is added to cnt[idx],
// where idx is the slot of bin `bin` this lane uses (its copy).
// PEEL: the lanes whose BIN is that of the first valid lane are summed and added by that lane alone, at its own slot.
template <bool PEEL, bool GLOBAL, bool ONES, typename TS>
__device__ __forceinline__ void hist_wave_add(TS* cnt, unsigned bin, unsigned idx, bool valid, TS x, unsigned lane) {
	bool add = valid;
	if constexpr (PEEL) {
		const unsigned long long act = __ballot(valid);
		if (act != 0ull) {   // (wave-uniform)
			const unsigned lead = (unsigned) __ffsll(act) - 1u;
			const unsigned b0 = (unsigned) __builtin_amdgcn_readlane((int) bin, (int) lead);
			const bool m = valid && bin == b0;
			TS total;
			if constexpr (ONES) total = (TS) __popcll(__ballot(m));
			else total = clo_wave_reduce_sum<TS>(m ? x : (TS) 0);
			if (m) { add = lane == lead; x = total; }
		}
	}
	if (add) {
		if constexpr (GLOBAL) hist_global_add<TS>(cnt + idx, x);
		else atomicAdd(cnt + idx, x);
	}
}

template <typename TK, int CVT, int MODE>
__global__ __launch_bounds__(HIST_THREADS)
void clo_hist_kernel(const TK* __restrict__ keys, const typename hist_cvt<CVT>::TV* __restrict__ values, size_t n, unsigned tiles,
	typename hist_cvt<CVT>::TS* __restrict__ hist_out, TK lower, TK flip, unsigned shift, unsigned num_bins, unsigned clog, int kvec, int vvec) {
	typedef typename hist_cvt<CVT>::TV TV;
	typedef typename hist_cvt<CVT>::TS TS;
	constexpr bool VALS = hist_cvt<CVT>::vs != 0;
	constexpr bool GLOBAL = MODE == HIST_GLOBAL;
	constexpr int PER = hist_per((int) sizeof(TK), hist_cvt<CVT>::vs);
	constexpr size_t TILE = hist_tile((int) sizeof(TK), hist_cvt<CVT>::vs);
	extern __shared__ __attribute__((aligned(16))) unsigned char hist_lds[];
	TS* const s_cnt = reinterpret_cast<TS*>(hist_lds);
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	if constexpr (MODE == HIST_COPIES) clog = 5u;
	const unsigned copy = GLOBAL ? 0u : (lane & ((1u << clog) - 1u));
	const TK lo = (TK) (lower ^ flip);   // signed keys: both operands with the sign bit flipped compare as unsigned numbers

	TK k[HIST_UNITS][PER];
	TV v[HIST_UNITS][PER];
	unsigned tile = blockIdx.x;
	const auto load = [&](unsigned t, TK (&kk)[HIST_UNITS][PER], TV (&vv)[HIST_UNITS][PER]) {
		#pragma unroll
		for (int u = 0; u < HIST_UNITS; ++u) {
			const size_t i0 = (size_t) t * TILE + ((size_t) u * HIST_THREADS + tid) * PER;
			hist_load<TK, PER>(keys, i0, n, kvec != 0, kk[u]);
			if constexpr (VALS) hist_load<TV, PER>(values, i0, n, vvec != 0, vv[u]);
		}
	};
	// requested FIRST: the counters are zeroed and the barrier passed while the first tile is on its way
	if (tile < tiles) load(tile, k, v);
	if constexpr (!GLOBAL) {
		const unsigned words = num_bins << clog;
		for (unsigned i = tid; i < words; i += HIST_THREADS) s_cnt[i] = (TS) 0;
		clo_lds_barrier();
	}
	while (tile < tiles) {   // (the same for the whole group)
		const unsigned next = tile + gridDim.x;
		TK kn[HIST_UNITS][PER];
		TV vn[HIST_UNITS][PER];
		if (next < tiles) load(next, kn, vn);
		#pragma unroll
		for (int u = 0; u < HIST_UNITS; ++u) {
			const size_t i0 = (size_t) tile * TILE + ((size_t) u * HIST_THREADS + tid) * PER;
			#pragma unroll
			for (int c = 0; c < PER; ++c) {
				const TK x = (TK) (k[u][c] ^ flip);
				// key >= lower, explicitly: where lower + (num_bins << shift) runs past the type's maximum, the wrapped
				// difference of a key below lower would land inside the range
				bool valid = i0 + c < n && x >= lo;
				const TK b = (TK) ((TK) (x - lo) >> shift);
				valid = valid && (unsigned long long) b < (unsigned long long) num_bins;
				TS a = (TS) 1;
				if constexpr (VALS) a = (TS) v[u][c];
				const unsigned idx = GLOBAL ? (unsigned) b : (((unsigned) b << clog) + copy);
				hist_wave_add<MODE != HIST_COPIES, GLOBAL, !VALS, TS>(GLOBAL ? hist_out : s_cnt, (unsigned) b, idx, valid, a, lane);
			}
		}
		if (next < tiles) {
			#pragma unroll
			for (int u = 0; u < HIST_UNITS; ++u) {
				#pragma unroll
				for (int c = 0; c < PER; ++c) { k[u][c] = kn[u][c]; if constexpr (VALS) v[u][c] = vn[u][c]; }
			}
		}
		tile = next;
	}
	if constexpr (!GLOBAL) {
		// the flush: a bin's copies summed (rotated by the bin: the lanes' rows start a whole number of banks apart),
		// what is not zero ADDED onto hist_out — other groups add to the same words
		__syncthreads();
		const unsigned cm = (1u << clog) - 1u;
		for (unsigned b = tid; b < num_bins; b += HIST_THREADS) {
			TS h = (TS) 0;
			for (unsigned c = 0; c <= cm; ++c) h += s_cnt[(b << clog) + ((c + b) & cm)];
			if (h != (TS) 0) hist_global_add<TS>(hist_out + b, h);
		}
	}
}

struct hist_args {
	const void* keys; const void* values; void* out; size_t n; unsigned long long lower, flip;
	unsigned shift, num_bins, max_groups; hipStream_t s;
};

inline int hist_cus() {   // of the current device, as the stream is taken to be
	int dev = 0, c = 0;
	if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) return 256;
	return c;
}

// The counter copies of a launch: 32 where they fit HIST_LDS_SPREAD, else the largest power of two that does (at least
// 1, inside HIST_LDS_MAX); -1: more bins than LDS holds.
inline int hist_copies_log2(size_t num_bins, size_t sum_size) {
	if (num_bins * sum_size > (size_t) HIST_LDS_MAX) return -1;
	int clog = 5;
	while (clog > 0 && ((num_bins * sum_size) << clog) > (size_t) HIST_LDS_SPREAD) --clog;
	return clog;
}

template <typename TK, int CVT>
int hist_launch(const hist_args& a) {
	typedef typename hist_cvt<CVT>::TV TV;
	typedef typename hist_cvt<CVT>::TS TS;
	constexpr int PER = hist_per((int) sizeof(TK), hist_cvt<CVT>::vs);
	const size_t tile = hist_tile((int) sizeof(TK), hist_cvt<CVT>::vs);
	const unsigned tiles = (unsigned) ((a.n + tile - 1) / tile);
	const int clog = hist_copies_log2(a.num_bins, sizeof(TS));
	const size_t lds = clog < 0 ? 0 : (((size_t) a.num_bins * sizeof(TS)) << clog);
	size_t per_cu = HIST_GROUPS_PER_CU;
	if (lds > (size_t) HIST_LDS_SPREAD) per_cu = 2;
	size_t groups = (size_t) hist_cus() * per_cu;
	if (groups > tiles) groups = tiles;
	if (a.max_groups != 0 && groups > a.max_groups) groups = a.max_groups;
	const int kvec = (uintptr_t) a.keys % (PER * sizeof(TK)) == 0;
	const int vvec = (uintptr_t) a.values % (PER * sizeof(TV)) == 0;
	clo_timing_scope timing("histogram", a.s);
	#define CLO_HIST_GO(MODE) hipLaunchKernelGGL((clo_hist_kernel<TK, CVT, MODE>), dim3((unsigned) groups), dim3(HIST_THREADS), lds, a.s, \
		(const TK*) a.keys, (const TV*) a.values, a.n, tiles, (TS*) a.out, (TK) a.lower, (TK) a.flip, a.shift, a.num_bins, \
		(unsigned) (clog < 0 ? 0 : clog), kvec, vvec)
	if (clog < 0) CLO_HIST_GO(HIST_GLOBAL);
	else if (clog == 5) CLO_HIST_GO(HIST_COPIES);
	else CLO_HIST_GO(HIST_PEEL);
	#undef CLO_HIST_GO
	return (int) hipGetLastError();
}

template <typename TK>
int hist_dispatch(const hist_args& a, int cvt) {
	switch (cvt) {
		case HIST_CVT_ONE32: return hist_launch<TK, HIST_CVT_ONE32>(a);
		case HIST_CVT_ONE64: return hist_launch<TK, HIST_CVT_ONE64>(a);
		case HIST_CVT_32: return hist_launch<TK, HIST_CVT_32>(a);
		case HIST_CVT_S64: return hist_launch<TK, HIST_CVT_S64>(a);
		case HIST_CVT_U64: return hist_launch<TK, HIST_CVT_U64>(a);
		case HIST_CVT_64: return hist_launch<TK, HIST_CVT_64>(a);
		default: return CLO_HIP_EUNSUPPORTED;
	}
}

// which conversion the kernels make, or -1: a pair of types this library does not sum
int hist_cvt_of(bool vals, int value_type, int sum_type) {
	if (!clo_op_int_type(sum_type)) return -1;
	const int ss = clo_op_type_size(sum_type);
	if (!vals) return ss == 8 ? HIST_CVT_ONE64 : HIST_CVT_ONE32;
	if (!clo_op_int_type(value_type)) return -1;
	const int vs = clo_op_type_size(value_type);
	if (ss < vs) return -1;
	if (ss == 4) return HIST_CVT_32;
	if (vs == 8) return HIST_CVT_64;
	return clo_op_type_signed(value_type) ? HIST_CVT_S64 : HIST_CVT_U64;
}

}  // namespace

extern "C" {

size_t clo_hip_histogram_tile(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return hist_tile(key_size, value_size);
}

size_t clo_hip_histogram_lds_bins(int sum_size) {
	if (sum_size != 4 && sum_size != 8) return 0;
	return (size_t) HIST_LDS_MAX / (size_t) sum_size;
}

size_t clo_hip_histogram_workspace_bytes(size_t numel, size_t num_bins) {
	(void) numel; (void) num_bins;
	return 0;   // every counter lives in LDS or in hist_out itself
}

int clo_hip_histogram(const void* keys_in, const void* values_in, void* hist_out, size_t numel, int key_size, int key_signed,
	int value_type, int sum_type, uint64_t lower, unsigned shift, size_t num_bins, int accumulate, unsigned max_groups,
	void* workspace, size_t workspace_bytes, void* stream) {
	hipStream_t s = (hipStream_t) stream;
	(void) workspace; (void) workspace_bytes;
	if (!hist_out || num_bins == 0 || num_bins > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size)) return CLO_HIP_EUNSUPPORTED;
	if (shift >= 8u * (unsigned) key_size) return CLO_HIP_EARGS;
	const int cvt = hist_cvt_of(values_in != nullptr, value_type, sum_type);
	if (cvt < 0) return CLO_HIP_EUNSUPPORTED;
	const size_t ss = (size_t) clo_op_type_size(sum_type);
	if (clo_misaligned(hist_out, ss)) return CLO_HIP_EARGS;
	if (numel > 0 && !keys_in) return CLO_HIP_EARGS;
	if (clo_misaligned(keys_in, (size_t) key_size) || (values_in && clo_misaligned(values_in, (size_t) clo_op_type_size(value_type)))) return CLO_HIP_EARGS;
	if (!accumulate) {
		const hipError_t e = hipMemsetAsync(hist_out, 0, num_bins * ss, s);
		if (e != hipSuccess) return (int) e;
	}
	if (numel == 0) return 0;

	hist_args a;
	a.keys = keys_in; a.values = values_in; a.out = hist_out; a.n = numel; a.shift = shift; a.num_bins = (unsigned) num_bins;
	a.max_groups = max_groups; a.s = s;
	a.flip = key_signed ? 1ull << (8 * key_size - 1) : 0ull;
	a.lower = lower;   // (the low key_size bytes: the value's two's complement for signed keys)
	return clo_op_by_key_size(key_size, [&](auto tk) { return hist_dispatch<decltype(tk)>(a, cvt); });
}

}  // extern "C"
