// clo_hip_op_device.h — what the kernels of the operations that are not upstream share (clo_hip_rbk, sbk, merge,
// search, setop, select, topk, hist, expand, segreduce, segsort, segscan, bucket and segarg .hip). Each
// piece is here once because its copies were the same text, or differed only by a parameter a copy had fixed; what
// differs on purpose stays in its file. Everything has internal linkage, and every __global__ function stays in its own
// file under its own name. The 64-bit segment ends and the merge path of the operations over segments from counts or
// offsets are in clo_hip_seg_device.h, which includes this header.
#ifndef CLO_HIP_OP_DEVICE_H
#define CLO_HIP_OP_DEVICE_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "clo_hip.h"
#include "clo_hip_internal.h"

namespace {

// The work-group the block-wide helpers below stride by; a file that uses one of them asserts that its own *_THREADS
// is this.
constexpr int CLO_OP_THREADS = 256;
constexpr int CLO_OP_VEC = 4;   // consecutive elements of a lane in the tiles of rows (load4)

// ---- host: sizes, types, alignment ----

inline size_t clo_op_ws_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }
inline bool clo_op_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }
inline bool clo_op_value_size_ok(int vs) { return vs == 0 || vs == 4 || vs == 8; }

// CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7
inline bool clo_op_int_type(int t) { return t >= 4 && t <= 7; }
inline int clo_op_type_size(int t) { return t >= 6 ? 8 : 4; }
inline bool clo_op_type_signed(int t) { return t == 4 || t == 6; }

// what load4's vec_ok asks of the array's start
template <typename T>
inline int clo_op_vec_ok(const void* p) { return !clo_misaligned(p, sizeof(T) * CLO_OP_VEC < 16 ? sizeof(T) * CLO_OP_VEC : 16); }

// f(a key of key_size bytes), key_size one of 1, 2, 4, 8
template <typename F>
inline int clo_op_by_key_size(int key_size, F f) {
	switch (key_size) {
		case 1: return f(uint8_t());
		case 2: return f(uint16_t());
		case 4: return f(uint32_t());
		default: return f(uint64_t());
	}
}

// ---- what travels with the keys (merge, setop, select, topk) ----

enum { CLO_OP_KEYS = 0, CLO_OP_V4 = 1, CLO_OP_V8 = 2, CLO_OP_ARG = 3 };
template <int MODE> struct clo_op_val { typedef uint32_t T; static constexpr int size = MODE == CLO_OP_KEYS ? 0 : 4; };
template <> struct clo_op_val<CLO_OP_V8> { typedef unsigned long long T; static constexpr int size = 8; };
inline int clo_op_mode(int value_size, bool arg) { return value_size == 0 ? CLO_OP_KEYS : arg ? CLO_OP_ARG : value_size == 4 ? CLO_OP_V4 : CLO_OP_V8; }

__device__ __forceinline__ unsigned clo_op_min(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned clo_op_max(unsigned a, unsigned b) { return a > b ? a : b; }

// Four consecutive elements from element index i0 (a multiple of 4) of an array of n: 16-byte (or 4 elements') vector
// loads where the array's start allows them (vec_ok) and all four exist, else one by one; elements past the end read
// as 0.
template <typename T>
__device__ __forceinline__ void clo_op_load4(const T* __restrict__ p, size_t i0, size_t n, bool vec_ok, T (&v)[CLO_OP_VEC]) {
	if (vec_ok && i0 + CLO_OP_VEC <= n) {
		if constexpr (sizeof(T) == 8) {
			typedef T vec2 __attribute__((ext_vector_type(2)));
			const vec2 a = *reinterpret_cast<const vec2*>(p + i0), b = *reinterpret_cast<const vec2*>(p + i0 + 2);
			v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
		} else {
			typedef T vec4 __attribute__((ext_vector_type(4)));
			const vec4 x = *reinterpret_cast<const vec4*>(p + i0);
			v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
		}
	} else {
		#pragma unroll
		for (int c = 0; c < CLO_OP_VEC; ++c) v[c] = i0 + c < n ? p[i0 + c] : (T) 0;
	}
}

// ---- the merge path (merge, setop; stage and min / max: search too) ----

// How many of the first d outputs of merging a[0, na) and b[0, nb) come from a, ties going to a. Whatever the arrays
// hold, the result lies in [max(0, d - nb), min(d, na)] and only a[< na] and b[< nb] are read. XF: the keys are raw
// and go through clo_keyx_fwd first.
template <typename TK, bool XF>
__device__ __forceinline__ unsigned clo_op_path(const TK* a, const TK* b, unsigned na, unsigned nb, unsigned d, const clo_keyx& kx) {
	unsigned lo = d > nb ? d - nb : 0u, hi = clo_op_min(d, na);
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		TK x = a[mid], y = b[d - 1u - mid];
		if constexpr (XF) { x = clo_keyx_fwd<TK>(x, kx); y = clo_keyx_fwd<TK>(y, kx); }
		if (x <= y) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

// The body of a partition kernel: one thread per tile boundary d = t * TILE of the merged sequence writes split[t], how
// many of the first d merged elements come from A (tiles + 1 words).
template <typename TK, size_t TILE>
__device__ __forceinline__ void clo_op_partition(const TK* __restrict__ ka, const TK* __restrict__ kb, unsigned na, unsigned nb, unsigned tiles,
	const clo_keyx& kx, unsigned* __restrict__ split) {
	const unsigned t = blockIdx.x * CLO_OP_THREADS + threadIdx.x;
	if (t > tiles) return;
	const unsigned long long n = (unsigned long long) na + nb, dd = (unsigned long long) t * TILE;
	split[t] = clo_op_path<TK, true>(ka, kb, na, nb, (unsigned) (dd < n ? dd : n), kx);
}

// The tile's outputs [d0, d0 + cnt) of the MERGE and its ranges [a0, a0 + na_t) of A and [b0, b0 + nb_t) of B. The
// searches' results are clamped to what d0, d1, na and nb alone allow: a0 in [d0 - nb, min(d0, na)], a1 - a0 in [0, d1
// - d0], a1 in [d1 - nb, na], so that whatever the searches found on unsorted inputs every read stays inside the inputs
// and the tile has at most TILE elements. (Sorted inputs: the searches are monotone and nothing is changed.)
struct clo_op_range { unsigned d0, cnt, a0, b0, na_t, nb_t; };

template <unsigned TILE>
__device__ __forceinline__ clo_op_range clo_op_tile_range(const unsigned* __restrict__ split, unsigned na, unsigned nb) {
	const unsigned long long n = (unsigned long long) na + nb, dd0 = (unsigned long long) blockIdx.x * TILE;
	const unsigned d0 = (unsigned) (dd0 < n ? dd0 : n), d1 = (unsigned) (dd0 + TILE < n ? dd0 + TILE : n);
	clo_op_range r;
	r.d0 = d0;
	r.cnt = d1 - d0;
	unsigned a0 = split[blockIdx.x], a1 = split[blockIdx.x + 1u];
	a0 = clo_op_min(clo_op_max(a0, d0 > nb ? d0 - nb : 0u), clo_op_min(d0, na));
	a1 = clo_op_min(clo_op_max(a1, clo_op_max(a0, d1 > nb ? d1 - nb : 0u)), clo_op_min(na, a0 + r.cnt));
	r.a0 = a0;
	r.b0 = d0 - a0;
	r.na_t = a1 - a0;
	r.nb_t = r.cnt - r.na_t;
	return r;
}

// src[0, count) into dst[0, count) (LDS), lanes on adjacent 16-byte vectors from src's first 16-byte boundary on.
template <typename T, bool XF>
__device__ __forceinline__ void clo_op_stage(const T* __restrict__ src, unsigned count, T* dst, const clo_keyx& kx, unsigned tid) {
	constexpr unsigned PER = 16u / sizeof(T);
	typedef T vec __attribute__((ext_vector_type(PER)));
	const unsigned head = clo_op_min((unsigned) ((16u - ((uintptr_t) src & 15u)) & 15u) / (unsigned) sizeof(T), count);
	const unsigned nvec = (count - head) / PER, body_end = head + nvec * PER;
	for (unsigned v = tid; v < nvec; v += CLO_OP_THREADS) {
		const unsigned i0 = head + v * PER;
		const vec x = *reinterpret_cast<const vec*>(src + i0);
		#pragma unroll
		for (unsigned c = 0; c < PER; ++c) dst[i0 + c] = XF ? clo_keyx_fwd<T>(x[c], kx) : x[c];
	}
	const unsigned rest = head + (count - body_end);   // fewer than 2 PER <= 32 elements
	if (tid < rest) {
		const unsigned i = tid < head ? tid : body_end + (tid - head);
		dst[i] = XF ? clo_keyx_fwd<T>(src[i], kx) : src[i];
	}
}

// dst[i] = get(i) for i in [0, count), the same division: 16-byte vector stores from dst's first 16-byte boundary on,
// the fewer than two vectors' worth before and after them element by element. (search_store copies from an array
// and is not this one.)
template <typename T, typename F>
__device__ __forceinline__ void clo_op_store(T* __restrict__ dst, unsigned count, unsigned tid, F get) {
	constexpr unsigned PER = 16u / sizeof(T);
	typedef T vec __attribute__((ext_vector_type(PER)));
	const unsigned head = clo_op_min((unsigned) ((16u - ((uintptr_t) dst & 15u)) & 15u) / (unsigned) sizeof(T), count);
	const unsigned nvec = (count - head) / PER, body_end = head + nvec * PER;
	for (unsigned v = tid; v < nvec; v += CLO_OP_THREADS) {
		const unsigned i0 = head + v * PER;
		vec x;
		#pragma unroll
		for (unsigned c = 0; c < PER; ++c) x[c] = get(i0 + c);
		*reinterpret_cast<vec*>(dst + i0) = x;
	}
	const unsigned rest = head + (count - body_end);   // fewer than 2 PER <= 32 elements
	if (tid < rest) {
		const unsigned i = tid < head ? tid : body_end + (tid - head);
		dst[i] = get(i);
	}
}

// ---- the segmented scan of the by-key operations (rbk, sbk) ----

// rows per tile: 256 bytes of keys and values per thread at most (the apply sweeps keep them, and the state of the
// lanes before it for every row, in registers between their two scans)
constexpr int clo_op_seg_rows(int key_size, int value_size) { return key_size + value_size <= 8 ? 8 : 4; }
constexpr size_t CLO_OP_SEG_MIN_TILE = (size_t) CLO_OP_THREADS * CLO_OP_VEC * 4;   // sizes the workspace, whose getter knows no sizes
inline size_t clo_op_seg_max_tiles(size_t numel) { return (numel + CLO_OP_SEG_MIN_TILE - 1) / CLO_OP_SEG_MIN_TILE + 1; }
// the tile states: the heads, and behind them the aggregates in the widest sum type
inline size_t clo_op_seg_workspace_bytes(size_t numel) {
	const size_t t = clo_op_seg_max_tiles(numel);
	return clo_op_ws_align(t * sizeof(unsigned)) + clo_op_ws_align(t * sizeof(unsigned long long));
}

enum { CLO_OP_SUM = 0, CLO_OP_MIN = 1, CLO_OP_MAX = 2 };
// How a value becomes a number of the sum type, `(sum type) x` seen as bits:
enum {
	CLO_OP_CVT_NONE = 0,    // no aggregate wanted (reduce by key without aggr_out): the kernels count heads only
	CLO_OP_CVT_32 = 1,      // 32-bit value, 32-bit sum
	CLO_OP_CVT_S64 = 2,     // int value, 64-bit sum (sign extension)
	CLO_OP_CVT_U64 = 3,     // uint value, 64-bit sum
	CLO_OP_CVT_64 = 4,      // 64-bit value, 64-bit sum
	CLO_OP_CVT_ONE32 = 5,   // values absent: every value is 1, 32-bit sum
	CLO_OP_CVT_ONE64 = 6    // the same, 64-bit sum
};
template <int CVT> struct clo_op_cvt;
template <> struct clo_op_cvt<CLO_OP_CVT_NONE> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 0; };
template <> struct clo_op_cvt<CLO_OP_CVT_32> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 4; };
template <> struct clo_op_cvt<CLO_OP_CVT_S64> { typedef int32_t TV; typedef uint64_t TS; static constexpr int vs = 4; };
template <> struct clo_op_cvt<CLO_OP_CVT_U64> { typedef uint32_t TV; typedef uint64_t TS; static constexpr int vs = 4; };
template <> struct clo_op_cvt<CLO_OP_CVT_64> { typedef uint64_t TV; typedef uint64_t TS; static constexpr int vs = 8; };
template <> struct clo_op_cvt<CLO_OP_CVT_ONE32> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 0; };
template <> struct clo_op_cvt<CLO_OP_CVT_ONE64> { typedef uint32_t TV; typedef uint64_t TS; static constexpr int vs = 0; };

// which conversion the kernels make, or -1: a pair of types this library does not combine
inline int clo_op_cvt_of(bool aggr, bool vals, int value_type, int sum_type) {
	if (!aggr) return CLO_OP_CVT_NONE;
	if (!clo_op_int_type(sum_type)) return -1;
	const int ss = clo_op_type_size(sum_type);
	if (!vals) return ss == 8 ? CLO_OP_CVT_ONE64 : CLO_OP_CVT_ONE32;
	if (!clo_op_int_type(value_type)) return -1;
	const int vs = clo_op_type_size(value_type);
	if (ss < vs) return -1;
	if (ss == 4) return CLO_OP_CVT_32;
	if (vs == 8) return CLO_OP_CVT_64;
	return clo_op_type_signed(value_type) ? CLO_OP_CVT_S64 : CLO_OP_CVT_U64;
}

template <int OP, typename TS>
__device__ __forceinline__ constexpr TS clo_op_seg_identity() { return OP == CLO_OP_MIN ? (TS) ~(TS) 0 : (TS) 0; }
template <int OP, typename TS>
__device__ __forceinline__ TS clo_op_seg_op(TS a, TS b) {
	if constexpr (OP == CLO_OP_SUM) return (TS) (a + b);
	else if constexpr (OP == CLO_OP_MIN) return a < b ? a : b;
	else return a > b ? a : b;
}

// The state of a stretch of elements: the heads in it, and the aggregate from its last head (from its start
// when it has none) to its end. AGG = false: heads only.
template <typename TS>
struct clo_op_seg_state { unsigned h; TS a; };

template <int OP, bool AGG, typename TS>
__device__ __forceinline__ clo_op_seg_state<TS> clo_op_seg_combine(const clo_op_seg_state<TS>& l, const clo_op_seg_state<TS>& r) {
	clo_op_seg_state<TS> o;
	o.h = l.h + r.h;
	if constexpr (AGG) o.a = r.h ? r.a : clo_op_seg_op<OP, TS>(l.a, r.a);
	else o.a = 0;
	return o;
}
template <int OP, typename TS>
__device__ __forceinline__ clo_op_seg_state<TS> clo_op_seg_empty() { clo_op_seg_state<TS> o; o.h = 0; o.a = clo_op_seg_identity<OP, TS>(); return o; }

// One DPP move of a 32- or 64-bit integer; a lane without a source (and every lane of a row the mask leaves out)
// gets `old`.
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ T clo_op_dpp(T old, T x) {
	static_assert(std::is_integral<T>::value && (sizeof(T) == 4 || sizeof(T) == 8), "32- or 64-bit integers");
	if constexpr (sizeof(T) == 4) {
		return (T) (unsigned) __builtin_amdgcn_update_dpp((int) old, (int) x, CTRL, ROW_MASK, 0xF, false);
	} else {
		const unsigned long long o = (unsigned long long) old, v = (unsigned long long) x;
		const unsigned lo = (unsigned) __builtin_amdgcn_update_dpp((int) (unsigned) o, (int) (unsigned) v, CTRL, ROW_MASK, 0xF, false);
		const unsigned hi = (unsigned) __builtin_amdgcn_update_dpp((int) (unsigned) (o >> 32), (int) (unsigned) (v >> 32), CTRL, ROW_MASK, 0xF, false);
		return (T) (((unsigned long long) hi << 32) | lo);
	}
}

template <int OP, bool AGG, int CTRL, int ROW_MASK, typename TS>
__device__ __forceinline__ void clo_op_seg_step(clo_op_seg_state<TS>& s) {
	clo_op_seg_state<TS> l;
	l.h = clo_op_dpp<CTRL, ROW_MASK, unsigned>(0u, s.h);
	if constexpr (AGG) l.a = clo_op_dpp<CTRL, ROW_MASK, TS>(clo_op_seg_identity<OP, TS>(), s.a);
	else l.a = 0;
	s = clo_op_seg_combine<OP, AGG, TS>(l, s);
}

// Inclusive segmented scan of the 64 lane states of a whole wave: the network of clo_wave_scan_inclusive
// (clo_hip_internal.h) with the operator above. Where only heads are counted it IS that scan.
template <int OP, bool AGG, typename TS>
__device__ __forceinline__ clo_op_seg_state<TS> clo_op_seg_wave_scan(clo_op_seg_state<TS> s) {
	if constexpr (!AGG) {
		s.h = clo_wave_scan_inclusive<unsigned>(s.h, 0u);
	} else {
		clo_op_seg_step<OP, AGG, 0x111, 0xF, TS>(s);   // row_shr:1
		clo_op_seg_step<OP, AGG, 0x112, 0xF, TS>(s);   // row_shr:2
		clo_op_seg_step<OP, AGG, 0x114, 0xF, TS>(s);   // row_shr:4
		clo_op_seg_step<OP, AGG, 0x118, 0xF, TS>(s);   // row_shr:8
		clo_op_seg_step<OP, AGG, 0x142, 0xA, TS>(s);   // row_bcast:15 into rows 1 and 3
		clo_op_seg_step<OP, AGG, 0x143, 0xC, TS>(s);   // row_bcast:31 into rows 2 and 3
	}
	return s;
}

template <typename T>
__device__ __forceinline__ T clo_op_shfl(T v, int src_lane) {
	if constexpr (sizeof(T) == 8) {
		const unsigned long long b = (unsigned long long) v;
		const unsigned lo = (unsigned) __shfl((int) (unsigned) b, src_lane, 64);
		const unsigned hi = (unsigned) __shfl((int) (unsigned) (b >> 32), src_lane, 64);
		return (T) (((unsigned long long) hi << 32) | lo);
	} else {
		return (T) (unsigned) __shfl((int) (unsigned) v, src_lane, 64);
	}
}

// the state of the lanes before this one: the inclusive scan moved up one lane
template <int OP, bool AGG, typename TS>
__device__ __forceinline__ clo_op_seg_state<TS> clo_op_seg_wave_exclusive(const clo_op_seg_state<TS>& incl, unsigned lane) {
	clo_op_seg_state<TS> e;
	e.h = clo_op_shfl<unsigned>(incl.h, (int) lane - 1);
	if constexpr (AGG) e.a = clo_op_shfl<TS>(incl.a, (int) lane - 1);
	else e.a = 0;
	return lane == 0 ? clo_op_seg_empty<OP, TS>() : e;
}

template <typename T>
__device__ __forceinline__ T clo_op_readlane(T v, unsigned lane) {   // `lane` is wave-uniform
	if constexpr (sizeof(T) == 8) {
		const unsigned long long b = (unsigned long long) v;
		const unsigned lo = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) b, (int) lane);
		const unsigned hi = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) (b >> 32), (int) lane);
		return (T) (((unsigned long long) hi << 32) | lo);
	} else {
		return (T) (unsigned) __builtin_amdgcn_readlane((int) (unsigned) v, (int) lane);
	}
}

// The pieces of a tile (the wave totals of its rows, in LDS, written before the tile's barrier): every wave scans them
// for itself; piece p's exclusive state comes back for p = row * waves + wave.
template <int OP, bool AGG, typename TS, int PIECES>
__device__ __forceinline__ clo_op_seg_state<TS> clo_op_seg_scan_pieces(const unsigned* s_h, const TS* s_a, unsigned lane, clo_op_seg_state<TS>* total) {
	static_assert(PIECES <= 64, "one piece per lane");
	clo_op_seg_state<TS> p = clo_op_seg_empty<OP, TS>();
	if (lane < (unsigned) PIECES) {
		p.h = s_h[lane];
		if constexpr (AGG) p.a = s_a[lane];
	}
	const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, AGG, TS>(p);
	total->h = clo_op_readlane<unsigned>(incl.h, 63u);
	total->a = AGG ? clo_op_readlane<TS>(incl.a, 63u) : (TS) 0;
	return clo_op_seg_wave_exclusive<OP, AGG, TS>(incl, lane);
}

}  // namespace

#endif
