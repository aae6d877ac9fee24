// clo_hip_rbk.hip — reduce by key (CloReduceByKey, include/clo_reduce.h; not upstream): every run of
// consecutive elements whose keys have the same bytes becomes one row (the run's key, and the sum / min /
// max of its values in an integer sum type, or its length when there are no values).
//
// Three launches, and no work-group ever waits for another:
//   1. tile sweep   a group reads one tile and writes its STATE: (heads, tail) — the number of run heads in
//                   the tile, and the aggregate of the values from the tile's last head to its end (of the
//                   whole tile when it has no head);
//   2. state scan   one group walks the tile states with the segmented-scan operator
//                       (hL, aL) o (hR, aR) = (hL + hR, hR ? aR : aL op aR)
//                   and leaves, per tile, the state of everything before it: the heads before the tile and
//                   the carry into it (the open run's aggregate so far); it writes the number of runs;
//   3. apply sweep  a group reads its tile again, runs the same segmented scan over it starting from the
//                   tile's incoming state, and every element that ENDS a run (the last one, or one whose
//                   right neighbour has another key) stores row number heads-up-to-here - 1.
// A tile is 256 threads x 4 consecutive elements x ROWS rows (the scan kernel's shape, clo_hip_scan.hip):
// a lane's four elements come in one vector load, a row is one coalesced stretch of 1024 elements. Inside
// a tile the order is row, wave, lane, element: a wave scans the 64 lane states of a row on the DPP network
// (integer-only and on whole waves, as the clo_wave_scan_inclusive family), the ROWS x 4 wave totals of a
// tile are the PIECES every wave scans again for itself after the tile's one barrier.
// min / max are computed on unsigned numbers: a signed sum type has its sign bit flipped on load and on
// store (`flip`), which keeps the order. The sum type only matters by its width otherwise.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "clo_hip.h"
#include "clo_hip_internal.h"

namespace {

constexpr int RBK_THREADS = 256;
constexpr int RBK_WAVES = RBK_THREADS / 64;
constexpr int RBK_VEC = 4;
constexpr int RBK_ROW_ELEMS = RBK_THREADS * RBK_VEC;   // 1024

// rows per tile: 256 bytes of keys and values per thread at most (the apply sweep keeps them, and the state of the
// lanes before it for every row, in registers between its two scans)
constexpr int rbk_rows(int key_size, int value_size) { return key_size + value_size <= 8 ? 8 : 4; }

enum { RBK_SUM = 0, RBK_MIN = 1, RBK_MAX = 2 };
// How a value becomes a number of the sum type, `(sum type) x` seen as bits:
enum {
	RBK_CVT_NONE = 0,    // no aggregate wanted (aggr_out absent): the kernels count heads only
	RBK_CVT_32 = 1,      // 32-bit value, 32-bit sum
	RBK_CVT_S64 = 2,     // int value, 64-bit sum (sign extension)
	RBK_CVT_U64 = 3,     // uint value, 64-bit sum
	RBK_CVT_64 = 4,      // 64-bit value, 64-bit sum
	RBK_CVT_ONE32 = 5,   // values absent: every value is 1, 32-bit sum
	RBK_CVT_ONE64 = 6    // the same, 64-bit sum
};
template <int CVT> struct rbk_cvt;
template <> struct rbk_cvt<RBK_CVT_NONE> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 0; };
template <> struct rbk_cvt<RBK_CVT_32> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 4; };
template <> struct rbk_cvt<RBK_CVT_S64> { typedef int32_t TV; typedef uint64_t TS; static constexpr int vs = 4; };
template <> struct rbk_cvt<RBK_CVT_U64> { typedef uint32_t TV; typedef uint64_t TS; static constexpr int vs = 4; };
template <> struct rbk_cvt<RBK_CVT_64> { typedef uint64_t TV; typedef uint64_t TS; static constexpr int vs = 8; };
template <> struct rbk_cvt<RBK_CVT_ONE32> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 0; };
template <> struct rbk_cvt<RBK_CVT_ONE64> { typedef uint32_t TV; typedef uint64_t TS; static constexpr int vs = 0; };

template <int OP, typename TS>
__device__ __forceinline__ constexpr TS rbk_identity() { return OP == RBK_MIN ? (TS) ~(TS) 0 : (TS) 0; }
template <int OP, typename TS>
__device__ __forceinline__ TS rbk_op(TS a, TS b) {
	if constexpr (OP == RBK_SUM) return (TS) (a + b);
	else if constexpr (OP == RBK_MIN) return a < b ? a : b;
	else return a > b ? a : b;
}

// The state of a stretch of elements: the heads in it, and the aggregate from its last head (from its start
// when it has none) to its end. AGG = false: heads only.
template <typename TS>
struct rbk_state { unsigned h; TS a; };

template <int OP, bool AGG, typename TS>
__device__ __forceinline__ rbk_state<TS> rbk_combine(const rbk_state<TS>& l, const rbk_state<TS>& r) {
	rbk_state<TS> o;
	o.h = l.h + r.h;
	if constexpr (AGG) o.a = r.h ? r.a : rbk_op<OP, TS>(l.a, r.a);
	else o.a = 0;
	return o;
}
template <int OP, typename TS>
__device__ __forceinline__ rbk_state<TS> rbk_empty() { rbk_state<TS> o; o.h = 0; o.a = rbk_identity<OP, TS>(); return o; }

// One DPP move of a 32- or 64-bit integer; a lane without a source (and every lane of a row the mask leaves out)
// gets `old`.
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ T rbk_dpp(T old, T x) {
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
__device__ __forceinline__ void rbk_seg_step(rbk_state<TS>& s) {
	rbk_state<TS> l;
	l.h = rbk_dpp<CTRL, ROW_MASK, unsigned>(0u, s.h);
	if constexpr (AGG) l.a = rbk_dpp<CTRL, ROW_MASK, TS>(rbk_identity<OP, TS>(), s.a);
	else l.a = 0;
	s = rbk_combine<OP, AGG, TS>(l, s);
}

// Inclusive segmented scan of the 64 lane states of a whole wave: the network of clo_wave_scan_inclusive
// (clo_hip_internal.h) with the operator above. Where only heads are counted it IS that scan.
template <int OP, bool AGG, typename TS>
__device__ __forceinline__ rbk_state<TS> rbk_wave_scan(rbk_state<TS> s) {
	if constexpr (!AGG) {
		s.h = clo_wave_scan_inclusive<unsigned>(s.h, 0u);
	} else {
		rbk_seg_step<OP, AGG, 0x111, 0xF, TS>(s);   // row_shr:1
		rbk_seg_step<OP, AGG, 0x112, 0xF, TS>(s);   // row_shr:2
		rbk_seg_step<OP, AGG, 0x114, 0xF, TS>(s);   // row_shr:4
		rbk_seg_step<OP, AGG, 0x118, 0xF, TS>(s);   // row_shr:8
		rbk_seg_step<OP, AGG, 0x142, 0xA, TS>(s);   // row_bcast:15 into rows 1 and 3
		rbk_seg_step<OP, AGG, 0x143, 0xC, TS>(s);   // row_bcast:31 into rows 2 and 3
	}
	return s;
}

template <typename T>
__device__ __forceinline__ T rbk_shfl(T v, int src_lane) {
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
__device__ __forceinline__ rbk_state<TS> rbk_wave_exclusive(const rbk_state<TS>& incl, unsigned lane) {
	rbk_state<TS> e;
	e.h = rbk_shfl<unsigned>(incl.h, (int) lane - 1);
	if constexpr (AGG) e.a = rbk_shfl<TS>(incl.a, (int) lane - 1);
	else e.a = 0;
	return lane == 0 ? rbk_empty<OP, TS>() : e;
}

template <typename T>
__device__ __forceinline__ T rbk_readlane(T v, unsigned lane) {   // `lane` is wave-uniform
	if constexpr (sizeof(T) == 8) {
		const unsigned long long b = (unsigned long long) v;
		const unsigned lo = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) b, (int) lane);
		const unsigned hi = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) (b >> 32), (int) lane);
		return (T) (((unsigned long long) hi << 32) | lo);
	} else {
		return (T) (unsigned) __builtin_amdgcn_readlane((int) (unsigned) v, (int) lane);
	}
}

// Four consecutive elements from element index i0 (a multiple of 4) of an array of n: one vector load where the
// array's start allows it and all four exist, else one by one; elements past the end read as 0.
template <typename T>
__device__ __forceinline__ void rbk_load4(const T* __restrict__ p, size_t i0, size_t n, bool vec_ok, T (&v)[RBK_VEC]) {
	if (vec_ok && i0 + RBK_VEC <= n) {
		typedef T vec4 __attribute__((ext_vector_type(4)));
		const vec4 x = *reinterpret_cast<const vec4*>(p + i0);
		v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
	} else {
		#pragma unroll
		for (int c = 0; c < RBK_VEC; ++c) v[c] = i0 + c < n ? p[i0 + c] : (T) 0;
	}
}

// What both sweeps know about one row of a lane: bit c of `heads` = element c starts a run, bit 4 = the element
// after the lane's four does (or is the end of the array); the lane's state; the values as numbers of the sum type.
template <typename TK, int CVT, int OP>
struct rbk_row {
	typedef typename rbk_cvt<CVT>::TV TV;
	typedef typename rbk_cvt<CVT>::TS TS;
	static constexpr bool AGG = CVT != RBK_CVT_NONE;
	static constexpr bool VALS = rbk_cvt<CVT>::vs != 0;

	// NEXT: also find out whether the element after the lane's four starts a run (the apply sweep's run ends)
	template <bool NEXT>
	static __device__ __forceinline__ unsigned heads(const TK* __restrict__ keys, const TK (&k)[RBK_VEC], size_t i0, size_t n, unsigned lane) {
		// the key before the lane's first: the lane below has it, lane 0 reads it (the tile's first element: across the tile edge)
		TK prev = rbk_shfl<TK>(k[RBK_VEC - 1], (int) lane - 1);
		if (lane == 0 && i0 > 0 && i0 < n) prev = keys[i0 - 1];
		unsigned hb = 0;
		if (i0 < n && (i0 == 0 || k[0] != prev)) hb |= 1u;
		#pragma unroll
		for (int c = 1; c < RBK_VEC; ++c) if (i0 + c < n && k[c] != k[c - 1]) hb |= 1u << c;
		if constexpr (NEXT) {
			unsigned nh = (unsigned) __shfl((int) (hb & 1u), (int) lane + 1, 64);
			if (lane == 63) nh = i0 + RBK_VEC < n ? (unsigned) (keys[i0 + RBK_VEC] != k[RBK_VEC - 1]) : 0u;
			hb |= nh << RBK_VEC;
			// the end of the array counts as a head, so that the last element ends its run (whatever lies past the
			// end comes after every real element in the tile's order: it changes nothing that is stored)
			if (i0 < n && n - i0 <= (size_t) RBK_VEC) hb |= 1u << (unsigned) (n - i0);
		}
		return hb;
	}

	static __device__ __forceinline__ TS value(const TV (&v)[RBK_VEC], int c, TS flip) {
		if constexpr (!VALS) return (TS) 1;
		else if constexpr (OP == RBK_SUM) return (TS) v[c];
		else return (TS) ((TS) v[c] ^ flip);
	}

	// `s` continued over the lane's four elements of one row
	static __device__ __forceinline__ void advance(rbk_state<TS>& s, unsigned hb, const TV (&v)[RBK_VEC], int c, TS flip) {
		if constexpr (AGG) {
			const TS x = value(v, c, flip);
			s.a = ((hb >> c) & 1u) ? x : rbk_op<OP, TS>(s.a, x);
		}
		s.h += (hb >> c) & 1u;
	}
};

// The pieces of a tile (ROWS x RBK_WAVES wave totals, in LDS, written before the tile's barrier): every wave scans
// them for itself; piece p's exclusive state, continued from `start`, comes back for p = row * RBK_WAVES + wave.
template <int OP, bool AGG, typename TS, int PIECES>
__device__ __forceinline__ rbk_state<TS> rbk_scan_pieces(const unsigned* s_h, const TS* s_a, unsigned lane, rbk_state<TS>* total) {
	static_assert(PIECES <= 64, "one piece per lane");
	rbk_state<TS> p = rbk_empty<OP, TS>();
	if (lane < (unsigned) PIECES) {
		p.h = s_h[lane];
		if constexpr (AGG) p.a = s_a[lane];
	}
	const rbk_state<TS> incl = rbk_wave_scan<OP, AGG, TS>(p);
	total->h = rbk_readlane<unsigned>(incl.h, 63u);
	total->a = AGG ? rbk_readlane<TS>(incl.a, 63u) : (TS) 0;
	return rbk_wave_exclusive<OP, AGG, TS>(incl, lane);
}

// ---- 1. tile sweep ----
template <typename TK, int CVT, int OP, int ROWS>
__global__ __launch_bounds__(RBK_THREADS)
void clo_rbk_sweep_kernel(const TK* __restrict__ keys, const typename rbk_cvt<CVT>::TV* __restrict__ values, size_t n,
	unsigned* __restrict__ tile_h, typename rbk_cvt<CVT>::TS* __restrict__ tile_a, typename rbk_cvt<CVT>::TS flip, int kvec, int vvec) {
	typedef rbk_row<TK, CVT, OP> R;
	typedef typename R::TV TV;
	typedef typename R::TS TS;
	constexpr bool AGG = R::AGG;
	constexpr int PIECES = ROWS * RBK_WAVES;
	__shared__ unsigned s_h[PIECES];
	__shared__ TS s_a[PIECES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const size_t base = (size_t) blockIdx.x * (size_t) (ROWS * RBK_ROW_ELEMS) + (size_t) tid * RBK_VEC;

	TK k[ROWS][RBK_VEC];
	TV v[ROWS][RBK_VEC];
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		rbk_load4<TK>(keys, base + (size_t) r * RBK_ROW_ELEMS, n, kvec != 0, k[r]);
		if constexpr (R::VALS) rbk_load4<TV>(values, base + (size_t) r * RBK_ROW_ELEMS, n, vvec != 0, v[r]);
	}
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const size_t i0 = base + (size_t) r * RBK_ROW_ELEMS;
		const unsigned hb = R::template heads<false>(keys, k[r], i0, n, lane);
		rbk_state<TS> s = rbk_empty<OP, TS>();
		#pragma unroll
		for (int c = 0; c < RBK_VEC; ++c) R::advance(s, hb, v[r], c, flip);
		s = rbk_wave_scan<OP, AGG, TS>(s);
		if (lane == 63) {
			s_h[r * RBK_WAVES + wave] = s.h;
			if constexpr (AGG) s_a[r * RBK_WAVES + wave] = s.a;
		}
	}
	__syncthreads();
	if (wave == 0) {
		rbk_state<TS> total;
		(void) rbk_scan_pieces<OP, AGG, TS, PIECES>(s_h, s_a, lane, &total);
		if (lane == 0) {
			tile_h[blockIdx.x] = total.h;
			if constexpr (AGG) tile_a[blockIdx.x] = total.a;
		}
	}
}

// ---- 2. state scan: one group; tile t gets the state of the tiles before it, in place ----
template <int CVT, int OP>
__global__ __launch_bounds__(RBK_THREADS)
void clo_rbk_states_kernel(unsigned* __restrict__ tile_h, typename rbk_cvt<CVT>::TS* __restrict__ tile_a, unsigned tiles,
	unsigned long long* __restrict__ num_runs) {
	typedef typename rbk_cvt<CVT>::TS TS;
	constexpr bool AGG = CVT != RBK_CVT_NONE;
	constexpr int PER = 4;   // consecutive states per thread
	__shared__ unsigned s_h[RBK_WAVES];
	__shared__ TS s_a[RBK_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	rbk_state<TS> running = rbk_empty<OP, TS>();   // the state of everything before this chunk (the same in every thread)
	for (unsigned chunk = 0; chunk < tiles; chunk += RBK_THREADS * PER) {
		const unsigned t0 = chunk + tid * PER;
		rbk_state<TS> st[PER];
		rbk_state<TS> mine = rbk_empty<OP, TS>();
		#pragma unroll
		for (int j = 0; j < PER; ++j) {
			st[j] = rbk_empty<OP, TS>();
			if (t0 + j < tiles) {
				st[j].h = tile_h[t0 + j];
				if constexpr (AGG) st[j].a = tile_a[t0 + j];
			}
			mine = rbk_combine<OP, AGG, TS>(mine, st[j]);
		}
		const rbk_state<TS> incl = rbk_wave_scan<OP, AGG, TS>(mine);
		if (lane == 63) {
			s_h[wave] = incl.h;
			if constexpr (AGG) s_a[wave] = incl.a;
		}
		__syncthreads();
		rbk_state<TS> before = running, all = running;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) RBK_WAVES; ++w) {
			rbk_state<TS> p;
			p.h = s_h[w];
			p.a = AGG ? s_a[w] : (TS) 0;
			if (w < wave) before = rbk_combine<OP, AGG, TS>(before, p);
			all = rbk_combine<OP, AGG, TS>(all, p);
		}
		rbk_state<TS> s = rbk_combine<OP, AGG, TS>(before, rbk_wave_exclusive<OP, AGG, TS>(incl, lane));
		#pragma unroll
		for (int j = 0; j < PER; ++j) {
			if (t0 + j < tiles) {
				tile_h[t0 + j] = s.h;
				if constexpr (AGG) tile_a[t0 + j] = s.a;
			}
			s = rbk_combine<OP, AGG, TS>(s, st[j]);
		}
		running = all;
		__syncthreads();   // s_h / s_a are written again in the next chunk
	}
	if (tid == 0) *num_runs = (unsigned long long) running.h;
}

// ---- 3. apply sweep ----
template <typename TK, int CVT, int OP, int ROWS>
__global__ __launch_bounds__(RBK_THREADS)
void clo_rbk_apply_kernel(const TK* __restrict__ keys, const typename rbk_cvt<CVT>::TV* __restrict__ values, size_t n,
	const unsigned* __restrict__ tile_h, const typename rbk_cvt<CVT>::TS* __restrict__ tile_a, typename rbk_cvt<CVT>::TS flip, int kvec, int vvec,
	TK* __restrict__ keys_out, typename rbk_cvt<CVT>::TS* __restrict__ aggr_out) {
	typedef rbk_row<TK, CVT, OP> R;
	typedef typename R::TV TV;
	typedef typename R::TS TS;
	constexpr bool AGG = R::AGG;
	constexpr int PIECES = ROWS * RBK_WAVES;
	__shared__ unsigned s_h[PIECES];
	__shared__ TS s_a[PIECES];
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	const unsigned wave = (unsigned) __builtin_amdgcn_readfirstlane((int) (tid >> 6));
	const size_t base = (size_t) blockIdx.x * (size_t) (ROWS * RBK_ROW_ELEMS) + (size_t) tid * RBK_VEC;

	TK k[ROWS][RBK_VEC];
	TV v[ROWS][RBK_VEC];
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		rbk_load4<TK>(keys, base + (size_t) r * RBK_ROW_ELEMS, n, kvec != 0, k[r]);
		if constexpr (R::VALS) rbk_load4<TV>(values, base + (size_t) r * RBK_ROW_ELEMS, n, vvec != 0, v[r]);
	}
	// the state of everything before the tile: heads before it, and the carry into it
	rbk_state<TS> tile_in;
	tile_in.h = tile_h[blockIdx.x];
	tile_in.a = AGG ? tile_a[blockIdx.x] : (TS) 0;

	unsigned hb[ROWS];
	rbk_state<TS> ex[ROWS];   // the lanes of this wave before this one, per row
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const size_t i0 = base + (size_t) r * RBK_ROW_ELEMS;
		hb[r] = R::template heads<true>(keys, k[r], i0, n, lane);
		rbk_state<TS> s = rbk_empty<OP, TS>();
		#pragma unroll
		for (int c = 0; c < RBK_VEC; ++c) R::advance(s, hb[r], v[r], c, flip);
		s = rbk_wave_scan<OP, AGG, TS>(s);
		if (lane == 63) {
			s_h[r * RBK_WAVES + wave] = s.h;
			if constexpr (AGG) s_a[r * RBK_WAVES + wave] = s.a;
		}
		ex[r] = rbk_wave_exclusive<OP, AGG, TS>(s, lane);
	}
	__syncthreads();
	rbk_state<TS> total;
	const rbk_state<TS> pieces = rbk_scan_pieces<OP, AGG, TS, PIECES>(s_h, s_a, lane, &total);
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const size_t i0 = base + (size_t) r * RBK_ROW_ELEMS;
		rbk_state<TS> before;   // the pieces before this wave's piece of row r
		before.h = rbk_readlane<unsigned>(pieces.h, (unsigned) r * RBK_WAVES + wave);
		before.a = AGG ? rbk_readlane<TS>(pieces.a, (unsigned) r * RBK_WAVES + wave) : (TS) 0;
		rbk_state<TS> s = rbk_combine<OP, AGG, TS>(rbk_combine<OP, AGG, TS>(tile_in, before), ex[r]);
		#pragma unroll
		for (int c = 0; c < RBK_VEC; ++c) {
			R::advance(s, hb[r], v[r], c, flip);
			// the element ends a run: it is the last one, or the next one is a head
			const size_t rank = (size_t) s.h - 1u;   // (below n by construction; checked all the same: it is an address)
			if (i0 + c < n && ((hb[r] >> (c + 1)) & 1u) && rank < n) {
				if (keys_out) keys_out[rank] = k[r][c];
				if constexpr (AGG) aggr_out[rank] = OP == RBK_SUM ? s.a : (TS) (s.a ^ flip);
			}
		}
	}
}

struct rbk_args {
	const void* keys_in; const void* values_in; void* keys_out; void* aggr_out; unsigned long long* num_runs;
	size_t n; unsigned long long flip; void* ws; hipStream_t s;
};

inline size_t rbk_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }
constexpr size_t RBK_MIN_TILE = (size_t) RBK_ROW_ELEMS * 4;
inline size_t rbk_max_tiles(size_t numel) { return (numel + RBK_MIN_TILE - 1) / RBK_MIN_TILE + 1; }

template <typename TK, int CVT, int OP>
int rbk_launch(const rbk_args& a) {
	typedef typename rbk_cvt<CVT>::TV TV;
	typedef typename rbk_cvt<CVT>::TS TS;
	constexpr int ROWS = rbk_rows((int) sizeof(TK), rbk_cvt<CVT>::vs);
	const size_t tile = (size_t) ROWS * RBK_ROW_ELEMS;
	const unsigned tiles = (unsigned) ((a.n + tile - 1) / tile);
	unsigned* tile_h = (unsigned*) a.ws;
	TS* tile_a = (TS*) ((char*) a.ws + rbk_align(rbk_max_tiles(a.n) * sizeof(unsigned)));
	const int kvec = (uintptr_t) a.keys_in % (RBK_VEC * sizeof(TK)) == 0;
	const int vvec = (uintptr_t) a.values_in % (RBK_VEC * sizeof(TV)) == 0;
	{
		clo_timing_scope timing("rbk_sweep", a.s);
		hipLaunchKernelGGL((clo_rbk_sweep_kernel<TK, CVT, OP, ROWS>), dim3(tiles), dim3(RBK_THREADS), 0, a.s,
			(const TK*) a.keys_in, (const TV*) a.values_in, a.n, tile_h, tile_a, (TS) a.flip, kvec, vvec);
	}
	{
		clo_timing_scope timing("rbk_states", a.s);
		hipLaunchKernelGGL((clo_rbk_states_kernel<CVT, OP>), dim3(1), dim3(RBK_THREADS), 0, a.s, tile_h, tile_a, tiles, a.num_runs);
	}
	{
		clo_timing_scope timing("rbk_apply", a.s);
		hipLaunchKernelGGL((clo_rbk_apply_kernel<TK, CVT, OP, ROWS>), dim3(tiles), dim3(RBK_THREADS), 0, a.s,
			(const TK*) a.keys_in, (const TV*) a.values_in, a.n, (const unsigned*) tile_h, (const TS*) tile_a, (TS) a.flip, kvec, vvec,
			(TK*) a.keys_out, (TS*) a.aggr_out);
	}
	return (int) hipGetLastError();
}

template <typename TK, int CVT>
int rbk_dispatch_op(const rbk_args& a, int op) {
	if constexpr (CVT == RBK_CVT_NONE || CVT == RBK_CVT_ONE32 || CVT == RBK_CVT_ONE64) {
		return rbk_launch<TK, CVT, RBK_SUM>(a);   // (no values: min / max were refused; no aggregate: the op is not used)
	} else {
		switch (op) {
			case RBK_SUM: return rbk_launch<TK, CVT, RBK_SUM>(a);
			case RBK_MIN: return rbk_launch<TK, CVT, RBK_MIN>(a);
			case RBK_MAX: return rbk_launch<TK, CVT, RBK_MAX>(a);
			default: return CLO_HIP_EARGS;
		}
	}
}

template <typename TK>
int rbk_dispatch_cvt(const rbk_args& a, int cvt, int op) {
	switch (cvt) {
		case RBK_CVT_NONE: return rbk_dispatch_op<TK, RBK_CVT_NONE>(a, op);
		case RBK_CVT_32: return rbk_dispatch_op<TK, RBK_CVT_32>(a, op);
		case RBK_CVT_S64: return rbk_dispatch_op<TK, RBK_CVT_S64>(a, op);
		case RBK_CVT_U64: return rbk_dispatch_op<TK, RBK_CVT_U64>(a, op);
		case RBK_CVT_64: return rbk_dispatch_op<TK, RBK_CVT_64>(a, op);
		case RBK_CVT_ONE32: return rbk_dispatch_op<TK, RBK_CVT_ONE32>(a, op);
		case RBK_CVT_ONE64: return rbk_dispatch_op<TK, RBK_CVT_ONE64>(a, op);
		default: return CLO_HIP_EUNSUPPORTED;
	}
}

// CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7
inline bool rbk_int_type(int t) { return t >= 4 && t <= 7; }
inline int rbk_type_size(int t) { return t >= 6 ? 8 : 4; }
inline bool rbk_type_signed(int t) { return t == 4 || t == 6; }

// which conversion the kernels make, or -1: a pair of types this library does not reduce
int rbk_cvt_of(bool aggr, bool vals, int value_type, int sum_type) {
	if (!aggr) return RBK_CVT_NONE;
	if (!rbk_int_type(sum_type)) return -1;
	const int ss = rbk_type_size(sum_type);
	if (!vals) return ss == 8 ? RBK_CVT_ONE64 : RBK_CVT_ONE32;
	if (!rbk_int_type(value_type)) return -1;
	const int vs = rbk_type_size(value_type);
	if (ss < vs) return -1;
	if (ss == 4) return RBK_CVT_32;
	if (vs == 8) return RBK_CVT_64;
	return rbk_type_signed(value_type) ? RBK_CVT_S64 : RBK_CVT_U64;
}

}  // namespace

extern "C" {

size_t clo_hip_reduce_by_key_tile(int key_size, int value_size) {
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return 0;
	if (value_size != 0 && value_size != 4 && value_size != 8) return 0;
	return (size_t) rbk_rows(key_size, value_size) * RBK_ROW_ELEMS;
}

size_t clo_hip_reduce_by_key_workspace_bytes(size_t numel) {
	const size_t t = rbk_max_tiles(numel);
	return rbk_align(t * sizeof(unsigned)) + rbk_align(t * sizeof(unsigned long long));
}

int clo_hip_reduce_by_key(const void* keys_in, const void* values_in, void* keys_out, void* aggr_out, uint64_t* num_runs_dev,
	size_t numel, int key_size, int value_type, int sum_type, int op, void* workspace, size_t workspace_bytes, void* stream) {
	hipStream_t s = (hipStream_t) stream;
	if (!num_runs_dev || clo_misaligned(num_runs_dev, 8) || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (!keys_out && !aggr_out) return CLO_HIP_EARGS;
	if (op != RBK_SUM && op != RBK_MIN && op != RBK_MAX) return CLO_HIP_EARGS;
	if (aggr_out && !values_in && op != RBK_SUM) return CLO_HIP_EARGS;   // the min / max of ones
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int cvt = rbk_cvt_of(aggr_out != nullptr, values_in != nullptr, value_type, sum_type);
	if (cvt < 0) return CLO_HIP_EUNSUPPORTED;
	if (numel == 0) return (int) hipMemsetAsync(num_runs_dev, 0, sizeof(uint64_t), s);   // no runs, no launch
	if (!keys_in || !workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_reduce_by_key_workspace_bytes(numel)) return CLO_HIP_EWORKSPACE;

	rbk_args a;
	a.keys_in = keys_in; a.values_in = cvt == RBK_CVT_NONE ? nullptr : values_in; a.keys_out = keys_out; a.aggr_out = aggr_out;
	a.num_runs = (unsigned long long*) num_runs_dev; a.n = numel; a.ws = workspace; a.s = s;
	// min / max in a signed sum type: compared as unsigned numbers with the sign bit flipped
	a.flip = (op != RBK_SUM && aggr_out && rbk_type_signed(sum_type)) ? 1ull << (8 * rbk_type_size(sum_type) - 1) : 0ull;
	switch (key_size) {
		case 1: return rbk_dispatch_cvt<uint8_t>(a, cvt, op);
		case 2: return rbk_dispatch_cvt<uint16_t>(a, cvt, op);
		case 4: return rbk_dispatch_cvt<uint32_t>(a, cvt, op);
		default: return rbk_dispatch_cvt<uint64_t>(a, cvt, op);
	}
}

}  // extern "C"
