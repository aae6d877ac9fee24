// clo_hip_sbk.hip — scan by key (CloScanByKey, include/clo_scan_by_key.h; not upstream): every element gets the
// running sum / min / max of the values of its RUN up to it (inclusive) or before it (exclusive; the identity at
// the run's first element), a run being a maximal stretch of consecutive elements whose keys have the same bytes.
// Without values every value is 1: the exclusive sum is the element's rank in its run.
//
// The three-launch schedule of reduce by key (clo_hip_rbk.hip); no work-group ever waits
// for another:
//   1. tile sweep   a group reads one tile and writes its STATE (heads, tail): the number of run heads in the
//                   tile, and the aggregate of the values from the tile's last head to its end (of the whole tile
//                   when it has no head);
//   2. state scan   one group walks the tile states with the segmented-scan operator
//                       (hL, aL) o (hR, aR) = (hL + hR, hR ? aR : aL op aR)
//                   and leaves, per tile, the state of everything before it; the scan by key uses its carry (the
//                   open run's aggregate so far), which the operator drops by itself at the tile's first head;
//   3. apply sweep  a group reads its tile again, runs the same segmented scan over it starting from the tile's
//                   incoming state, and stores EVERY element: the state before the element's own step (the identity
//                   where the element is a head) for the exclusive form, after it for the inclusive form.
// This file carries its own copies of the helpers and of the first two kernels of clo_hip_rbk.hip (which stays as it
// is): here there is always an aggregate, the "next element is a head" bit and the run count are not needed, and
// values / out carry no __restrict__, because out may be values_in itself (element i's result lands at index i, and
// a thread has loaded its elements of the tile before it stores any).
// A tile is 256 threads x 4 consecutive elements x ROWS rows; inside a tile the order is row, wave, lane, element.
// min / max are computed on unsigned numbers: a signed sum type has its sign bit flipped on load and on store.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "clo_hip.h"
#include "clo_hip_internal.h"

namespace {

constexpr int SBK_THREADS = 256;
constexpr int SBK_WAVES = SBK_THREADS / 64;
constexpr int SBK_VEC = 4;
constexpr int SBK_ROW_ELEMS = SBK_THREADS * SBK_VEC;   // 1024

// rows per tile: the rule of reduce by key (256 bytes of keys and values per thread at most)
constexpr int sbk_rows(int key_size, int value_size) { return key_size + value_size <= 8 ? 8 : 4; }

enum { SBK_SUM = 0, SBK_MIN = 1, SBK_MAX = 2 };
// How a value becomes a number of the sum type, `(sum type) x` seen as bits:
enum {
	SBK_CVT_32 = 0,      // 32-bit value, 32-bit sum
	SBK_CVT_S64 = 1,     // int value, 64-bit sum (sign extension)
	SBK_CVT_U64 = 2,     // uint value, 64-bit sum
	SBK_CVT_64 = 3,      // 64-bit value, 64-bit sum
	SBK_CVT_ONE32 = 4,   // values absent: every value is 1, 32-bit sum
	SBK_CVT_ONE64 = 5    // the same, 64-bit sum
};
template <int CVT> struct sbk_cvt;
template <> struct sbk_cvt<SBK_CVT_32> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 4; };
template <> struct sbk_cvt<SBK_CVT_S64> { typedef int32_t TV; typedef uint64_t TS; static constexpr int vs = 4; };
template <> struct sbk_cvt<SBK_CVT_U64> { typedef uint32_t TV; typedef uint64_t TS; static constexpr int vs = 4; };
template <> struct sbk_cvt<SBK_CVT_64> { typedef uint64_t TV; typedef uint64_t TS; static constexpr int vs = 8; };
template <> struct sbk_cvt<SBK_CVT_ONE32> { typedef uint32_t TV; typedef uint32_t TS; static constexpr int vs = 0; };
template <> struct sbk_cvt<SBK_CVT_ONE64> { typedef uint32_t TV; typedef uint64_t TS; static constexpr int vs = 0; };

template <int OP, typename TS>
__device__ __forceinline__ constexpr TS sbk_identity() { return OP == SBK_MIN ? (TS) ~(TS) 0 : (TS) 0; }
template <int OP, typename TS>
__device__ __forceinline__ TS sbk_op(TS a, TS b) {
	if constexpr (OP == SBK_SUM) return (TS) (a + b);
	else if constexpr (OP == SBK_MIN) return a < b ? a : b;
	else return a > b ? a : b;
}

// The state of a stretch of elements: the heads in it, and the aggregate from its last head (from its start
// when it has none) to its end.
template <typename TS>
struct sbk_state { unsigned h; TS a; };

template <int OP, typename TS>
__device__ __forceinline__ sbk_state<TS> sbk_combine(const sbk_state<TS>& l, const sbk_state<TS>& r) {
	sbk_state<TS> o;
	o.h = l.h + r.h;
	o.a = r.h ? r.a : sbk_op<OP, TS>(l.a, r.a);
	return o;
}
template <int OP, typename TS>
__device__ __forceinline__ sbk_state<TS> sbk_empty() { sbk_state<TS> o; o.h = 0; o.a = sbk_identity<OP, TS>(); return o; }

// One DPP move of a 32- or 64-bit integer; a lane without a source (and every lane of a row the mask leaves out)
// gets `old`.
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ T sbk_dpp(T old, T x) {
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

template <int OP, int CTRL, int ROW_MASK, typename TS>
__device__ __forceinline__ void sbk_seg_step(sbk_state<TS>& s) {
	sbk_state<TS> l;
	l.h = sbk_dpp<CTRL, ROW_MASK, unsigned>(0u, s.h);
	l.a = sbk_dpp<CTRL, ROW_MASK, TS>(sbk_identity<OP, TS>(), s.a);
	s = sbk_combine<OP, TS>(l, s);
}

// Inclusive segmented scan of the 64 lane states of a whole wave: the network of clo_wave_scan_inclusive
// (clo_hip_internal.h) with the operator above.
template <int OP, typename TS>
__device__ __forceinline__ sbk_state<TS> sbk_wave_scan(sbk_state<TS> s) {
	sbk_seg_step<OP, 0x111, 0xF, TS>(s);   // row_shr:1
	sbk_seg_step<OP, 0x112, 0xF, TS>(s);   // row_shr:2
	sbk_seg_step<OP, 0x114, 0xF, TS>(s);   // row_shr:4
	sbk_seg_step<OP, 0x118, 0xF, TS>(s);   // row_shr:8
	sbk_seg_step<OP, 0x142, 0xA, TS>(s);   // row_bcast:15 into rows 1 and 3
	sbk_seg_step<OP, 0x143, 0xC, TS>(s);   // row_bcast:31 into rows 2 and 3
	return s;
}

template <typename T>
__device__ __forceinline__ T sbk_shfl(T v, int src_lane) {
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
template <int OP, typename TS>
__device__ __forceinline__ sbk_state<TS> sbk_wave_exclusive(const sbk_state<TS>& incl, unsigned lane) {
	sbk_state<TS> e;
	e.h = sbk_shfl<unsigned>(incl.h, (int) lane - 1);
	e.a = sbk_shfl<TS>(incl.a, (int) lane - 1);
	return lane == 0 ? sbk_empty<OP, TS>() : e;
}

template <typename T>
__device__ __forceinline__ T sbk_readlane(T v, unsigned lane) {   // `lane` is wave-uniform
	if constexpr (sizeof(T) == 8) {
		const unsigned long long b = (unsigned long long) v;
		const unsigned lo = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) b, (int) lane);
		const unsigned hi = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) (b >> 32), (int) lane);
		return (T) (((unsigned long long) hi << 32) | lo);
	} else {
		return (T) (unsigned) __builtin_amdgcn_readlane((int) (unsigned) v, (int) lane);
	}
}

// Where a lane's elements lie is counted inside the TILE, in 32 bits: `t` points to the tile's first element, `off`
// (a multiple of 4) is the lane's first element of a row in the tile, and `lim` the number of elements the tile has
// (the tile size, less in the array's last tile). A bound is then one 32-bit compare against a scalar, and an
// address the tile's scalar base plus a 32-bit lane offset.
//
// Four consecutive elements from `off`: one vector load where the array's start allows it and all four exist, else
// one by one; elements past the end read as 0. (No __restrict__: the values may be the array the apply sweep
// stores to.)
template <typename T>
__device__ __forceinline__ void sbk_load4(const T* t, unsigned off, unsigned lim, bool vec_ok, T (&v)[SBK_VEC]) {
	if (vec_ok && off + SBK_VEC <= lim) {
		typedef T vec4 __attribute__((ext_vector_type(4)));
		const vec4 x = *reinterpret_cast<const vec4*>(t + off);
		v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
	} else {
		#pragma unroll
		for (int c = 0; c < SBK_VEC; ++c) v[c] = off + c < lim ? t[off + c] : (T) 0;
	}
}

// The counterpart for the results: 16-byte vector stores (one for 32-bit sums, two for 64-bit) where `out` is
// 16-byte aligned and all four elements exist, else element by element; nothing is stored at or past the end.
template <typename T>
__device__ __forceinline__ void sbk_store4(T* t, unsigned off, unsigned lim, bool vec_ok, const T (&v)[SBK_VEC]) {
	if (vec_ok && off + SBK_VEC <= lim) {
		if constexpr (sizeof(T) == 4) {
			typedef T vec4 __attribute__((ext_vector_type(4)));
			vec4 x; x.x = v[0]; x.y = v[1]; x.z = v[2]; x.w = v[3];
			*reinterpret_cast<vec4*>(t + off) = x;
		} else {
			typedef T vec2 __attribute__((ext_vector_type(2)));
			vec2 x, y; x.x = v[0]; x.y = v[1]; y.x = v[2]; y.y = v[3];
			*reinterpret_cast<vec2*>(t + off) = x;
			*reinterpret_cast<vec2*>(t + off + 2) = y;
		}
	} else {
		#pragma unroll
		for (int c = 0; c < SBK_VEC; ++c) if (off + c < lim) t[off + c] = v[c];
	}
}

// What both sweeps know about one row of a lane: bit c of `heads` = element c starts a run; the lane's state; the
// values as numbers of the sum type.
template <typename TK, int CVT, int OP>
struct sbk_row {
	typedef typename sbk_cvt<CVT>::TV TV;
	typedef typename sbk_cvt<CVT>::TS TS;
	static constexpr bool VALS = sbk_cvt<CVT>::vs != 0;

	// `first`: the tile is the array's first (its element 0 has no left neighbour and is a head)
	static __device__ __forceinline__ unsigned heads(const TK* __restrict__ t, const TK (&k)[SBK_VEC], unsigned off, unsigned lim, bool first, unsigned lane) {
		// the key before the lane's first: the lane below has it, lane 0 reads it (the tile's first element: across the tile edge)
		TK prev = sbk_shfl<TK>(k[SBK_VEC - 1], (int) lane - 1);
		const bool start = first && off == 0;
		if (lane == 0 && !start && off < lim) prev = t[(ptrdiff_t) off - 1];
		unsigned hb = 0;
		if (off < lim && (start || k[0] != prev)) hb |= 1u;
		#pragma unroll
		for (int c = 1; c < SBK_VEC; ++c) if (off + c < lim && k[c] != k[c - 1]) hb |= 1u << c;
		return hb;
	}

	static __device__ __forceinline__ TS value(const TV (&v)[SBK_VEC], int c, TS flip) {
		if constexpr (!VALS) return (TS) 1;
		else if constexpr (OP == SBK_SUM) return (TS) v[c];
		else return (TS) ((TS) v[c] ^ flip);
	}

	// `s` continued over element c of the lane's four; returns what the run had gathered BEFORE the element: the
	// identity where the element is a head. Without a branch or a lane mask: the head bit, spread over the word,
	// clears the aggregate (sets it for min, whose identity is all ones).
	static __device__ __forceinline__ TS advance(sbk_state<TS>& s, unsigned hb, const TV (&v)[SBK_VEC], int c, TS flip) {
		const unsigned head = (hb >> c) & 1u;
		const TS spread = (TS) 0 - (TS) head;
		const TS before = OP == SBK_MIN ? (TS) (s.a | spread) : (TS) (s.a & ~spread);
		s.a = sbk_op<OP, TS>(before, value(v, c, flip));
		s.h += head;
		return before;
	}
};

// The pieces of a tile (ROWS x SBK_WAVES wave totals, in LDS, written before the tile's barrier): every wave scans
// them for itself; piece p's exclusive state comes back for p = row * SBK_WAVES + wave.
template <int OP, typename TS, int PIECES>
__device__ __forceinline__ sbk_state<TS> sbk_scan_pieces(const unsigned* s_h, const TS* s_a, unsigned lane, sbk_state<TS>* total) {
	static_assert(PIECES <= 64, "one piece per lane");
	sbk_state<TS> p = sbk_empty<OP, TS>();
	if (lane < (unsigned) PIECES) {
		p.h = s_h[lane];
		p.a = s_a[lane];
	}
	const sbk_state<TS> incl = sbk_wave_scan<OP, TS>(p);
	total->h = sbk_readlane<unsigned>(incl.h, 63u);
	total->a = sbk_readlane<TS>(incl.a, 63u);
	return sbk_wave_exclusive<OP, TS>(incl, lane);
}

// ---- 1. tile sweep ----
template <typename TK, int CVT, int OP, int ROWS>
__global__ __launch_bounds__(SBK_THREADS)
void clo_sbk_sweep_kernel(const TK* __restrict__ keys, const typename sbk_cvt<CVT>::TV* __restrict__ values, size_t n,
	unsigned* __restrict__ tile_h, typename sbk_cvt<CVT>::TS* __restrict__ tile_a, typename sbk_cvt<CVT>::TS flip, int kvec, int vvec) {
	typedef sbk_row<TK, CVT, OP> R;
	typedef typename R::TV TV;
	typedef typename R::TS TS;
	constexpr int PIECES = ROWS * SBK_WAVES;
	__shared__ unsigned s_h[PIECES];
	__shared__ TS s_a[PIECES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	constexpr unsigned TILE = ROWS * SBK_ROW_ELEMS;
	const size_t tile_base = (size_t) blockIdx.x * TILE;
	const unsigned lim = n - tile_base < (size_t) TILE ? (unsigned) (n - tile_base) : TILE;
	const TK* tk = keys + tile_base;
	const TV* tv = values + tile_base;

	TK k[ROWS][SBK_VEC];
	TV v[ROWS][SBK_VEC];
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		sbk_load4<TK>(tk, tid * SBK_VEC + r * SBK_ROW_ELEMS, lim, kvec != 0, k[r]);
		if constexpr (R::VALS) sbk_load4<TV>(tv, tid * SBK_VEC + r * SBK_ROW_ELEMS, lim, vvec != 0, v[r]);
	}
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const unsigned hb = R::heads(tk, k[r], tid * SBK_VEC + r * SBK_ROW_ELEMS, lim, blockIdx.x == 0, lane);
		sbk_state<TS> s = sbk_empty<OP, TS>();
		#pragma unroll
		for (int c = 0; c < SBK_VEC; ++c) R::advance(s, hb, v[r], c, flip);
		s = sbk_wave_scan<OP, TS>(s);
		if (lane == 63) {
			s_h[r * SBK_WAVES + wave] = s.h;
			s_a[r * SBK_WAVES + wave] = s.a;
		}
	}
	__syncthreads();
	if (wave == 0) {
		sbk_state<TS> total;
		(void) sbk_scan_pieces<OP, TS, PIECES>(s_h, s_a, lane, &total);
		if (lane == 0) {
			tile_h[blockIdx.x] = total.h;
			tile_a[blockIdx.x] = total.a;
		}
	}
}

// ---- 2. state scan: one group; tile t gets the state of the tiles before it, in place ----
template <int CVT, int OP>
__global__ __launch_bounds__(SBK_THREADS)
void clo_sbk_states_kernel(unsigned* __restrict__ tile_h, typename sbk_cvt<CVT>::TS* __restrict__ tile_a, unsigned tiles) {
	typedef typename sbk_cvt<CVT>::TS TS;
	constexpr int PER = 4;   // consecutive states per thread
	__shared__ unsigned s_h[SBK_WAVES];
	__shared__ TS s_a[SBK_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	sbk_state<TS> running = sbk_empty<OP, TS>();   // the state of everything before this chunk (the same in every thread)
	for (unsigned chunk = 0; chunk < tiles; chunk += SBK_THREADS * PER) {
		const unsigned t0 = chunk + tid * PER;
		sbk_state<TS> st[PER];
		sbk_state<TS> mine = sbk_empty<OP, TS>();
		#pragma unroll
		for (int j = 0; j < PER; ++j) {
			st[j] = sbk_empty<OP, TS>();
			if (t0 + j < tiles) {
				st[j].h = tile_h[t0 + j];
				st[j].a = tile_a[t0 + j];
			}
			mine = sbk_combine<OP, TS>(mine, st[j]);
		}
		const sbk_state<TS> incl = sbk_wave_scan<OP, TS>(mine);
		if (lane == 63) {
			s_h[wave] = incl.h;
			s_a[wave] = incl.a;
		}
		__syncthreads();
		sbk_state<TS> before = running, all = running;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) SBK_WAVES; ++w) {
			sbk_state<TS> p;
			p.h = s_h[w];
			p.a = s_a[w];
			if (w < wave) before = sbk_combine<OP, TS>(before, p);
			all = sbk_combine<OP, TS>(all, p);
		}
		sbk_state<TS> s = sbk_combine<OP, TS>(before, sbk_wave_exclusive<OP, TS>(incl, lane));
		#pragma unroll
		for (int j = 0; j < PER; ++j) {
			if (t0 + j < tiles) {
				tile_h[t0 + j] = s.h;
				tile_a[t0 + j] = s.a;
			}
			s = sbk_combine<OP, TS>(s, st[j]);
		}
		running = all;
		__syncthreads();   // s_h / s_a are written again in the next chunk
	}
}

// ---- 3. apply sweep: every element stores its result. `values` and `out` may be the same array. ----
template <typename TK, int CVT, int OP, int ROWS>
__global__ __launch_bounds__(SBK_THREADS)
void clo_sbk_apply_kernel(const TK* __restrict__ keys, const typename sbk_cvt<CVT>::TV* values, size_t n,
	const typename sbk_cvt<CVT>::TS* __restrict__ tile_a, typename sbk_cvt<CVT>::TS flip, int kvec, int vvec, int ovec, int inclusive,
	typename sbk_cvt<CVT>::TS* out) {
	typedef sbk_row<TK, CVT, OP> R;
	typedef typename R::TV TV;
	typedef typename R::TS TS;
	constexpr int PIECES = ROWS * SBK_WAVES;
	__shared__ unsigned s_h[PIECES];
	__shared__ TS s_a[PIECES];
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	const unsigned wave = (unsigned) __builtin_amdgcn_readfirstlane((int) (tid >> 6));
	constexpr unsigned TILE = ROWS * SBK_ROW_ELEMS;
	const size_t tile_base = (size_t) blockIdx.x * TILE;
	const unsigned lim = n - tile_base < (size_t) TILE ? (unsigned) (n - tile_base) : TILE;
	const TK* tk = keys + tile_base;
	const TV* tv = values + tile_base;

	TV v[ROWS][SBK_VEC];
	unsigned hb[ROWS];
	sbk_state<TS> ex[ROWS];   // the lanes of this wave before this one, per row
	{
		TK k[ROWS][SBK_VEC];   // dead once the head bits are known
		#pragma unroll
		for (int r = 0; r < ROWS; ++r) {
			sbk_load4<TK>(tk, tid * SBK_VEC + r * SBK_ROW_ELEMS, lim, kvec != 0, k[r]);
			if constexpr (R::VALS) sbk_load4<TV>(tv, tid * SBK_VEC + r * SBK_ROW_ELEMS, lim, vvec != 0, v[r]);
		}
		#pragma unroll
		for (int r = 0; r < ROWS; ++r) {
			hb[r] = R::heads(tk, k[r], tid * SBK_VEC + r * SBK_ROW_ELEMS, lim, blockIdx.x == 0, lane);
			sbk_state<TS> s = sbk_empty<OP, TS>();
			#pragma unroll
			for (int c = 0; c < SBK_VEC; ++c) R::advance(s, hb[r], v[r], c, flip);
			s = sbk_wave_scan<OP, TS>(s);
			if (lane == 63) {
				s_h[r * SBK_WAVES + wave] = s.h;
				s_a[r * SBK_WAVES + wave] = s.a;
			}
			ex[r] = sbk_wave_exclusive<OP, TS>(s, lane);
		}
	}
	// the carry into the tile: the open run's aggregate so far (its head count does not matter here)
	sbk_state<TS> tile_in;
	tile_in.h = 0;
	tile_in.a = tile_a[blockIdx.x];
	__syncthreads();   // every thread of the group has loaded its elements: from here on `out` may be written over `values`
	// The stores test the bounds the loads tested. Left to itself the compiler keeps every one of those lane masks (an
	// SGPR pair each) alive from the loads across the barrier and spills SGPRs at 8 rows (44-48 of them in the
	// compiler's report); behind this empty statement it forms them again, one 32-bit compare each.
	unsigned lim2 = lim;
	asm volatile("" : "+s"(lim2));
	sbk_state<TS> total;
	const sbk_state<TS> pieces = sbk_scan_pieces<OP, TS, PIECES>(s_h, s_a, lane, &total);
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		sbk_state<TS> before;   // the pieces before this wave's piece of row r
		before.h = sbk_readlane<unsigned>(pieces.h, (unsigned) r * SBK_WAVES + wave);
		before.a = sbk_readlane<TS>(pieces.a, (unsigned) r * SBK_WAVES + wave);
		sbk_state<TS> s = sbk_combine<OP, TS>(sbk_combine<OP, TS>(tile_in, before), ex[r]);
		TS res[SBK_VEC];
		#pragma unroll
		for (int c = 0; c < SBK_VEC; ++c) {
			const TS excl = R::advance(s, hb[r], v[r], c, flip);   // the identity where the element starts a run
			const TS x = inclusive ? s.a : excl;
			res[c] = OP == SBK_SUM ? x : (TS) (x ^ flip);
		}
		sbk_store4<TS>(out + tile_base, tid * SBK_VEC + r * SBK_ROW_ELEMS, lim2, ovec != 0, res);
	}
}

struct sbk_args {
	const void* keys_in; const void* values_in; void* out;
	size_t n; unsigned long long flip; int inclusive; void* ws; hipStream_t s;
};

inline size_t sbk_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }
constexpr size_t SBK_MIN_TILE = (size_t) SBK_ROW_ELEMS * 4;
inline size_t sbk_max_tiles(size_t numel) { return (numel + SBK_MIN_TILE - 1) / SBK_MIN_TILE + 1; }

template <typename TK, int CVT, int OP>
int sbk_launch(const sbk_args& a) {
	typedef typename sbk_cvt<CVT>::TV TV;
	typedef typename sbk_cvt<CVT>::TS TS;
	constexpr int ROWS = sbk_rows((int) sizeof(TK), sbk_cvt<CVT>::vs);
	const size_t tile = (size_t) ROWS * SBK_ROW_ELEMS;
	const unsigned tiles = (unsigned) ((a.n + tile - 1) / tile);
	unsigned* tile_h = (unsigned*) a.ws;
	TS* tile_a = (TS*) ((char*) a.ws + sbk_align(sbk_max_tiles(a.n) * sizeof(unsigned)));
	const int kvec = (uintptr_t) a.keys_in % (SBK_VEC * sizeof(TK)) == 0;
	const int vvec = (uintptr_t) a.values_in % (SBK_VEC * sizeof(TV)) == 0;
	const int ovec = (uintptr_t) a.out % 16 == 0;
	{
		clo_timing_scope timing("sbk_sweep", a.s);
		hipLaunchKernelGGL((clo_sbk_sweep_kernel<TK, CVT, OP, ROWS>), dim3(tiles), dim3(SBK_THREADS), 0, a.s,
			(const TK*) a.keys_in, (const TV*) a.values_in, a.n, tile_h, tile_a, (TS) a.flip, kvec, vvec);
	}
	{
		clo_timing_scope timing("sbk_states", a.s);
		hipLaunchKernelGGL((clo_sbk_states_kernel<CVT, OP>), dim3(1), dim3(SBK_THREADS), 0, a.s, tile_h, tile_a, tiles);
	}
	{
		clo_timing_scope timing("sbk_apply", a.s);
		hipLaunchKernelGGL((clo_sbk_apply_kernel<TK, CVT, OP, ROWS>), dim3(tiles), dim3(SBK_THREADS), 0, a.s,
			(const TK*) a.keys_in, (const TV*) a.values_in, a.n, (const TS*) tile_a, (TS) a.flip, kvec, vvec, ovec, a.inclusive,
			(TS*) a.out);
	}
	return (int) hipGetLastError();
}

template <typename TK, int CVT>
int sbk_dispatch_op(const sbk_args& a, int op) {
	if constexpr (CVT == SBK_CVT_ONE32 || CVT == SBK_CVT_ONE64) {
		return sbk_launch<TK, CVT, SBK_SUM>(a);   // (no values: min / max were refused)
	} else {
		switch (op) {
			case SBK_SUM: return sbk_launch<TK, CVT, SBK_SUM>(a);
			case SBK_MIN: return sbk_launch<TK, CVT, SBK_MIN>(a);
			case SBK_MAX: return sbk_launch<TK, CVT, SBK_MAX>(a);
			default: return CLO_HIP_EARGS;
		}
	}
}

template <typename TK>
int sbk_dispatch_cvt(const sbk_args& a, int cvt, int op) {
	switch (cvt) {
		case SBK_CVT_32: return sbk_dispatch_op<TK, SBK_CVT_32>(a, op);
		case SBK_CVT_S64: return sbk_dispatch_op<TK, SBK_CVT_S64>(a, op);
		case SBK_CVT_U64: return sbk_dispatch_op<TK, SBK_CVT_U64>(a, op);
		case SBK_CVT_64: return sbk_dispatch_op<TK, SBK_CVT_64>(a, op);
		case SBK_CVT_ONE32: return sbk_dispatch_op<TK, SBK_CVT_ONE32>(a, op);
		case SBK_CVT_ONE64: return sbk_dispatch_op<TK, SBK_CVT_ONE64>(a, op);
		default: return CLO_HIP_EUNSUPPORTED;
	}
}

// CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7
inline bool sbk_int_type(int t) { return t >= 4 && t <= 7; }
inline int sbk_type_size(int t) { return t >= 6 ? 8 : 4; }
inline bool sbk_type_signed(int t) { return t == 4 || t == 6; }

// which conversion the kernels make, or -1: a pair of types this library does not scan
int sbk_cvt_of(bool vals, int value_type, int sum_type) {
	if (!sbk_int_type(sum_type)) return -1;
	const int ss = sbk_type_size(sum_type);
	if (!vals) return ss == 8 ? SBK_CVT_ONE64 : SBK_CVT_ONE32;
	if (!sbk_int_type(value_type)) return -1;
	const int vs = sbk_type_size(value_type);
	if (ss < vs) return -1;
	if (ss == 4) return SBK_CVT_32;
	if (vs == 8) return SBK_CVT_64;
	return sbk_type_signed(value_type) ? SBK_CVT_S64 : SBK_CVT_U64;
}

}  // namespace

extern "C" {

size_t clo_hip_scan_by_key_tile(int key_size, int value_size) {
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return 0;
	if (value_size != 0 && value_size != 4 && value_size != 8) return 0;
	return (size_t) sbk_rows(key_size, value_size) * SBK_ROW_ELEMS;
}

size_t clo_hip_scan_by_key_workspace_bytes(size_t numel) {
	const size_t t = sbk_max_tiles(numel);
	return sbk_align(t * sizeof(unsigned)) + sbk_align(t * sizeof(unsigned long long));
}

int clo_hip_scan_by_key(const void* keys_in, const void* values_in, void* out, size_t numel,
	int key_size, int value_type, int sum_type, int op, int inclusive,
	void* workspace, size_t workspace_bytes, void* stream) {
	hipStream_t s = (hipStream_t) stream;
	if (clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (op != SBK_SUM && op != SBK_MIN && op != SBK_MAX) return CLO_HIP_EARGS;
	if (inclusive != 0 && inclusive != 1) return CLO_HIP_EARGS;
	if (!values_in && op != SBK_SUM) return CLO_HIP_EARGS;   // the min / max of ones
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int cvt = sbk_cvt_of(values_in != nullptr, value_type, sum_type);
	if (cvt < 0) return CLO_HIP_EUNSUPPORTED;
	if (numel == 0) return 0;   // nothing to scan, no launch
	if (!keys_in || !out || !workspace) return CLO_HIP_EARGS;
	if (clo_misaligned(out, (size_t) sbk_type_size(sum_type))) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_scan_by_key_workspace_bytes(numel)) return CLO_HIP_EWORKSPACE;

	sbk_args a;
	a.keys_in = keys_in; a.values_in = values_in; a.out = out; a.n = numel; a.inclusive = inclusive; a.ws = workspace; a.s = s;
	// min / max in a signed sum type: compared as unsigned numbers with the sign bit flipped
	a.flip = (op != SBK_SUM && sbk_type_signed(sum_type)) ? 1ull << (8 * sbk_type_size(sum_type) - 1) : 0ull;
	switch (key_size) {
		case 1: return sbk_dispatch_cvt<uint8_t>(a, cvt, op);
		case 2: return sbk_dispatch_cvt<uint16_t>(a, cvt, op);
		case 4: return sbk_dispatch_cvt<uint32_t>(a, cvt, op);
		default: return sbk_dispatch_cvt<uint64_t>(a, cvt, op);
	}
}

}  // extern "C"
