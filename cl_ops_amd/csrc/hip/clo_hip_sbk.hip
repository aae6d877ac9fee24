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
// The segmented scan itself — the operator, the wave scan and the scan of a tile's pieces — is shared with reduce by
// key (clo_hip_op_device.h) and used here with an aggregate always (AGG = true). What differs here on purpose: loads
// and stores count inside the tile in 32 bits, the "next element is a head" bit and the run count are not needed,
// advance() is branch-free, and values / out carry no __restrict__, because out may be values_in itself (element i's
// result lands at index i, and a thread has loaded its elements of the tile before it stores any).
// A tile is 256 threads x 4 consecutive elements x ROWS rows; inside a tile the order is row, wave, lane, element.
// min / max are computed on unsigned numbers: a signed sum type has its sign bit flipped on load and on store.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

constexpr int SBK_THREADS = 256;
constexpr int SBK_WAVES = SBK_THREADS / 64;
constexpr int SBK_VEC = 4;
constexpr int SBK_ROW_ELEMS = SBK_THREADS * SBK_VEC;   // 1024
static_assert(SBK_THREADS == CLO_OP_THREADS && SBK_VEC == CLO_OP_VEC, "the shared helpers' work-group and vector");

// the conversions CLO_OP_CVT_* (clo_hip_op_device.h); the table keeps a name of its own here because the kernels'
// symbols spell it
template <int CVT> struct sbk_cvt : clo_op_cvt<CVT> {};

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
		TK prev = clo_op_shfl<TK>(k[SBK_VEC - 1], (int) lane - 1);
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
		else if constexpr (OP == CLO_OP_SUM) return (TS) v[c];
		else return (TS) ((TS) v[c] ^ flip);
	}

	// `s` continued over element c of the lane's four; returns what the run had gathered BEFORE the element: the
	// identity where the element is a head. Without a branch or a lane mask: the head bit, spread over the word,
	// clears the aggregate (sets it for min, whose identity is all ones).
	static __device__ __forceinline__ TS advance(clo_op_seg_state<TS>& s, unsigned hb, const TV (&v)[SBK_VEC], int c, TS flip) {
		const unsigned head = (hb >> c) & 1u;
		const TS spread = (TS) 0 - (TS) head;
		const TS before = OP == CLO_OP_MIN ? (TS) (s.a | spread) : (TS) (s.a & ~spread);
		s.a = clo_op_seg_op<OP, TS>(before, value(v, c, flip));
		s.h += head;
		return before;
	}
};

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
		clo_op_seg_state<TS> s = clo_op_seg_empty<OP, TS>();
		#pragma unroll
		for (int c = 0; c < SBK_VEC; ++c) R::advance(s, hb, v[r], c, flip);
		s = clo_op_seg_wave_scan<OP, true, TS>(s);
		if (lane == 63) {
			s_h[r * SBK_WAVES + wave] = s.h;
			s_a[r * SBK_WAVES + wave] = s.a;
		}
	}
	__syncthreads();
	if (wave == 0) {
		clo_op_seg_state<TS> total;
		(void) clo_op_seg_scan_pieces<OP, true, TS, PIECES>(s_h, s_a, lane, &total);
		if (lane == 0) {
			tile_h[blockIdx.x] = total.h;
			tile_a[blockIdx.x] = total.a;
		}
	}
}

// ---- 2. state scan: one group; tile t gets the state of the tiles before it, in place. (clo_rbk_states_kernel's body
// with AGG = true and no run count; as one shared function both compiled to other instructions, so each file keeps its own.) ----
template <int CVT, int OP>
__global__ __launch_bounds__(SBK_THREADS)
void clo_sbk_states_kernel(unsigned* __restrict__ tile_h, typename sbk_cvt<CVT>::TS* __restrict__ tile_a, unsigned tiles) {
	typedef typename sbk_cvt<CVT>::TS TS;
	constexpr int PER = 4;   // consecutive states per thread
	__shared__ unsigned s_h[SBK_WAVES];
	__shared__ TS s_a[SBK_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	clo_op_seg_state<TS> running = clo_op_seg_empty<OP, TS>();   // the state of everything before this chunk (the same in every thread)
	for (unsigned chunk = 0; chunk < tiles; chunk += SBK_THREADS * PER) {
		const unsigned t0 = chunk + tid * PER;
		clo_op_seg_state<TS> st[PER];
		clo_op_seg_state<TS> mine = clo_op_seg_empty<OP, TS>();
		#pragma unroll
		for (int j = 0; j < PER; ++j) {
			st[j] = clo_op_seg_empty<OP, TS>();
			if (t0 + j < tiles) {
				st[j].h = tile_h[t0 + j];
				st[j].a = tile_a[t0 + j];
			}
			mine = clo_op_seg_combine<OP, true, TS>(mine, st[j]);
		}
		const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, true, TS>(mine);
		if (lane == 63) {
			s_h[wave] = incl.h;
			s_a[wave] = incl.a;
		}
		__syncthreads();
		clo_op_seg_state<TS> before = running, all = running;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) SBK_WAVES; ++w) {
			clo_op_seg_state<TS> p;
			p.h = s_h[w];
			p.a = s_a[w];
			if (w < wave) before = clo_op_seg_combine<OP, true, TS>(before, p);
			all = clo_op_seg_combine<OP, true, TS>(all, p);
		}
		clo_op_seg_state<TS> s = clo_op_seg_combine<OP, true, TS>(before, clo_op_seg_wave_exclusive<OP, true, TS>(incl, lane));
		#pragma unroll
		for (int j = 0; j < PER; ++j) {
			if (t0 + j < tiles) {
				tile_h[t0 + j] = s.h;
				tile_a[t0 + j] = s.a;
			}
			s = clo_op_seg_combine<OP, true, TS>(s, st[j]);
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
	clo_op_seg_state<TS> ex[ROWS];   // the lanes of this wave before this one, per row
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
			clo_op_seg_state<TS> s = clo_op_seg_empty<OP, TS>();
			#pragma unroll
			for (int c = 0; c < SBK_VEC; ++c) R::advance(s, hb[r], v[r], c, flip);
			s = clo_op_seg_wave_scan<OP, true, TS>(s);
			if (lane == 63) {
				s_h[r * SBK_WAVES + wave] = s.h;
				s_a[r * SBK_WAVES + wave] = s.a;
			}
			ex[r] = clo_op_seg_wave_exclusive<OP, true, TS>(s, lane);
		}
	}
	// the carry into the tile: the open run's aggregate so far (its head count does not matter here)
	clo_op_seg_state<TS> tile_in;
	tile_in.h = 0;
	tile_in.a = tile_a[blockIdx.x];
	__syncthreads();   // every thread of the group has loaded its elements: from here on `out` may be written over `values`
	// The stores test the bounds the loads tested. Left to itself the compiler keeps every one of those lane masks (an
	// SGPR pair each) alive from the loads across the barrier and spills SGPRs at 8 rows (44-48 of them in the
	// compiler's report); behind this empty statement it forms them again, one 32-bit compare each.
	unsigned lim2 = lim;
	asm volatile("" : "+s"(lim2));
	clo_op_seg_state<TS> total;
	const clo_op_seg_state<TS> pieces = clo_op_seg_scan_pieces<OP, true, TS, PIECES>(s_h, s_a, lane, &total);
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		clo_op_seg_state<TS> before;   // the pieces before this wave's piece of row r
		before.h = clo_op_readlane<unsigned>(pieces.h, (unsigned) r * SBK_WAVES + wave);
		before.a = clo_op_readlane<TS>(pieces.a, (unsigned) r * SBK_WAVES + wave);
		clo_op_seg_state<TS> s = clo_op_seg_combine<OP, true, TS>(clo_op_seg_combine<OP, true, TS>(tile_in, before), ex[r]);
		TS res[SBK_VEC];
		#pragma unroll
		for (int c = 0; c < SBK_VEC; ++c) {
			const TS excl = R::advance(s, hb[r], v[r], c, flip);   // the identity where the element starts a run
			const TS x = inclusive ? s.a : excl;
			res[c] = OP == CLO_OP_SUM ? x : (TS) (x ^ flip);
		}
		sbk_store4<TS>(out + tile_base, tid * SBK_VEC + r * SBK_ROW_ELEMS, lim2, ovec != 0, res);
	}
}

struct sbk_args {
	const void* keys_in; const void* values_in; void* out;
	size_t n; unsigned long long flip; int inclusive; void* ws; hipStream_t s;
};

template <typename TK, int CVT, int OP>
int sbk_launch(const sbk_args& a) {
	typedef typename sbk_cvt<CVT>::TV TV;
	typedef typename sbk_cvt<CVT>::TS TS;
	constexpr int ROWS = clo_op_seg_rows((int) sizeof(TK), sbk_cvt<CVT>::vs);
	const size_t tile = (size_t) ROWS * SBK_ROW_ELEMS;
	const unsigned tiles = (unsigned) ((a.n + tile - 1) / tile);
	unsigned* tile_h = (unsigned*) a.ws;
	TS* tile_a = (TS*) ((char*) a.ws + clo_op_ws_align(clo_op_seg_max_tiles(a.n) * sizeof(unsigned)));
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
	if constexpr (CVT == CLO_OP_CVT_ONE32 || CVT == CLO_OP_CVT_ONE64) {
		return sbk_launch<TK, CVT, CLO_OP_SUM>(a);   // (no values: min / max were refused)
	} else {
		switch (op) {
			case CLO_OP_SUM: return sbk_launch<TK, CVT, CLO_OP_SUM>(a);
			case CLO_OP_MIN: return sbk_launch<TK, CVT, CLO_OP_MIN>(a);
			case CLO_OP_MAX: return sbk_launch<TK, CVT, CLO_OP_MAX>(a);
			default: return CLO_HIP_EARGS;
		}
	}
}

template <typename TK>
int sbk_dispatch_cvt(const sbk_args& a, int cvt, int op) {
	switch (cvt) {
		case CLO_OP_CVT_32: return sbk_dispatch_op<TK, CLO_OP_CVT_32>(a, op);
		case CLO_OP_CVT_S64: return sbk_dispatch_op<TK, CLO_OP_CVT_S64>(a, op);
		case CLO_OP_CVT_U64: return sbk_dispatch_op<TK, CLO_OP_CVT_U64>(a, op);
		case CLO_OP_CVT_64: return sbk_dispatch_op<TK, CLO_OP_CVT_64>(a, op);
		case CLO_OP_CVT_ONE32: return sbk_dispatch_op<TK, CLO_OP_CVT_ONE32>(a, op);
		case CLO_OP_CVT_ONE64: return sbk_dispatch_op<TK, CLO_OP_CVT_ONE64>(a, op);
		default: return CLO_HIP_EUNSUPPORTED;   // (CLO_OP_CVT_NONE too: a scan always has an aggregate)
	}
}

}  // namespace

extern "C" {

size_t clo_hip_scan_by_key_tile(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return (size_t) clo_op_seg_rows(key_size, value_size) * SBK_ROW_ELEMS;
}

size_t clo_hip_scan_by_key_workspace_bytes(size_t numel) { return clo_op_seg_workspace_bytes(numel); }

int clo_hip_scan_by_key(const void* keys_in, const void* values_in, void* out, size_t numel,
	int key_size, int value_type, int sum_type, int op, int inclusive,
	void* workspace, size_t workspace_bytes, void* stream) {
	hipStream_t s = (hipStream_t) stream;
	if (clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (op != CLO_OP_SUM && op != CLO_OP_MIN && op != CLO_OP_MAX) return CLO_HIP_EARGS;
	if (inclusive != 0 && inclusive != 1) return CLO_HIP_EARGS;
	if (!values_in && op != CLO_OP_SUM) return CLO_HIP_EARGS;   // the min / max of ones
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size)) return CLO_HIP_EUNSUPPORTED;
	const int cvt = clo_op_cvt_of(true, values_in != nullptr, value_type, sum_type);
	if (cvt < 0) return CLO_HIP_EUNSUPPORTED;
	if (numel == 0) return 0;   // nothing to scan, no launch
	if (!keys_in || !out || !workspace) return CLO_HIP_EARGS;
	if (clo_misaligned(out, (size_t) clo_op_type_size(sum_type))) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_scan_by_key_workspace_bytes(numel)) return CLO_HIP_EWORKSPACE;

	sbk_args a;
	a.keys_in = keys_in; a.values_in = values_in; a.out = out; a.n = numel; a.inclusive = inclusive; a.ws = workspace; a.s = s;
	// min / max in a signed sum type: compared as unsigned numbers with the sign bit flipped
	a.flip = (op != CLO_OP_SUM && clo_op_type_signed(sum_type)) ? 1ull << (8 * clo_op_type_size(sum_type) - 1) : 0ull;
	return clo_op_by_key_size(key_size, [&](auto tk) { return sbk_dispatch_cvt<decltype(tk)>(a, cvt, op); });
}

}  // extern "C"
