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

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

constexpr int RBK_THREADS = 256;
constexpr int RBK_WAVES = RBK_THREADS / 64;
constexpr int RBK_VEC = 4;
constexpr int RBK_ROW_ELEMS = RBK_THREADS * RBK_VEC;   // 1024
static_assert(RBK_THREADS == CLO_OP_THREADS && RBK_VEC == CLO_OP_VEC, "the shared helpers' work-group and vector");

// the conversions CLO_OP_CVT_* (clo_hip_op_device.h); the table keeps a name of its own here because the kernels'
// symbols spell it
template <int CVT> struct rbk_cvt : clo_op_cvt<CVT> {};

// What both sweeps know about one row of a lane: bit c of `heads` = element c starts a run, bit 4 = the element
// after the lane's four does (or is the end of the array); the lane's state; the values as numbers of the sum type.
template <typename TK, int CVT, int OP>
struct rbk_row {
	typedef typename rbk_cvt<CVT>::TV TV;
	typedef typename rbk_cvt<CVT>::TS TS;
	static constexpr bool AGG = CVT != CLO_OP_CVT_NONE;
	static constexpr bool VALS = rbk_cvt<CVT>::vs != 0;

	// NEXT: also find out whether the element after the lane's four starts a run (the apply sweep's run ends)
	template <bool NEXT>
	static __device__ __forceinline__ unsigned heads(const TK* __restrict__ keys, const TK (&k)[RBK_VEC], size_t i0, size_t n, unsigned lane) {
		// the key before the lane's first: the lane below has it, lane 0 reads it (the tile's first element: across the tile edge)
		TK prev = clo_op_shfl<TK>(k[RBK_VEC - 1], (int) lane - 1);
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
		else if constexpr (OP == CLO_OP_SUM) return (TS) v[c];
		else return (TS) ((TS) v[c] ^ flip);
	}

	// `s` continued over the lane's four elements of one row
	static __device__ __forceinline__ void advance(clo_op_seg_state<TS>& s, unsigned hb, const TV (&v)[RBK_VEC], int c, TS flip) {
		if constexpr (AGG) {
			const TS x = value(v, c, flip);
			s.a = ((hb >> c) & 1u) ? x : clo_op_seg_op<OP, TS>(s.a, x);
		}
		s.h += (hb >> c) & 1u;
	}
};

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
		clo_op_load4<TK>(keys, base + (size_t) r * RBK_ROW_ELEMS, n, kvec != 0, k[r]);
		if constexpr (R::VALS) clo_op_load4<TV>(values, base + (size_t) r * RBK_ROW_ELEMS, n, vvec != 0, v[r]);
	}
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const size_t i0 = base + (size_t) r * RBK_ROW_ELEMS;
		const unsigned hb = R::template heads<false>(keys, k[r], i0, n, lane);
		clo_op_seg_state<TS> s = clo_op_seg_empty<OP, TS>();
		#pragma unroll
		for (int c = 0; c < RBK_VEC; ++c) R::advance(s, hb, v[r], c, flip);
		s = clo_op_seg_wave_scan<OP, AGG, TS>(s);
		if (lane == 63) {
			s_h[r * RBK_WAVES + wave] = s.h;
			if constexpr (AGG) s_a[r * RBK_WAVES + wave] = s.a;
		}
	}
	__syncthreads();
	if (wave == 0) {
		clo_op_seg_state<TS> total;
		(void) clo_op_seg_scan_pieces<OP, AGG, TS, PIECES>(s_h, s_a, lane, &total);
		if (lane == 0) {
			tile_h[blockIdx.x] = total.h;
			if constexpr (AGG) tile_a[blockIdx.x] = total.a;
		}
	}
}

// ---- 2. state scan: one group; tile t gets the state of the tiles before it, in place. (clo_sbk_states_kernel has the
// same body with AGG = true; as one shared function both compiled to other instructions, so each file keeps its own.) ----
template <int CVT, int OP>
__global__ __launch_bounds__(RBK_THREADS)
void clo_rbk_states_kernel(unsigned* __restrict__ tile_h, typename rbk_cvt<CVT>::TS* __restrict__ tile_a, unsigned tiles,
	unsigned long long* __restrict__ num_runs) {
	typedef typename rbk_cvt<CVT>::TS TS;
	constexpr bool AGG = CVT != CLO_OP_CVT_NONE;
	constexpr int PER = 4;   // consecutive states per thread
	__shared__ unsigned s_h[RBK_WAVES];
	__shared__ TS s_a[RBK_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	clo_op_seg_state<TS> running = clo_op_seg_empty<OP, TS>();   // the state of everything before this chunk (the same in every thread)
	for (unsigned chunk = 0; chunk < tiles; chunk += RBK_THREADS * PER) {
		const unsigned t0 = chunk + tid * PER;
		clo_op_seg_state<TS> st[PER];
		clo_op_seg_state<TS> mine = clo_op_seg_empty<OP, TS>();
		#pragma unroll
		for (int j = 0; j < PER; ++j) {
			st[j] = clo_op_seg_empty<OP, TS>();
			if (t0 + j < tiles) {
				st[j].h = tile_h[t0 + j];
				if constexpr (AGG) st[j].a = tile_a[t0 + j];
			}
			mine = clo_op_seg_combine<OP, AGG, TS>(mine, st[j]);
		}
		const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, AGG, TS>(mine);
		if (lane == 63) {
			s_h[wave] = incl.h;
			if constexpr (AGG) s_a[wave] = incl.a;
		}
		__syncthreads();
		clo_op_seg_state<TS> before = running, all = running;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) RBK_WAVES; ++w) {
			clo_op_seg_state<TS> p;
			p.h = s_h[w];
			p.a = AGG ? s_a[w] : (TS) 0;
			if (w < wave) before = clo_op_seg_combine<OP, AGG, TS>(before, p);
			all = clo_op_seg_combine<OP, AGG, TS>(all, p);
		}
		clo_op_seg_state<TS> s = clo_op_seg_combine<OP, AGG, TS>(before, clo_op_seg_wave_exclusive<OP, AGG, TS>(incl, lane));
		#pragma unroll
		for (int j = 0; j < PER; ++j) {
			if (t0 + j < tiles) {
				tile_h[t0 + j] = s.h;
				if constexpr (AGG) tile_a[t0 + j] = s.a;
			}
			s = clo_op_seg_combine<OP, AGG, TS>(s, st[j]);
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
		clo_op_load4<TK>(keys, base + (size_t) r * RBK_ROW_ELEMS, n, kvec != 0, k[r]);
		if constexpr (R::VALS) clo_op_load4<TV>(values, base + (size_t) r * RBK_ROW_ELEMS, n, vvec != 0, v[r]);
	}
	// the state of everything before the tile: heads before it, and the carry into it
	clo_op_seg_state<TS> tile_in;
	tile_in.h = tile_h[blockIdx.x];
	tile_in.a = AGG ? tile_a[blockIdx.x] : (TS) 0;

	unsigned hb[ROWS];
	clo_op_seg_state<TS> ex[ROWS];   // the lanes of this wave before this one, per row
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const size_t i0 = base + (size_t) r * RBK_ROW_ELEMS;
		hb[r] = R::template heads<true>(keys, k[r], i0, n, lane);
		clo_op_seg_state<TS> s = clo_op_seg_empty<OP, TS>();
		#pragma unroll
		for (int c = 0; c < RBK_VEC; ++c) R::advance(s, hb[r], v[r], c, flip);
		s = clo_op_seg_wave_scan<OP, AGG, TS>(s);
		if (lane == 63) {
			s_h[r * RBK_WAVES + wave] = s.h;
			if constexpr (AGG) s_a[r * RBK_WAVES + wave] = s.a;
		}
		ex[r] = clo_op_seg_wave_exclusive<OP, AGG, TS>(s, lane);
	}
	__syncthreads();
	clo_op_seg_state<TS> total;
	const clo_op_seg_state<TS> pieces = clo_op_seg_scan_pieces<OP, AGG, TS, PIECES>(s_h, s_a, lane, &total);
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const size_t i0 = base + (size_t) r * RBK_ROW_ELEMS;
		clo_op_seg_state<TS> before;   // the pieces before this wave's piece of row r
		before.h = clo_op_readlane<unsigned>(pieces.h, (unsigned) r * RBK_WAVES + wave);
		before.a = AGG ? clo_op_readlane<TS>(pieces.a, (unsigned) r * RBK_WAVES + wave) : (TS) 0;
		clo_op_seg_state<TS> s = clo_op_seg_combine<OP, AGG, TS>(clo_op_seg_combine<OP, AGG, TS>(tile_in, before), ex[r]);
		#pragma unroll
		for (int c = 0; c < RBK_VEC; ++c) {
			R::advance(s, hb[r], v[r], c, flip);
			// the element ends a run: it is the last one, or the next one is a head
			const size_t rank = (size_t) s.h - 1u;   // (below n by construction; checked all the same: it is an address)
			if (i0 + c < n && ((hb[r] >> (c + 1)) & 1u) && rank < n) {
				if (keys_out) keys_out[rank] = k[r][c];
				if constexpr (AGG) aggr_out[rank] = OP == CLO_OP_SUM ? s.a : (TS) (s.a ^ flip);
			}
		}
	}
}

struct rbk_args {
	const void* keys_in; const void* values_in; void* keys_out; void* aggr_out; unsigned long long* num_runs;
	size_t n; unsigned long long flip; void* ws; hipStream_t s;
};

template <typename TK, int CVT, int OP>
int rbk_launch(const rbk_args& a) {
	typedef typename rbk_cvt<CVT>::TV TV;
	typedef typename rbk_cvt<CVT>::TS TS;
	constexpr int ROWS = clo_op_seg_rows((int) sizeof(TK), rbk_cvt<CVT>::vs);
	const size_t tile = (size_t) ROWS * RBK_ROW_ELEMS;
	const unsigned tiles = (unsigned) ((a.n + tile - 1) / tile);
	unsigned* tile_h = (unsigned*) a.ws;
	TS* tile_a = (TS*) ((char*) a.ws + clo_op_ws_align(clo_op_seg_max_tiles(a.n) * sizeof(unsigned)));
	// (the alignment of all four elements, 32 bytes for 8-byte ones: more than clo_op_load4's two 16-byte loads need)
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
	if constexpr (CVT == CLO_OP_CVT_NONE || CVT == CLO_OP_CVT_ONE32 || CVT == CLO_OP_CVT_ONE64) {
		return rbk_launch<TK, CVT, CLO_OP_SUM>(a);   // (no values: min / max were refused; no aggregate: the op is not used)
	} else {
		switch (op) {
			case CLO_OP_SUM: return rbk_launch<TK, CVT, CLO_OP_SUM>(a);
			case CLO_OP_MIN: return rbk_launch<TK, CVT, CLO_OP_MIN>(a);
			case CLO_OP_MAX: return rbk_launch<TK, CVT, CLO_OP_MAX>(a);
			default: return CLO_HIP_EARGS;
		}
	}
}

template <typename TK>
int rbk_dispatch_cvt(const rbk_args& a, int cvt, int op) {
	switch (cvt) {
		case CLO_OP_CVT_NONE: return rbk_dispatch_op<TK, CLO_OP_CVT_NONE>(a, op);
		case CLO_OP_CVT_32: return rbk_dispatch_op<TK, CLO_OP_CVT_32>(a, op);
		case CLO_OP_CVT_S64: return rbk_dispatch_op<TK, CLO_OP_CVT_S64>(a, op);
		case CLO_OP_CVT_U64: return rbk_dispatch_op<TK, CLO_OP_CVT_U64>(a, op);
		case CLO_OP_CVT_64: return rbk_dispatch_op<TK, CLO_OP_CVT_64>(a, op);
		case CLO_OP_CVT_ONE32: return rbk_dispatch_op<TK, CLO_OP_CVT_ONE32>(a, op);
		case CLO_OP_CVT_ONE64: return rbk_dispatch_op<TK, CLO_OP_CVT_ONE64>(a, op);
		default: return CLO_HIP_EUNSUPPORTED;
	}
}

}  // namespace

extern "C" {

size_t clo_hip_reduce_by_key_tile(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return (size_t) clo_op_seg_rows(key_size, value_size) * RBK_ROW_ELEMS;
}

size_t clo_hip_reduce_by_key_workspace_bytes(size_t numel) { return clo_op_seg_workspace_bytes(numel); }

int clo_hip_reduce_by_key(const void* keys_in, const void* values_in, void* keys_out, void* aggr_out, uint64_t* num_runs_dev,
	size_t numel, int key_size, int value_type, int sum_type, int op, void* workspace, size_t workspace_bytes, void* stream) {
	hipStream_t s = (hipStream_t) stream;
	if (!num_runs_dev || clo_misaligned(num_runs_dev, 8) || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (!keys_out && !aggr_out) return CLO_HIP_EARGS;
	if (op != CLO_OP_SUM && op != CLO_OP_MIN && op != CLO_OP_MAX) return CLO_HIP_EARGS;
	if (aggr_out && !values_in && op != CLO_OP_SUM) return CLO_HIP_EARGS;   // the min / max of ones
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size)) return CLO_HIP_EUNSUPPORTED;
	const int cvt = clo_op_cvt_of(aggr_out != nullptr, values_in != nullptr, value_type, sum_type);
	if (cvt < 0) return CLO_HIP_EUNSUPPORTED;
	if (numel == 0) return (int) hipMemsetAsync(num_runs_dev, 0, sizeof(uint64_t), s);   // no runs, no launch
	if (!keys_in || !workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_reduce_by_key_workspace_bytes(numel)) return CLO_HIP_EWORKSPACE;

	rbk_args a;
	a.keys_in = keys_in; a.values_in = cvt == CLO_OP_CVT_NONE ? nullptr : values_in; a.keys_out = keys_out; a.aggr_out = aggr_out;
	a.num_runs = (unsigned long long*) num_runs_dev; a.n = numel; a.ws = workspace; a.s = s;
	// min / max in a signed sum type: compared as unsigned numbers with the sign bit flipped
	a.flip = (op != CLO_OP_SUM && aggr_out && clo_op_type_signed(sum_type)) ? 1ull << (8 * clo_op_type_size(sum_type) - 1) : 0ull;
	return clo_op_by_key_size(key_size, [&](auto tk) { return rbk_dispatch_cvt<decltype(tk)>(a, cvt, op); });
}

}  // extern "C"
