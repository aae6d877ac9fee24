// clo_hip_segreduce.hip — sum, min and max per segment from counts or from CSR offsets (CloSegReduce,
// include/clo_segreduce.h; not upstream). With m = min(numel_seg, *num_in) segments whose ends are e_r
// (the running sums of the counts, or offsets[r + 1] - offsets[0]) and n rows of values:
//     aggr_out[r] = op over i in [min(e_(r-1), n), min(e_r, n)) of (sum type) values_in[i],     the identity without a row.
//
// The schedule is the merge path of clo_hip_seg_device.h, which has its argument and the bounds of every read: ENDS,
// PARTITION, SWEEP, CARRY, FIXUP. What is this file's:
//   SWEEP      a step that closes a segment ends the open aggregate, a step that takes a row joins it. The lanes' states
//              (closes, open aggregate) go through the segmented scan of the by-key operations. Every segment that closes
//              in the tile is then written: through LDS, as one coalesced stretch aggr_out[a0, a1). The tile leaves
//              (whether a segment closed, the open aggregate at its end, its first closing segment) in the workspace.
//   FIXUP      one thread per tile: the carry into the tile joins the first segment that closes there. (A segment closes
//              in exactly one tile, so no two threads meet.)
// values_in is read once. A lane closes at most na = a1 - a0 segments, so every write lands in aggr_out[a0, a1), a1 <= m.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_seg_device.h"

namespace {

typedef clo_op_u64 seg_u64;

constexpr unsigned SEG_NONE = 0xffffffffu;   // a tile in which no segment closes

// ---- 1. the ends of the counts form: the three launches of clo_hip_seg_device.h ----

template <typename TC>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segreduce_sums_kernel(const TC* __restrict__ counts, const seg_u64* __restrict__ num_in, unsigned m_h, int vec_ok, seg_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segreduce_sums_scan_kernel(seg_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segreduce_ends_kernel(const TC* __restrict__ counts, const seg_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const seg_u64* __restrict__ tsum, seg_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. partition ----
template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segreduce_partition_kernel(const TC* __restrict__ src, const seg_u64* __restrict__ ends, const seg_u64* __restrict__ num_in, unsigned m_h,
	unsigned n, unsigned tiles, unsigned* __restrict__ split, seg_u64* __restrict__ num_out) {
	clo_seg_partition<TC, OFFSETS>(src, ends, num_in, m_h, n, tiles, split, num_out);
}

// numel_seg 0: there is nothing to read
__global__ void clo_segreduce_empty_kernel(seg_u64* __restrict__ num_out) { *num_out = 0ull; }

// ---- 3. tile sweep ----
template <typename TC, bool OFFSETS, int CVT, int OP>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segreduce_sweep_kernel(const TC* __restrict__ src, const seg_u64* __restrict__ ends, const seg_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ split, const typename clo_op_cvt<CVT>::TV* __restrict__ values, typename clo_op_cvt<CVT>::TS* __restrict__ aggr_out,
	typename clo_op_cvt<CVT>::TS flip, unsigned* __restrict__ tile_h, unsigned* __restrict__ tile_first, seg_u64* __restrict__ tile_a) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	// the tile's rows as they lie in memory until the lanes have walked them, then the aggregates of its segments
	__shared__ __attribute__((aligned(16))) TS s_val[CLO_SEG_TILE];
	__shared__ unsigned short s_end[CLO_SEG_TILE];   // positions in [0, nb], nb <= T: 16 bits, so that more groups fit a CU
	__shared__ unsigned s_start[CLO_SEG_THREADS + 1];
	__shared__ unsigned s_h[CLO_SEG_WAVES];
	__shared__ TS s_a[CLO_SEG_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);

	const clo_seg_steps st = clo_seg_tile_steps(m, n);
	if (st.cnt == 0u) {   // the whole work-group: beyond the last step (m < numel_seg)
		if (tid == 0u) { tile_h[blockIdx.x] = 0u; tile_first[blockIdx.x] = SEG_NONE; tile_a[blockIdx.x] = (seg_u64) clo_op_seg_identity<OP, TS>(); }
		return;
	}
	const clo_seg_range g = clo_seg_tile_clamp(st, split, m, n);
	const unsigned a0 = g.a0, na = g.na;

	clo_keyx kx;
	kx.sign = 0; kx.field = 0; kx.kind = 0;   // (not looked at: the rows are staged as they are)
	clo_op_stage<TV, false>(values + g.b0, g.nb, reinterpret_cast<TV*>(s_val), kx, tid);
	if (na > 0u) clo_seg_stage_ends<TC, OFFSETS>(clo_op_ends_make<TC, OFFSETS>(src, ends), g, n, s_end, tid);
	__syncthreads();
	clo_seg_lane l = clo_seg_lane_begin(g, s_end, s_start, tid);
	clo_seg_lane_closes(l, s_end);
	const unsigned b = l.b, steps = l.steps, closes = l.closes;
	// x[k] = the value of the row step k takes, the identity where it takes none: 17 reads that do not wait for each other
	const TV* s_row = reinterpret_cast<const TV*>(s_val);
	TS x[CLO_SEG_ITEMS];
	clo_op_seg_state<TS> s = clo_op_seg_empty<OP, TS>();
	#pragma unroll
	for (int k = 0; k < CLO_SEG_ITEMS; ++k) {
		const bool close = (closes >> k) & 1u;
		const unsigned rs = (unsigned) k - (unsigned) __popc(closes & ((1u << k) - 1u));
		const TV raw = s_row[clo_op_min(b + rs, CLO_SEG_TILE - 1u)];
		const TS v = OP == CLO_OP_SUM ? (TS) raw : (TS) ((TS) raw ^ flip);
		x[k] = (!close && (unsigned) k < steps) ? v : clo_op_seg_identity<OP, TS>();
		s.h += close ? 1u : 0u;
		s.a = close ? clo_op_seg_identity<OP, TS>() : clo_op_seg_op<OP, TS>(s.a, x[k]);
	}

	// the lanes' states through the segmented scan: the lanes, then the waves
	const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, true, TS>(s);
	if (lane == 63u) { s_h[wave] = incl.h; s_a[wave] = incl.a; }
	__syncthreads();   // and every lane has its rows: s_val is free
	clo_op_seg_state<TS> before = clo_op_seg_empty<OP, TS>(), all = clo_op_seg_empty<OP, TS>();
	#pragma unroll
	for (unsigned w = 0; w < (unsigned) CLO_SEG_WAVES; ++w) {
		clo_op_seg_state<TS> p;
		p.h = s_h[w]; p.a = s_a[w];
		if (w < wave) before = clo_op_seg_combine<OP, true, TS>(before, p);
		all = clo_op_seg_combine<OP, true, TS>(all, p);
	}
	const clo_op_seg_state<TS> in = clo_op_seg_combine<OP, true, TS>(before, clo_op_seg_wave_exclusive<OP, true, TS>(incl, lane));
	if (tid == 0u) {
		tile_h[blockIdx.x] = all.h ? 1u : 0u;
		tile_first[blockIdx.x] = na > 0u ? a0 : SEG_NONE;
		tile_a[blockIdx.x] = (seg_u64) all.a;
	}
	if (na == 0u) return;   // the whole work-group

	// the walk again, from registers, with what was open before the lane: a close stores the segment's aggregate
	TS open = in.a;
	unsigned at = l.a;   // a step closes at most ne times, and l.a + ne <= na
	#pragma unroll
	for (int k = 0; k < CLO_SEG_ITEMS; ++k) {
		if ((closes >> k) & 1u) {
			s_val[at] = open;
			++at;
			open = clo_op_seg_identity<OP, TS>();
		} else {
			open = clo_op_seg_op<OP, TS>(open, x[k]);
		}
	}
	__syncthreads();
	clo_op_store<TS>(aggr_out + a0, na, tid, [&](unsigned i) { return OP == CLO_OP_SUM ? s_val[i] : (TS) (s_val[i] ^ flip); });
}

// ---- 4. carry scan: one group; tile t gets the state of the tiles before it, in place ----
template <typename TS, int OP>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segreduce_carry_kernel(unsigned* __restrict__ tile_h, seg_u64* __restrict__ tile_a, unsigned tiles) {
	clo_seg_carry<TS, OP>(tile_h, tile_a, tiles);
}

// ---- 5. fix-up: the carry into tile t joins the first segment that closes there ----
template <typename TS, int OP>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segreduce_fixup_kernel(const unsigned* __restrict__ tile_first, const seg_u64* __restrict__ tile_a, unsigned tiles, unsigned m_h,
	TS* __restrict__ aggr_out, TS flip) {
	const unsigned t = blockIdx.x * CLO_SEG_THREADS + threadIdx.x;
	if (t >= tiles) return;
	const unsigned r = tile_first[t];
	if (r >= m_h) return;   // SEG_NONE, or not a row of aggr_out
	const TS carry = (TS) tile_a[t];
	if constexpr (OP == CLO_OP_SUM) aggr_out[r] = (TS) (aggr_out[r] + carry);
	else aggr_out[r] = (TS) (clo_op_seg_op<OP, TS>(carry, (TS) (aggr_out[r] ^ flip)) ^ flip);
}

// The workspace: the ends of the counts form, the tile boundaries' splits, the tiles' three words, the sums of the ends'
// scan. Laid out from `base`, or only measured where that is null; returns the size.
struct seg_ws { seg_u64* ends; unsigned* split; unsigned* tile_h; unsigned* tile_first; seg_u64* tile_a; seg_u64* tsum; };

inline size_t seg_layout(seg_ws& w, char* base, size_t numel_seg, size_t numel) {
	const size_t tiles = clo_seg_tiles(numel_seg, numel);
	size_t at = 0;
	w.ends = clo_op_ws_take<seg_u64>(base, at, numel_seg);
	w.split = clo_op_ws_take<unsigned>(base, at, tiles + 1);
	w.tile_h = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tile_first = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tile_a = clo_op_ws_take<seg_u64>(base, at, tiles);
	w.tsum = clo_op_ws_take<seg_u64>(base, at, clo_op_ends_tiles(numel_seg) + 1);
	return at;
}

struct seg_args : seg_ws {
	const void* src; const seg_u64* num_in; const void* vin; void* aggr; seg_u64* num_out;
	unsigned m_h, n; seg_u64 flip; hipStream_t s;
};

constexpr const char* SEG_ENDS_LABELS[3] = { "segreduce_sums", "segreduce_sums_scan", "segreduce_ends" };

template <typename TC, bool OFFSETS, int CVT, int OP>
int seg_launch(const seg_args& a) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	if constexpr (!OFFSETS) {
		const int st = clo_op_ends_launch<TC>(clo_segreduce_sums_kernel<TC>, clo_segreduce_sums_scan_kernel, clo_segreduce_ends_kernel<TC>, SEG_ENDS_LABELS,
			a.src, a.num_in, a.m_h, a.tsum, a.ends, a.s);
		if (st != 0) return st;
	}
	const unsigned tiles = (unsigned) clo_seg_tiles(a.m_h, a.n);   // >= 1: m_h > 0
	{
		clo_timing_scope timing("segreduce_partition", a.s);
		hipLaunchKernelGGL((clo_segreduce_partition_kernel<TC, OFFSETS>), dim3(tiles / CLO_SEG_THREADS + 1u), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const seg_u64*) a.ends, a.num_in, a.m_h, a.n, tiles, a.split, a.num_out);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segreduce_sweep", a.s);
		hipLaunchKernelGGL((clo_segreduce_sweep_kernel<TC, OFFSETS, CVT, OP>), dim3(tiles), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const seg_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TV*) a.vin, (TS*) a.aggr, (TS) a.flip,
			a.tile_h, a.tile_first, a.tile_a);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segreduce_carry", a.s);
		hipLaunchKernelGGL((clo_segreduce_carry_kernel<TS, OP>), dim3(1), dim3(CLO_SEG_THREADS), 0, a.s, a.tile_h, a.tile_a, tiles);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segreduce_fixup", a.s);
	hipLaunchKernelGGL((clo_segreduce_fixup_kernel<TS, OP>), dim3((tiles + CLO_SEG_THREADS - 1u) / CLO_SEG_THREADS), dim3(CLO_SEG_THREADS), 0, a.s,
		(const unsigned*) a.tile_first, (const seg_u64*) a.tile_a, tiles, a.m_h, (TS*) a.aggr, (TS) a.flip);
	return (int) hipGetLastError();
}

template <typename TC, bool OFFSETS, int CVT>
int seg_dispatch_op(const seg_args& a, int op) {
	switch (op) {
		case CLO_OP_SUM: return seg_launch<TC, OFFSETS, CVT, CLO_OP_SUM>(a);
		case CLO_OP_MIN: return seg_launch<TC, OFFSETS, CVT, CLO_OP_MIN>(a);
		default: return seg_launch<TC, OFFSETS, CVT, CLO_OP_MAX>(a);
	}
}

template <typename TC, bool OFFSETS>
int seg_dispatch_cvt(const seg_args& a, int cvt, int op) {
	switch (cvt) {
		case CLO_OP_CVT_32: return seg_dispatch_op<TC, OFFSETS, CLO_OP_CVT_32>(a, op);
		case CLO_OP_CVT_S64: return seg_dispatch_op<TC, OFFSETS, CLO_OP_CVT_S64>(a, op);
		case CLO_OP_CVT_U64: return seg_dispatch_op<TC, OFFSETS, CLO_OP_CVT_U64>(a, op);
		case CLO_OP_CVT_64: return seg_dispatch_op<TC, OFFSETS, CLO_OP_CVT_64>(a, op);
		default: return CLO_HIP_EUNSUPPORTED;
	}
}

template <typename TC>
int seg_dispatch(const seg_args& a, int form, int cvt, int op) {
	return form == CLO_HIP_SEGREDUCE_OFFSETS ? seg_dispatch_cvt<TC, true>(a, cvt, op) : seg_dispatch_cvt<TC, false>(a, cvt, op);
}

}  // namespace

extern "C" {

size_t clo_hip_segreduce_tile(int value_size, int sum_size) {
	return (value_size == 4 || value_size == 8) && (sum_size == 4 || sum_size == 8) && sum_size >= value_size ? CLO_SEG_TILE : 0;
}

size_t clo_hip_segreduce_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	seg_ws w;
	return seg_layout(w, nullptr, numel_seg, numel);
}

int clo_hip_segreduce(int op, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* aggr_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (op != CLO_OP_SUM && op != CLO_OP_MIN && op != CLO_OP_MAX) return CLO_HIP_EARGS;
	if (form != CLO_HIP_SEGREDUCE_COUNTS && form != CLO_HIP_SEGREDUCE_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int cvt = clo_op_cvt_of(true, true, value_type, sum_type);
	if (cvt < 0) return CLO_HIP_EUNSUPPORTED;
	const size_t vs = (size_t) clo_op_type_size(value_type), ss = (size_t) clo_op_type_size(sum_type);
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGREDUCE_OFFSETS)) return CLO_HIP_EARGS;
	if (!values_in && numel > 0) return CLO_HIP_EARGS;
	if (!aggr_out && numel_seg > 0) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8) || clo_misaligned(num_in, 8)) return CLO_HIP_EARGS;
	if (clo_misaligned(counts_or_offsets, (size_t) count_size) || clo_misaligned(values_in, vs) || clo_misaligned(aggr_out, ss)) return CLO_HIP_EARGS;
	if (numel_seg == 0) {
		hipLaunchKernelGGL(clo_segreduce_empty_kernel, dim3(1), dim3(1), 0, (hipStream_t) stream, (seg_u64*) num_out);
		return (int) hipGetLastError();
	}
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_segreduce_workspace_bytes(numel_seg, numel)) return CLO_HIP_EWORKSPACE;

	seg_args a;
	a.src = counts_or_offsets; a.num_in = (const seg_u64*) num_in; a.vin = values_in; a.aggr = aggr_out; a.num_out = (seg_u64*) num_out;
	a.m_h = (unsigned) numel_seg; a.n = (unsigned) numel; a.s = (hipStream_t) stream;
	// min / max in a signed sum type: compared as unsigned numbers with the sign bit flipped
	a.flip = (op != CLO_OP_SUM && clo_op_type_signed(sum_type)) ? 1ull << (8 * ss - 1) : 0ull;
	seg_layout(a, (char*) workspace, numel_seg, numel);
	return count_size == 8 ? seg_dispatch<uint64_t>(a, form, cvt, op) : seg_dispatch<uint32_t>(a, form, cvt, op);
}

}  // extern "C"
