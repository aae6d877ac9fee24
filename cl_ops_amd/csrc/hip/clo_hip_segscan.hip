// clo_hip_segscan.hip — running sum, min and max within segments given by counts or by CSR offsets (CloSegScan,
// include/clo_segscan.h; not upstream). With m = min(numel_seg, *num_in) segments whose ends are e_r (the
// running sums of the counts, or offsets[r + 1] - offsets[0]), n rows of values and ct = min(e_(m-1), n): every row i < ct
// lies in one clipped segment, whose first row is b(i), and
//     data_out[i] = op over j in [b(i), i] (inclusive) or [b(i), i) (exclusive) of (sum type) values_in[j].
//
// The schedule is the merge path of clo_hip_seg_device.h, which has its argument and the bounds of every read: ENDS,
// PARTITION, TAILS, CARRY, SWEEP. A step that closes a segment starts what is open again from the identity. What is this
// file's:
//   TAILS      one work-group per tile: the tile's state, (does a segment close here, the op over the rows it takes after
//              its last close). The last close is ONE clipped end, so the rows are [c, b0 + nb) with c clamped into the
//              tile's rows: the whole tile where nothing closes, a few rows where the segments are short. No merge.
//   SWEEP      after CARRY, so that the lanes' states go through the segmented scan of the by-key operations starting from
//              the tile's carry. Every lane then walks its steps again from registers and puts the running value of each
//              ROW (before or after the row, by kind) into LDS at the row's position; the tile leaves as one coalesced
//              stretch data_out[b0, min(b0 + nb, ct)).
// values_in is read once, plus the open tails. In place (data_out == values_in, equal widths): TAILS completes before
// SWEEP on the stream, and a group of SWEEP stages its rows before it stores the same rows; no group reads another's.
// The store is count min(nb, ct - b0) from b0, so it stays in data_out[0, n).
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_seg_device.h"

namespace {

typedef clo_op_u64 sscan_u64;

// ---- 1. the ends of the counts form: the three launches of clo_hip_seg_device.h ----

template <typename TC>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segscan_sums_kernel(const TC* __restrict__ counts, const sscan_u64* __restrict__ num_in, unsigned m_h, int vec_ok, sscan_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segscan_sums_scan_kernel(sscan_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segscan_ends_kernel(const TC* __restrict__ counts, const sscan_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const sscan_u64* __restrict__ tsum, sscan_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. partition ----
template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segscan_partition_kernel(const TC* __restrict__ src, const sscan_u64* __restrict__ ends, const sscan_u64* __restrict__ num_in, unsigned m_h,
	unsigned n, unsigned tiles, unsigned* __restrict__ split, sscan_u64* __restrict__ num_out) {
	clo_seg_partition<TC, OFFSETS>(src, ends, num_in, m_h, n, tiles, split, num_out);
}

// numel_seg 0: there is nothing to read
__global__ void clo_segscan_empty_kernel(sscan_u64* __restrict__ num_out) { *num_out = 0ull; }

// (sum type) value, for min and max with the sign bit of a signed sum type flipped: compared as unsigned numbers
template <int CVT, int OP>
__device__ __forceinline__ typename clo_op_cvt<CVT>::TS sscan_value(typename clo_op_cvt<CVT>::TV raw, typename clo_op_cvt<CVT>::TS flip) {
	typedef typename clo_op_cvt<CVT>::TS TS;
	return OP == CLO_OP_SUM ? (TS) raw : (TS) ((TS) raw ^ flip);
}

// ---- 3. tails: the state of every tile ----
template <typename TC, bool OFFSETS, int CVT, int OP>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segscan_tails_kernel(const TC* __restrict__ src, const sscan_u64* __restrict__ ends, const sscan_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ split, const typename clo_op_cvt<CVT>::TV* __restrict__ values, typename clo_op_cvt<CVT>::TS flip,
	unsigned* __restrict__ tile_h, sscan_u64* __restrict__ tile_a) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	__shared__ TS s_a[CLO_SEG_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_seg_range g = clo_seg_tile_range(split, m, n);
	if (g.cnt == 0u) {   // the whole work-group
		if (tid == 0u) { tile_h[blockIdx.x] = 0u; tile_a[blockIdx.x] = (sscan_u64) clo_op_seg_identity<OP, TS>(); }
		return;
	}
	// the rows after the tile's last close: [c, b0 + nb), c the last closing end clipped and clamped into the tile's rows
	sscan_u64 c = g.b0;
	if (g.na > 0u) {
		const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
		const sscan_u64 last = clo_op_min64(e.at(g.a0 + g.na - 1u), n);   // a0 + na - 1 < m
		c = clo_op_min64(clo_op_max64(last, g.b0), g.b0 + g.nb);
	}
	const TV* __restrict__ p = values + c;
	const unsigned count = (unsigned) (g.b0 + g.nb - c);   // <= nb <= T, and c + count <= n
	TS acc = clo_op_seg_identity<OP, TS>();
	{   // clo_op_stage's division: 16-byte loads from p's first 16-byte boundary on
		constexpr unsigned PER = 16u / sizeof(TV);
		typedef TV vec __attribute__((ext_vector_type(PER)));
		const unsigned head = clo_op_min((unsigned) ((16u - ((uintptr_t) p & 15u)) & 15u) / (unsigned) sizeof(TV), count);
		const unsigned nvec = (count - head) / PER, body_end = head + nvec * PER;
		for (unsigned v = tid; v < nvec; v += CLO_SEG_THREADS) {
			const vec x = *reinterpret_cast<const vec*>(p + head + v * PER);
			#pragma unroll
			for (unsigned k = 0; k < PER; ++k) acc = clo_op_seg_op<OP, TS>(acc, sscan_value<CVT, OP>(x[k], flip));
		}
		const unsigned rest = head + (count - body_end);   // fewer than 2 PER <= 32 elements
		if (tid < rest) {
			const unsigned i = tid < head ? tid : body_end + (tid - head);
			acc = clo_op_seg_op<OP, TS>(acc, sscan_value<CVT, OP>(p[i], flip));
		}
	}
	clo_op_seg_state<TS> s;
	s.h = 0u; s.a = acc;   // no heads: the segmented scan is the plain one, lane 63 holds the wave's aggregate
	const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, true, TS>(s);
	if (lane == 63u) s_a[wave] = incl.a;
	__syncthreads();
	if (tid == 0u) {
		TS all = s_a[0];
		#pragma unroll
		for (int w = 1; w < CLO_SEG_WAVES; ++w) all = clo_op_seg_op<OP, TS>(all, s_a[w]);
		tile_h[blockIdx.x] = g.na > 0u ? 1u : 0u;
		tile_a[blockIdx.x] = (sscan_u64) all;
	}
}

// ---- 4. carry scan: one group; tile t gets the state of the tiles before it, in place ----
template <typename TS, int OP>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segscan_carry_kernel(const unsigned* __restrict__ tile_h, sscan_u64* __restrict__ tile_a, unsigned tiles) {
	clo_seg_carry<TS, OP>(tile_h, tile_a, tiles);
}

// ---- 5. tile sweep ----
// values and data_out may be the same array (in place): neither is __restrict__.
template <typename TC, bool OFFSETS, int CVT, int OP, bool INCL>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segscan_sweep_kernel(const TC* __restrict__ src, const sscan_u64* __restrict__ ends, const sscan_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ split, const typename clo_op_cvt<CVT>::TV* values, typename clo_op_cvt<CVT>::TS* data_out,
	typename clo_op_cvt<CVT>::TS flip, const sscan_u64* __restrict__ tile_a) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	// the tile's rows as they lie in memory until the lanes have walked them, then the rows' results
	__shared__ __attribute__((aligned(16))) TS s_val[CLO_SEG_TILE];
	__shared__ unsigned short s_end[CLO_SEG_TILE];   // positions in [0, nb], nb <= T: 16 bits, so that more groups fit a CU
	__shared__ unsigned s_start[CLO_SEG_THREADS + 1];
	__shared__ unsigned s_h[CLO_SEG_WAVES];
	__shared__ TS s_a[CLO_SEG_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_seg_range g = clo_seg_tile_range(split, m, n);
	if (g.cnt == 0u || g.nb == 0u) return;   // the whole work-group: beyond the last step, or no row to write
	const unsigned nb = g.nb;
	const sscan_u64 b0 = g.b0;
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	// rows at and beyond ct = min(e_(m-1), n) are not written
	const sscan_u64 ct = m > 0u ? clo_op_min64(e.at(m - 1u), n) : 0ull;
	const unsigned nstore = (unsigned) (clo_op_max64(clo_op_min64(b0 + nb, ct), b0) - b0);   // the tile's rows below ct: [b0, that end)
	if (nstore == 0u) return;   // the whole work-group
	const TS carry = (TS) tile_a[blockIdx.x];

	clo_keyx kx;
	kx.sign = 0; kx.field = 0; kx.kind = 0;   // (not looked at: the rows are staged as they are)
	clo_op_stage<TV, false>(values + b0, nb, reinterpret_cast<TV*>(s_val), kx, tid);
	clo_seg_stage_ends<TC, OFFSETS>(e, g, n, s_end, tid);
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
		x[k] = (!close && (unsigned) k < steps) ? sscan_value<CVT, OP>(raw, flip) : clo_op_seg_identity<OP, TS>();
		s.h += close ? 1u : 0u;
		s.a = close ? clo_op_seg_identity<OP, TS>() : clo_op_seg_op<OP, TS>(s.a, x[k]);
	}

	// the lanes' states through the segmented scan: the lanes, then the waves, then the tile's carry
	const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, true, TS>(s);
	if (lane == 63u) { s_h[wave] = incl.h; s_a[wave] = incl.a; }
	__syncthreads();   // and every lane has its rows: s_val is free
	clo_op_seg_state<TS> before;
	before.h = 0u; before.a = carry;
	#pragma unroll
	for (unsigned w = 0; w < (unsigned) CLO_SEG_WAVES; ++w) {
		clo_op_seg_state<TS> p;
		p.h = s_h[w]; p.a = s_a[w];
		if (w < wave) before = clo_op_seg_combine<OP, true, TS>(before, p);
	}
	const clo_op_seg_state<TS> in = clo_op_seg_combine<OP, true, TS>(before, clo_op_seg_wave_exclusive<OP, true, TS>(incl, lane));

	// the walk again, from registers, with what was open before the lane: every row leaves its running value at its
	// position (clamped below T: a lane whose ends do not ascend may count more rows than it has)
	TS open = in.a;
	unsigned at = b;
	#pragma unroll
	for (int k = 0; k < CLO_SEG_ITEMS; ++k) {
		if ((closes >> k) & 1u) {
			open = clo_op_seg_identity<OP, TS>();
		} else if ((unsigned) k < steps) {
			const TS after = clo_op_seg_op<OP, TS>(open, x[k]);
			s_val[clo_op_min(at, CLO_SEG_TILE - 1u)] = INCL ? after : open;
			open = after;
			++at;
		}
	}
	__syncthreads();
	clo_op_store<TS>(data_out + b0, nstore, tid, [&](unsigned i) { return OP == CLO_OP_SUM ? s_val[i] : (TS) (s_val[i] ^ flip); });
}

// The workspace: the ends of the counts form, the tile boundaries' splits, the tiles' two words, the sums of the ends'
// scan. Laid out from `base`, or only measured where that is null; returns the size.
struct sscan_ws { sscan_u64* ends; unsigned* split; unsigned* tile_h; sscan_u64* tile_a; sscan_u64* tsum; };

inline size_t sscan_layout(sscan_ws& w, char* base, size_t numel_seg, size_t numel) {
	const size_t tiles = clo_seg_tiles(numel_seg, numel);
	size_t at = 0;
	w.ends = clo_op_ws_take<sscan_u64>(base, at, numel_seg);
	w.split = clo_op_ws_take<unsigned>(base, at, tiles + 1);
	w.tile_h = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tile_a = clo_op_ws_take<sscan_u64>(base, at, tiles);
	w.tsum = clo_op_ws_take<sscan_u64>(base, at, clo_op_ends_tiles(numel_seg) + 1);
	return at;
}

struct sscan_args : sscan_ws {
	const void* src; const sscan_u64* num_in; const void* vin; void* out; sscan_u64* num_out;
	unsigned m_h, n; sscan_u64 flip; hipStream_t s;
};

constexpr const char* SCAN_ENDS_LABELS[3] = { "segscan_sums", "segscan_sums_scan", "segscan_ends" };

// the launches every kind shares: ends, partition, tails, carry
template <typename TC, bool OFFSETS, int CVT, int OP>
int sscan_launch_states(const sscan_args& a, unsigned tiles) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	if constexpr (!OFFSETS) {
		const int st = clo_op_ends_launch<TC>(clo_segscan_sums_kernel<TC>, clo_segscan_sums_scan_kernel, clo_segscan_ends_kernel<TC>, SCAN_ENDS_LABELS,
			a.src, a.num_in, a.m_h, a.tsum, a.ends, a.s);
		if (st != 0) return st;
	}
	{
		clo_timing_scope timing("segscan_partition", a.s);
		hipLaunchKernelGGL((clo_segscan_partition_kernel<TC, OFFSETS>), dim3(tiles / CLO_SEG_THREADS + 1u), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const sscan_u64*) a.ends, a.num_in, a.m_h, a.n, tiles, a.split, a.num_out);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	if (a.n == 0u) return 0;   // no row: num_out is all there is to write
	{
		clo_timing_scope timing("segscan_tails", a.s);
		hipLaunchKernelGGL((clo_segscan_tails_kernel<TC, OFFSETS, CVT, OP>), dim3(tiles), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const sscan_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TV*) a.vin, (TS) a.flip, a.tile_h, a.tile_a);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segscan_carry", a.s);
	hipLaunchKernelGGL((clo_segscan_carry_kernel<TS, OP>), dim3(1), dim3(CLO_SEG_THREADS), 0, a.s, (const unsigned*) a.tile_h, a.tile_a, tiles);
	return (int) hipGetLastError();
}

template <typename TC, bool OFFSETS, int CVT, int OP>
int sscan_launch(const sscan_args& a, int inclusive) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	const unsigned tiles = (unsigned) clo_seg_tiles(a.m_h, a.n);   // >= 1: m_h > 0
	const int st = sscan_launch_states<TC, OFFSETS, CVT, OP>(a, tiles);
	if (st != 0 || a.n == 0u) return st;
	clo_timing_scope timing("segscan_sweep", a.s);
	if (inclusive)
		hipLaunchKernelGGL((clo_segscan_sweep_kernel<TC, OFFSETS, CVT, OP, true>), dim3(tiles), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const sscan_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TV*) a.vin, (TS*) a.out, (TS) a.flip,
			(const sscan_u64*) a.tile_a);
	else
		hipLaunchKernelGGL((clo_segscan_sweep_kernel<TC, OFFSETS, CVT, OP, false>), dim3(tiles), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const sscan_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TV*) a.vin, (TS*) a.out, (TS) a.flip,
			(const sscan_u64*) a.tile_a);
	return (int) hipGetLastError();
}

template <typename TC, bool OFFSETS, int CVT>
int sscan_dispatch_op(const sscan_args& a, int op, int inclusive) {
	switch (op) {
		case CLO_OP_SUM: return sscan_launch<TC, OFFSETS, CVT, CLO_OP_SUM>(a, inclusive);
		case CLO_OP_MIN: return sscan_launch<TC, OFFSETS, CVT, CLO_OP_MIN>(a, inclusive);
		default: return sscan_launch<TC, OFFSETS, CVT, CLO_OP_MAX>(a, inclusive);
	}
}

template <typename TC, bool OFFSETS>
int sscan_dispatch_cvt(const sscan_args& a, int cvt, int op, int inclusive) {
	switch (cvt) {
		case CLO_OP_CVT_32: return sscan_dispatch_op<TC, OFFSETS, CLO_OP_CVT_32>(a, op, inclusive);
		case CLO_OP_CVT_S64: return sscan_dispatch_op<TC, OFFSETS, CLO_OP_CVT_S64>(a, op, inclusive);
		case CLO_OP_CVT_U64: return sscan_dispatch_op<TC, OFFSETS, CLO_OP_CVT_U64>(a, op, inclusive);
		case CLO_OP_CVT_64: return sscan_dispatch_op<TC, OFFSETS, CLO_OP_CVT_64>(a, op, inclusive);
		default: return CLO_HIP_EUNSUPPORTED;
	}
}

template <typename TC>
int sscan_dispatch(const sscan_args& a, int form, int cvt, int op, int inclusive) {
	return form == CLO_HIP_SEGSCAN_OFFSETS ? sscan_dispatch_cvt<TC, true>(a, cvt, op, inclusive) : sscan_dispatch_cvt<TC, false>(a, cvt, op, inclusive);
}

}  // namespace

extern "C" {

size_t clo_hip_segscan_tile(int value_size, int sum_size) {
	return (value_size == 4 || value_size == 8) && (sum_size == 4 || sum_size == 8) && sum_size >= value_size ? CLO_SEG_TILE : 0;
}

size_t clo_hip_segscan_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	sscan_ws w;
	return sscan_layout(w, nullptr, numel_seg, numel);
}

int clo_hip_segscan(int op, int inclusive, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* data_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (op != CLO_OP_SUM && op != CLO_OP_MIN && op != CLO_OP_MAX) return CLO_HIP_EARGS;
	if (inclusive != 0 && inclusive != 1) return CLO_HIP_EARGS;
	if (form != CLO_HIP_SEGSCAN_COUNTS && form != CLO_HIP_SEGSCAN_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int cvt = clo_op_cvt_of(true, true, value_type, sum_type);
	if (cvt < 0) return CLO_HIP_EUNSUPPORTED;
	const size_t vs = (size_t) clo_op_type_size(value_type), ss = (size_t) clo_op_type_size(sum_type);
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGSCAN_OFFSETS)) return CLO_HIP_EARGS;
	if ((!values_in || !data_out) && numel > 0) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8) || clo_misaligned(num_in, 8)) return CLO_HIP_EARGS;
	if (clo_misaligned(counts_or_offsets, (size_t) count_size) || clo_misaligned(values_in, vs) || clo_misaligned(data_out, ss)) return CLO_HIP_EARGS;
	if (numel_seg == 0) {
		hipLaunchKernelGGL(clo_segscan_empty_kernel, dim3(1), dim3(1), 0, (hipStream_t) stream, (sscan_u64*) num_out);
		return (int) hipGetLastError();
	}
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_segscan_workspace_bytes(numel_seg, numel)) return CLO_HIP_EWORKSPACE;

	sscan_args a;
	a.src = counts_or_offsets; a.num_in = (const sscan_u64*) num_in; a.vin = values_in; a.out = data_out; a.num_out = (sscan_u64*) num_out;
	a.m_h = (unsigned) numel_seg; a.n = (unsigned) numel; a.s = (hipStream_t) stream;
	// min / max in a signed sum type: compared as unsigned numbers with the sign bit flipped
	a.flip = (op != CLO_OP_SUM && clo_op_type_signed(sum_type)) ? 1ull << (8 * ss - 1) : 0ull;
	sscan_layout(a, (char*) workspace, numel_seg, numel);
	return count_size == 8 ? sscan_dispatch<uint64_t>(a, form, cvt, op, inclusive) : sscan_dispatch<uint32_t>(a, form, cvt, op, inclusive);
}

}  // extern "C"
