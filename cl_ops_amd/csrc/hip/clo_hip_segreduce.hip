// clo_hip_segreduce.hip — sum, min and max per segment from counts or from CSR offsets (CloSegReduce,
// include/clo_segreduce.h; not upstream). With m = min(numel_seg, *num_in) segments whose ends are e_r
// (the running sums of the counts, or offsets[r + 1] - offsets[0]) and n rows of values:
//     aggr_out[r] = op over i in [min(e_(r-1), n), min(e_r, n)) of (sum type) values_in[i],     the identity without a row.
//
// The schedule is the merge path of Merrill & Garland's merge-based SpMV: the m clipped ends c_r = min(e_r, n) are
// merged with the row indices 0 .. n - 1, an end going first when c_r <= j. A step of the merge either CLOSES segment r
// (its aggregate is complete) or takes row j into the open aggregate; a tile is T steps, whatever they are, so that a
// work-group's work does not depend on how the ends are spread. None of the launches waits for another work-group, none
// uses a global atomic:
//   ENDS       the counts form only: the numel_seg inclusive ends as uint64 in the workspace (the three launches CloExpand
//              has, clo_hip_op_device.h). The offsets form is read where it lies.
//   PARTITION  one thread per tile boundary d = t * T: split[t] = how many of the first d steps close a segment, by a
//              halving over the ends; thread 0 writes num_out = e_(m-1).
//   SWEEP      one work-group per tile. The split is CLAMPED to what d, m and n alone allow (clo_op_tile_range's rule, in
//              64 bits: m + n may pass 2^32). The tile's rows are staged in LDS by 16-byte loads, its ends as positions
//              relative to the tile's first row. A lane finds where its 17 steps begin by a halving in LDS and learns
//              from the next lane's beginning how many of them close a segment; end a + j of the lane then closes at step
//              j + (the lane's rows before it), so the steps are known as a bit mask without walking them, and the 17
//              LDS reads of ends and the 17 of rows do not wait for each other. The lanes' states (closes, open
//              aggregate) go through the segmented scan of the by-key operations. Every segment that closes in the tile is then written: through LDS, as one coalesced
//              stretch aggr_out[a0, a1). The tile leaves (whether a segment closed, the open aggregate at its end, its
//              first closing segment) in the workspace.
//   CARRY      one work-group: the exclusive segmented scan of the tiles' states, SEG_CARRY_TRIP tiles per trip.
//   FIXUP      one thread per tile: the carry into the tile joins the first segment that closes there. (A segment closes
//              in exactly one tile, so no two threads meet.)
// values_in is read once. Whatever the arrays hold: the halvings are loops over [lo, hi) that shrink every trip; ends are
// loaded at indices below m only; a tile's rows are [b0, b0 + nb) with b0 + nb <= n by the clamp; an end's position is
// clamped to [0, nb]; a lane closes at most na = a1 - a0 segments, so every write lands in aggr_out[a0, a1), a1 <= m.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

typedef clo_op_u64 seg_u64;

constexpr int SEG_THREADS = 256;
constexpr int SEG_WAVES = SEG_THREADS / 64;
static_assert(SEG_THREADS == CLO_OP_THREADS, "the shared helpers stride by CLO_OP_THREADS");
constexpr int SEG_ITEMS = 17;                                   // merge steps per lane: odd, so that the lanes' LDS reads spread over the banks
constexpr unsigned SEG_TILE = SEG_THREADS * SEG_ITEMS;          // T = 4352 merge steps, for every type
static_assert(SEG_TILE < 65536u, "an end's position in its tile is kept in 16 bits");
constexpr unsigned SEG_NONE = 0xffffffffu;                      // a tile in which no segment closes
constexpr int SEG_CARRY_ITEMS = 16;
static_assert(SEG_CARRY_ITEMS % 4 == 0, "a thread's states are loaded four and two at a time");
constexpr unsigned SEG_CARRY_TRIP = SEG_THREADS * SEG_CARRY_ITEMS;   // tile states per trip of the one-group scan

inline size_t seg_tiles(size_t numel_seg, size_t numel) { return (numel_seg + numel + SEG_TILE - 1) / SEG_TILE; }

__device__ __forceinline__ seg_u64 seg_min64(seg_u64 a, seg_u64 b) { return a < b ? a : b; }
__device__ __forceinline__ seg_u64 seg_max64(seg_u64 a, seg_u64 b) { return a > b ? a : b; }

// ---- 1. the ends of the counts form: the three launches of clo_hip_op_device.h ----

template <typename TC>
__global__ __launch_bounds__(SEG_THREADS)
void clo_segreduce_sums_kernel(const TC* __restrict__ counts, const seg_u64* __restrict__ num_in, unsigned m_h, int vec_ok, seg_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(SEG_THREADS)
void clo_segreduce_sums_scan_kernel(seg_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(SEG_THREADS)
void clo_segreduce_ends_kernel(const TC* __restrict__ counts, const seg_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const seg_u64* __restrict__ tsum, seg_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. partition ----
// split[t] = how many of the first d = min(t * T, m + n) merge steps close a segment; in [max(0, d - n), min(d, m)].
template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(SEG_THREADS)
void clo_segreduce_partition_kernel(const TC* __restrict__ src, const seg_u64* __restrict__ ends, const seg_u64* __restrict__ num_in, unsigned m_h,
	unsigned n, unsigned tiles, unsigned* __restrict__ split, seg_u64* __restrict__ num_out) {
	const unsigned t = blockIdx.x * SEG_THREADS + threadIdx.x;
	if (t > tiles) return;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	const seg_u64 d = seg_min64((seg_u64) t * SEG_TILE, (seg_u64) m + n);
	unsigned lo = d > n ? (unsigned) (d - n) : 0u, hi = (unsigned) seg_min64(d, m);
	while (lo < hi) {   // at most 32 trips: hi - lo halves
		const unsigned mid = lo + ((hi - lo) >> 1);   // < hi <= m
		const seg_u64 c = seg_min64(e.at(mid), n);
		if (c <= d - 1u - mid) lo = mid + 1u; else hi = mid;
	}
	split[t] = lo;
	if (t == 0) *num_out = m > 0u ? e.at(m - 1u) : 0ull;
}

// numel_seg 0: there is nothing to read
__global__ void clo_segreduce_empty_kernel(seg_u64* __restrict__ num_out) { *num_out = 0ull; }

// ---- 3. tile sweep ----
template <typename TC, bool OFFSETS, int CVT, int OP>
__global__ __launch_bounds__(SEG_THREADS)
void clo_segreduce_sweep_kernel(const TC* __restrict__ src, const seg_u64* __restrict__ ends, const seg_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ split, const typename clo_op_cvt<CVT>::TV* __restrict__ values, typename clo_op_cvt<CVT>::TS* __restrict__ aggr_out,
	typename clo_op_cvt<CVT>::TS flip, unsigned* __restrict__ tile_h, unsigned* __restrict__ tile_first, seg_u64* __restrict__ tile_a) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	// the tile's rows as they lie in memory until the lanes have walked them, then the aggregates of its segments
	__shared__ __attribute__((aligned(16))) TS s_val[SEG_TILE];
	__shared__ unsigned short s_end[SEG_TILE];   // positions in [0, nb], nb <= T: 16 bits, so that more groups fit a CU
	__shared__ unsigned s_start[SEG_THREADS + 1];
	__shared__ unsigned s_h[SEG_WAVES];
	__shared__ TS s_a[SEG_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);

	// the tile's steps [d0, d1), of which [a0, a1) close segments and the rest take rows [b0, b0 + nb): the split clamped
	const seg_u64 total = (seg_u64) m + n, dd0 = (seg_u64) blockIdx.x * SEG_TILE;
	const seg_u64 d0 = seg_min64(dd0, total), d1 = seg_min64(dd0 + SEG_TILE, total);
	const unsigned cnt = (unsigned) (d1 - d0);
	if (cnt == 0u) {   // the whole work-group: beyond the last step (m < numel_seg)
		if (tid == 0u) { tile_h[blockIdx.x] = 0u; tile_first[blockIdx.x] = SEG_NONE; tile_a[blockIdx.x] = (seg_u64) clo_op_seg_identity<OP, TS>(); }
		return;
	}
	seg_u64 a0w = split[blockIdx.x], a1w = split[blockIdx.x + 1u];
	a0w = seg_min64(seg_max64(a0w, d0 > n ? d0 - n : 0ull), seg_min64(d0, m));
	a1w = seg_min64(seg_max64(a1w, seg_max64(a0w, d1 > n ? d1 - n : 0ull)), seg_min64(m, a0w + cnt));
	const unsigned a0 = (unsigned) a0w, na = (unsigned) (a1w - a0w), nb = cnt - na;
	const seg_u64 b0 = d0 - a0w;   // b0 + nb = d1 - a1 <= n

	clo_keyx kx;
	kx.sign = 0; kx.field = 0; kx.kind = 0;   // (not looked at: the rows are staged as they are)
	clo_op_stage<TV, false>(values + b0, nb, reinterpret_cast<TV*>(s_val), kx, tid);
	if (na > 0u) {
		const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
		for (unsigned k = tid; k < na; k += SEG_THREADS) {
			const seg_u64 c = seg_min64(e.at(a0 + k), n);   // a0 + k < a1 <= m
			s_end[k] = (unsigned short) (c < b0 ? 0u : (unsigned) seg_min64(c - b0, nb));
		}
	}
	__syncthreads();

	// where this lane's steps begin: of the first d steps of the tile, `a` close a segment
	const unsigned d = clo_op_min(tid * SEG_ITEMS, cnt);
	unsigned a, b;
	{
		unsigned lo = d > nb ? d - nb : 0u, hi = clo_op_min(d, na);
		while (lo < hi) {
			const unsigned mid = lo + ((hi - lo) >> 1);
			if (s_end[mid] <= d - 1u - mid) lo = mid + 1u; else hi = mid;
		}
		a = lo; b = d - lo;
	}
	const unsigned a_lane = a;
	// what the lane's steps are is known without walking them: it closes the ends [a, the next lane's a) and takes the
	// rows between them, and end a + j closes at step j + (the lane's rows before it), whatever the other ends are
	s_start[tid] = a;
	if (tid == 0u) s_start[SEG_THREADS] = na;
	__syncthreads();
	const unsigned steps = clo_op_min((unsigned) SEG_ITEMS, cnt - d);
	const unsigned ne = clo_op_min(clo_op_max(s_start[tid + 1u], a) - a, steps);
	const unsigned nr = steps - ne;   // its rows [b, b + nr); b + nr <= nb
	unsigned closes = 0u;             // bit k = step k closes a segment
	#pragma unroll
	for (int j = 0; j < SEG_ITEMS; ++j) {
		const unsigned ea = s_end[clo_op_min(a + (unsigned) j, SEG_TILE - 1u)];
		const unsigned p = clo_op_min(ea > b ? ea - b : 0u, nr) + (unsigned) j;   // < steps where j < ne
		closes |= ((unsigned) j < ne ? 1u : 0u) << (p & 31u);
	}
	// x[k] = the value of the row step k takes, the identity where it takes none: 17 reads that do not wait for each other
	const TV* s_row = reinterpret_cast<const TV*>(s_val);
	TS x[SEG_ITEMS];
	clo_op_seg_state<TS> s = clo_op_seg_empty<OP, TS>();
	#pragma unroll
	for (int k = 0; k < SEG_ITEMS; ++k) {
		const bool close = (closes >> k) & 1u;
		const unsigned rs = (unsigned) k - (unsigned) __popc(closes & ((1u << k) - 1u));
		const TV raw = s_row[clo_op_min(b + rs, SEG_TILE - 1u)];
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
	for (unsigned w = 0; w < (unsigned) SEG_WAVES; ++w) {
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
	unsigned at = a_lane;   // a step closes at most ne times, and a_lane + ne <= na
	#pragma unroll
	for (int k = 0; k < SEG_ITEMS; ++k) {
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

// ---- 4. carry scan: one group; tile t gets the state of the tiles before it, in place (clo_rbk_states_kernel's walk,
// SEG_CARRY_TRIP states per trip) ----
template <typename TS, int OP>
__global__ __launch_bounds__(SEG_THREADS)
void clo_segreduce_carry_kernel(unsigned* __restrict__ tile_h, seg_u64* __restrict__ tile_a, unsigned tiles) {
	__shared__ unsigned s_h[SEG_WAVES];
	__shared__ TS s_a[SEG_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	clo_op_seg_state<TS> running = clo_op_seg_empty<OP, TS>();   // the state of everything before this trip (the same in every thread)
	// the next trip's states are requested before this trip's are combined
	clo_op_seg_state<TS> ahead[SEG_CARRY_ITEMS];
	typedef unsigned vec4 __attribute__((ext_vector_type(4)));
	typedef seg_u64 vec2 __attribute__((ext_vector_type(2)));
	auto request = [&](unsigned first) {
		if (first + SEG_CARRY_ITEMS <= tiles) {   // 16-byte loads: the arrays are 256-byte aligned, `first` a multiple of SEG_CARRY_ITEMS
			#pragma unroll
			for (int j = 0; j < SEG_CARRY_ITEMS; j += 4) {
				const vec4 h = *reinterpret_cast<const vec4*>(tile_h + first + j);
				ahead[j].h = h.x; ahead[j + 1].h = h.y; ahead[j + 2].h = h.z; ahead[j + 3].h = h.w;
			}
			#pragma unroll
			for (int j = 0; j < SEG_CARRY_ITEMS; j += 2) {
				const vec2 a = *reinterpret_cast<const vec2*>(tile_a + first + j);
				ahead[j].a = (TS) a.x; ahead[j + 1].a = (TS) a.y;
			}
		} else {
			#pragma unroll
			for (int j = 0; j < SEG_CARRY_ITEMS; ++j) {
				ahead[j] = clo_op_seg_empty<OP, TS>();
				if (first + j < tiles) { ahead[j].h = tile_h[first + j]; ahead[j].a = (TS) tile_a[first + j]; }
			}
		}
	};
	request(tid * SEG_CARRY_ITEMS);
	for (unsigned chunk = 0; chunk < tiles; chunk += SEG_CARRY_TRIP) {
		const unsigned t0 = chunk + tid * SEG_CARRY_ITEMS;
		clo_op_seg_state<TS> st[SEG_CARRY_ITEMS];
		clo_op_seg_state<TS> mine = clo_op_seg_empty<OP, TS>();
		#pragma unroll
		for (int j = 0; j < SEG_CARRY_ITEMS; ++j) {
			st[j] = ahead[j];
			mine = clo_op_seg_combine<OP, true, TS>(mine, st[j]);
		}
		request(t0 + SEG_CARRY_TRIP);   // (this thread's own tiles of the next trip: nobody writes them before)
		const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, true, TS>(mine);
		if (lane == 63u) { s_h[wave] = incl.h; s_a[wave] = incl.a; }
		__syncthreads();
		clo_op_seg_state<TS> before = running, all = running;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) SEG_WAVES; ++w) {
			clo_op_seg_state<TS> p;
			p.h = s_h[w]; p.a = s_a[w];
			if (w < wave) before = clo_op_seg_combine<OP, true, TS>(before, p);
			all = clo_op_seg_combine<OP, true, TS>(all, p);
		}
		clo_op_seg_state<TS> s = clo_op_seg_combine<OP, true, TS>(before, clo_op_seg_wave_exclusive<OP, true, TS>(incl, lane));
		seg_u64 out[SEG_CARRY_ITEMS];   // (tile_h is not needed again)
		#pragma unroll
		for (int j = 0; j < SEG_CARRY_ITEMS; ++j) {
			out[j] = (seg_u64) s.a;
			s = clo_op_seg_combine<OP, true, TS>(s, st[j]);
		}
		if (t0 + SEG_CARRY_ITEMS <= tiles) {
			#pragma unroll
			for (int j = 0; j < SEG_CARRY_ITEMS; j += 2) {
				vec2 a;
				a.x = out[j]; a.y = out[j + 1];
				*reinterpret_cast<vec2*>(tile_a + t0 + j) = a;
			}
		} else {
			#pragma unroll
			for (int j = 0; j < SEG_CARRY_ITEMS; ++j) if (t0 + j < tiles) tile_a[t0 + j] = out[j];
		}
		running = all;
		__syncthreads();   // s_h / s_a are written again in the next trip
	}
}

// ---- 5. fix-up: the carry into tile t joins the first segment that closes there ----
template <typename TS, int OP>
__global__ __launch_bounds__(SEG_THREADS)
void clo_segreduce_fixup_kernel(const unsigned* __restrict__ tile_first, const seg_u64* __restrict__ tile_a, unsigned tiles, unsigned m_h,
	TS* __restrict__ aggr_out, TS flip) {
	const unsigned t = blockIdx.x * SEG_THREADS + threadIdx.x;
	if (t >= tiles) return;
	const unsigned r = tile_first[t];
	if (r >= m_h) return;   // SEG_NONE, or not a row of aggr_out
	const TS carry = (TS) tile_a[t];
	if constexpr (OP == CLO_OP_SUM) aggr_out[r] = (TS) (aggr_out[r] + carry);
	else aggr_out[r] = (TS) (clo_op_seg_op<OP, TS>(carry, (TS) (aggr_out[r] ^ flip)) ^ flip);
}

struct seg_args {
	const void* src; const seg_u64* num_in; const void* vin; void* aggr; seg_u64* num_out;
	unsigned m_h, n; seg_u64 flip;
	seg_u64* ends; unsigned* split; unsigned* tile_h; unsigned* tile_first; seg_u64* tile_a; seg_u64* tsum; hipStream_t s;
};

template <typename TC>
int seg_ends_launch(const seg_args& a) {
	const unsigned tiles = (unsigned) clo_op_ends_tiles(a.m_h);
	const int vec_ok = clo_op_vec_ok<TC>(a.src);
	{
		clo_timing_scope timing("segreduce_sums", a.s);
		hipLaunchKernelGGL((clo_segreduce_sums_kernel<TC>), dim3(tiles), dim3(SEG_THREADS), 0, a.s, (const TC*) a.src, a.num_in, a.m_h, vec_ok, a.tsum);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segreduce_sums_scan", a.s);
		hipLaunchKernelGGL(clo_segreduce_sums_scan_kernel, dim3(1), dim3(SEG_THREADS), 0, a.s, a.tsum, tiles);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segreduce_ends", a.s);
	hipLaunchKernelGGL((clo_segreduce_ends_kernel<TC>), dim3(tiles), dim3(SEG_THREADS), 0, a.s, (const TC*) a.src, a.num_in, a.m_h, vec_ok,
		(const seg_u64*) a.tsum, a.ends);
	return (int) hipGetLastError();
}

template <typename TC, bool OFFSETS, int CVT, int OP>
int seg_launch(const seg_args& a) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	if constexpr (!OFFSETS) {
		const int st = seg_ends_launch<TC>(a);
		if (st != 0) return st;
	}
	const unsigned tiles = (unsigned) seg_tiles(a.m_h, a.n);   // >= 1: m_h > 0
	{
		clo_timing_scope timing("segreduce_partition", a.s);
		hipLaunchKernelGGL((clo_segreduce_partition_kernel<TC, OFFSETS>), dim3(tiles / SEG_THREADS + 1u), dim3(SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const seg_u64*) a.ends, a.num_in, a.m_h, a.n, tiles, a.split, a.num_out);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segreduce_sweep", a.s);
		hipLaunchKernelGGL((clo_segreduce_sweep_kernel<TC, OFFSETS, CVT, OP>), dim3(tiles), dim3(SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const seg_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TV*) a.vin, (TS*) a.aggr, (TS) a.flip,
			a.tile_h, a.tile_first, a.tile_a);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segreduce_carry", a.s);
		hipLaunchKernelGGL((clo_segreduce_carry_kernel<TS, OP>), dim3(1), dim3(SEG_THREADS), 0, a.s, a.tile_h, a.tile_a, tiles);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segreduce_fixup", a.s);
	hipLaunchKernelGGL((clo_segreduce_fixup_kernel<TS, OP>), dim3((tiles + SEG_THREADS - 1u) / SEG_THREADS), dim3(SEG_THREADS), 0, a.s,
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
	return (value_size == 4 || value_size == 8) && (sum_size == 4 || sum_size == 8) && sum_size >= value_size ? SEG_TILE : 0;
}

size_t clo_hip_segreduce_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	const size_t tiles = seg_tiles(numel_seg, numel);
	// the ends of the counts form, the tile boundaries' splits, the tiles' three words, the sums of the ends' scan
	return clo_op_ws_align(numel_seg * sizeof(seg_u64)) + clo_op_ws_align((tiles + 1) * sizeof(unsigned)) + 2 * clo_op_ws_align(tiles * sizeof(unsigned))
		+ clo_op_ws_align(tiles * sizeof(seg_u64)) + clo_op_ws_align((clo_op_ends_tiles(numel_seg) + 1) * sizeof(seg_u64));
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
	const size_t tiles = seg_tiles(numel_seg, numel);
	char* ws = (char*) workspace;
	a.ends = (seg_u64*) ws;
	ws += clo_op_ws_align(numel_seg * sizeof(seg_u64));
	a.split = (unsigned*) ws;
	ws += clo_op_ws_align((tiles + 1) * sizeof(unsigned));
	a.tile_h = (unsigned*) ws;
	ws += clo_op_ws_align(tiles * sizeof(unsigned));
	a.tile_first = (unsigned*) ws;
	ws += clo_op_ws_align(tiles * sizeof(unsigned));
	a.tile_a = (seg_u64*) ws;
	ws += clo_op_ws_align(tiles * sizeof(seg_u64));
	a.tsum = (seg_u64*) ws;
	return count_size == 8 ? seg_dispatch<uint64_t>(a, form, cvt, op) : seg_dispatch<uint32_t>(a, form, cvt, op);
}

}  // extern "C"
