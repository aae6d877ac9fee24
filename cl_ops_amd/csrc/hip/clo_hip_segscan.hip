// clo_hip_segscan.hip — running sum, min and max within segments given by counts or by CSR offsets (CloSegScan,
// include/clo_segscan.h; not upstream). With m = min(numel_seg, *num_in) segments whose ends are e_r (the
// running sums of the counts, or offsets[r + 1] - offsets[0]), n rows of values and ct = min(e_(m-1), n): every row i < ct
// lies in one clipped segment, whose first row is b(i), and
//     data_out[i] = op over j in [b(i), i] (inclusive) or [b(i), i) (exclusive) of (sum type) values_in[j].
//
// The schedule is CloSegReduce's merge path (clo_hip_segreduce.hip, Merrill & Garland's merge-based SpMV): the m clipped
// ends c_r = min(e_r, n) are merged with the row indices 0 .. n - 1, an end going first when c_r <= j. A step of the merge
// either CLOSES segment r (what is open starts again from the identity) or takes row j; a tile is T steps, whatever they
// are, so that a work-group's work does not depend on how the ends are spread. None of the launches waits for another
// work-group, none uses a global atomic:
//   ENDS       the counts form only: the numel_seg inclusive ends as uint64 in the workspace (the three launches CloExpand
//              has, clo_hip_op_device.h). The offsets form is read where it lies.
//   PARTITION  one thread per tile boundary d = t * T: split[t] = how many of the first d steps close a segment, by a
//              halving over the ends; thread 0 writes num_out = e_(m-1).
//   TAILS      one work-group per tile: the tile's state, (does a segment close here, the op over the rows it takes after
//              its last close). The last close is ONE clipped end, so the rows are [c, b0 + nb) with c clamped into the
//              tile's rows: the whole tile where nothing closes, a few rows where the segments are short. No merge.
//   CARRY      one work-group: the exclusive segmented scan of the tiles' states, SCAN_CARRY_TRIP tiles per trip.
//   SWEEP      one work-group per tile. The split is CLAMPED to what d, m and n alone allow. The tile's rows are staged in
//              LDS by 16-byte loads, its ends as 16-bit positions relative to the tile's first row. A lane finds where its
//              17 steps begin by a halving in LDS; which of them close is a bit mask from independent LDS reads. The lanes'
//              states go through the segmented scan of the by-key operations, starting from the tile's carry. Every lane
//              then walks its steps again from registers and puts the running value of each ROW (before or after the row,
//              by kind) into LDS at the row's position; the tile leaves as one coalesced stretch
//              data_out[b0, min(b0 + nb, ct)).
// values_in is read once, plus the open tails. In place (data_out == values_in, equal widths): TAILS completes before
// SWEEP on the stream, and a group of SWEEP stages its rows before it stores the same rows; no group reads another's.
// Whatever the arrays hold: the halvings are loops over [lo, hi) that shrink every trip; ends are loaded at indices below
// m only; a tile's rows are [b0, b0 + nb) with b0 + nb <= n by the clamp; an end's position is clamped to [0, nb]; a
// lane's LDS positions are clamped below T; the store is count min(nb, ct - b0) from b0, so it stays in data_out[0, n).
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

typedef clo_op_u64 sscan_u64;

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
static_assert(SCAN_THREADS == CLO_OP_THREADS, "the shared helpers stride by CLO_OP_THREADS");
constexpr int SCAN_ITEMS = 17;                                    // merge steps per lane: odd, so that the lanes' LDS accesses spread over the banks
constexpr unsigned SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;         // T = 4352 merge steps, for every type
static_assert(SCAN_TILE < 65536u, "an end's position in its tile is kept in 16 bits");
constexpr int SCAN_CARRY_ITEMS = 16;
static_assert(SCAN_CARRY_ITEMS % 4 == 0, "a thread's states are loaded four and two at a time");
constexpr unsigned SCAN_CARRY_TRIP = SCAN_THREADS * SCAN_CARRY_ITEMS;   // tile states per trip of the one-group scan

inline size_t sscan_tiles(size_t numel_seg, size_t numel) { return (numel_seg + numel + SCAN_TILE - 1) / SCAN_TILE; }

__device__ __forceinline__ sscan_u64 sscan_min64(sscan_u64 a, sscan_u64 b) { return a < b ? a : b; }
__device__ __forceinline__ sscan_u64 sscan_max64(sscan_u64 a, sscan_u64 b) { return a > b ? a : b; }

// ---- 1. the ends of the counts form: the three launches of clo_hip_op_device.h ----

template <typename TC>
__global__ __launch_bounds__(SCAN_THREADS)
void clo_segscan_sums_kernel(const TC* __restrict__ counts, const sscan_u64* __restrict__ num_in, unsigned m_h, int vec_ok, sscan_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(SCAN_THREADS)
void clo_segscan_sums_scan_kernel(sscan_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(SCAN_THREADS)
void clo_segscan_ends_kernel(const TC* __restrict__ counts, const sscan_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const sscan_u64* __restrict__ tsum, sscan_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. partition ----
// split[t] = how many of the first d = min(t * T, m + n) merge steps close a segment; in [max(0, d - n), min(d, m)].
template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(SCAN_THREADS)
void clo_segscan_partition_kernel(const TC* __restrict__ src, const sscan_u64* __restrict__ ends, const sscan_u64* __restrict__ num_in, unsigned m_h,
	unsigned n, unsigned tiles, unsigned* __restrict__ split, sscan_u64* __restrict__ num_out) {
	const unsigned t = blockIdx.x * SCAN_THREADS + threadIdx.x;
	if (t > tiles) return;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	const sscan_u64 d = sscan_min64((sscan_u64) t * SCAN_TILE, (sscan_u64) m + n);
	unsigned lo = d > n ? (unsigned) (d - n) : 0u, hi = (unsigned) sscan_min64(d, m);
	while (lo < hi) {   // at most 32 trips: hi - lo halves
		const unsigned mid = lo + ((hi - lo) >> 1);   // < hi <= m
		const sscan_u64 c = sscan_min64(e.at(mid), n);
		if (c <= d - 1u - mid) lo = mid + 1u; else hi = mid;
	}
	split[t] = lo;
	if (t == 0) *num_out = m > 0u ? e.at(m - 1u) : 0ull;
}

// numel_seg 0: there is nothing to read
__global__ void clo_segscan_empty_kernel(sscan_u64* __restrict__ num_out) { *num_out = 0ull; }

// The tile's steps [d0, d0 + cnt), of which [a0, a0 + na) close segments and the rest take rows [b0, b0 + nb): the split
// clamped to what d0, d1, m and n alone allow (clo_op_tile_range's rule, in 64 bits: m + n may pass 2^32), so that
// a0 + na <= m and b0 + nb <= n whatever the partition found.
struct sscan_range { unsigned cnt, a0, na, nb; sscan_u64 b0; };

__device__ __forceinline__ sscan_range sscan_tile_range(const unsigned* __restrict__ split, unsigned m, unsigned n) {
	const sscan_u64 total = (sscan_u64) m + n, dd0 = (sscan_u64) blockIdx.x * SCAN_TILE;
	const sscan_u64 d0 = sscan_min64(dd0, total), d1 = sscan_min64(dd0 + SCAN_TILE, total);
	sscan_range r;
	r.cnt = (unsigned) (d1 - d0);
	r.a0 = 0u; r.na = 0u; r.nb = 0u; r.b0 = 0ull;
	if (r.cnt == 0u) return r;   // beyond the last step (m < numel_seg): split is not looked at
	sscan_u64 a0w = split[blockIdx.x], a1w = split[blockIdx.x + 1u];
	a0w = sscan_min64(sscan_max64(a0w, d0 > n ? d0 - n : 0ull), sscan_min64(d0, m));
	a1w = sscan_min64(sscan_max64(a1w, sscan_max64(a0w, d1 > n ? d1 - n : 0ull)), sscan_min64(m, a0w + r.cnt));
	r.a0 = (unsigned) a0w;
	r.na = (unsigned) (a1w - a0w);
	r.nb = r.cnt - r.na;
	r.b0 = d0 - a0w;   // b0 + nb = d1 - a1 <= n
	return r;
}

// (sum type) value, for min and max with the sign bit of a signed sum type flipped: compared as unsigned numbers
template <int CVT, int OP>
__device__ __forceinline__ typename clo_op_cvt<CVT>::TS sscan_value(typename clo_op_cvt<CVT>::TV raw, typename clo_op_cvt<CVT>::TS flip) {
	typedef typename clo_op_cvt<CVT>::TS TS;
	return OP == CLO_OP_SUM ? (TS) raw : (TS) ((TS) raw ^ flip);
}

// ---- 3. tails: the state of every tile ----
template <typename TC, bool OFFSETS, int CVT, int OP>
__global__ __launch_bounds__(SCAN_THREADS)
void clo_segscan_tails_kernel(const TC* __restrict__ src, const sscan_u64* __restrict__ ends, const sscan_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ split, const typename clo_op_cvt<CVT>::TV* __restrict__ values, typename clo_op_cvt<CVT>::TS flip,
	unsigned* __restrict__ tile_h, sscan_u64* __restrict__ tile_a) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	__shared__ TS s_a[SCAN_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);
	const sscan_range g = sscan_tile_range(split, m, n);
	if (g.cnt == 0u) {   // the whole work-group
		if (tid == 0u) { tile_h[blockIdx.x] = 0u; tile_a[blockIdx.x] = (sscan_u64) clo_op_seg_identity<OP, TS>(); }
		return;
	}
	// the rows after the tile's last close: [c, b0 + nb), c the last closing end clipped and clamped into the tile's rows
	sscan_u64 c = g.b0;
	if (g.na > 0u) {
		const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
		const sscan_u64 last = sscan_min64(e.at(g.a0 + g.na - 1u), n);   // a0 + na - 1 < m
		c = sscan_min64(sscan_max64(last, g.b0), g.b0 + g.nb);
	}
	const TV* __restrict__ p = values + c;
	const unsigned count = (unsigned) (g.b0 + g.nb - c);   // <= nb <= T, and c + count <= n
	TS acc = clo_op_seg_identity<OP, TS>();
	{   // clo_op_stage's division: 16-byte loads from p's first 16-byte boundary on
		constexpr unsigned PER = 16u / sizeof(TV);
		typedef TV vec __attribute__((ext_vector_type(PER)));
		const unsigned head = clo_op_min((unsigned) ((16u - ((uintptr_t) p & 15u)) & 15u) / (unsigned) sizeof(TV), count);
		const unsigned nvec = (count - head) / PER, body_end = head + nvec * PER;
		for (unsigned v = tid; v < nvec; v += SCAN_THREADS) {
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
		for (int w = 1; w < SCAN_WAVES; ++w) all = clo_op_seg_op<OP, TS>(all, s_a[w]);
		tile_h[blockIdx.x] = g.na > 0u ? 1u : 0u;
		tile_a[blockIdx.x] = (sscan_u64) all;
	}
}

// ---- 4. carry scan: one group; tile t gets the state of the tiles before it, in place (clo_segreduce_carry_kernel's
// walk, SCAN_CARRY_TRIP states per trip) ----
template <typename TS, int OP>
__global__ __launch_bounds__(SCAN_THREADS)
void clo_segscan_carry_kernel(const unsigned* __restrict__ tile_h, sscan_u64* __restrict__ tile_a, unsigned tiles) {
	__shared__ unsigned s_h[SCAN_WAVES];
	__shared__ TS s_a[SCAN_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	clo_op_seg_state<TS> running = clo_op_seg_empty<OP, TS>();   // the state of everything before this trip (the same in every thread)
	// the next trip's states are requested before this trip's are combined
	clo_op_seg_state<TS> ahead[SCAN_CARRY_ITEMS];
	typedef unsigned vec4 __attribute__((ext_vector_type(4)));
	typedef sscan_u64 vec2 __attribute__((ext_vector_type(2)));
	auto request = [&](unsigned first) {
		if (first + SCAN_CARRY_ITEMS <= tiles) {   // 16-byte loads: the arrays are 256-byte aligned, `first` a multiple of SCAN_CARRY_ITEMS
			#pragma unroll
			for (int j = 0; j < SCAN_CARRY_ITEMS; j += 4) {
				const vec4 h = *reinterpret_cast<const vec4*>(tile_h + first + j);
				ahead[j].h = h.x; ahead[j + 1].h = h.y; ahead[j + 2].h = h.z; ahead[j + 3].h = h.w;
			}
			#pragma unroll
			for (int j = 0; j < SCAN_CARRY_ITEMS; j += 2) {
				const vec2 a = *reinterpret_cast<const vec2*>(tile_a + first + j);
				ahead[j].a = (TS) a.x; ahead[j + 1].a = (TS) a.y;
			}
		} else {
			#pragma unroll
			for (int j = 0; j < SCAN_CARRY_ITEMS; ++j) {
				ahead[j] = clo_op_seg_empty<OP, TS>();
				if (first + j < tiles) { ahead[j].h = tile_h[first + j]; ahead[j].a = (TS) tile_a[first + j]; }
			}
		}
	};
	request(tid * SCAN_CARRY_ITEMS);
	for (unsigned chunk = 0; chunk < tiles; chunk += SCAN_CARRY_TRIP) {
		const unsigned t0 = chunk + tid * SCAN_CARRY_ITEMS;
		clo_op_seg_state<TS> st[SCAN_CARRY_ITEMS];
		clo_op_seg_state<TS> mine = clo_op_seg_empty<OP, TS>();
		#pragma unroll
		for (int j = 0; j < SCAN_CARRY_ITEMS; ++j) {
			st[j] = ahead[j];
			mine = clo_op_seg_combine<OP, true, TS>(mine, st[j]);
		}
		request(t0 + SCAN_CARRY_TRIP);   // (this thread's own tiles of the next trip: nobody writes them before)
		const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, true, TS>(mine);
		if (lane == 63u) { s_h[wave] = incl.h; s_a[wave] = incl.a; }
		__syncthreads();
		clo_op_seg_state<TS> before = running, all = running;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) SCAN_WAVES; ++w) {
			clo_op_seg_state<TS> p;
			p.h = s_h[w]; p.a = s_a[w];
			if (w < wave) before = clo_op_seg_combine<OP, true, TS>(before, p);
			all = clo_op_seg_combine<OP, true, TS>(all, p);
		}
		clo_op_seg_state<TS> s = clo_op_seg_combine<OP, true, TS>(before, clo_op_seg_wave_exclusive<OP, true, TS>(incl, lane));
		sscan_u64 out[SCAN_CARRY_ITEMS];
		#pragma unroll
		for (int j = 0; j < SCAN_CARRY_ITEMS; ++j) {
			out[j] = (sscan_u64) s.a;
			s = clo_op_seg_combine<OP, true, TS>(s, st[j]);
		}
		if (t0 + SCAN_CARRY_ITEMS <= tiles) {
			#pragma unroll
			for (int j = 0; j < SCAN_CARRY_ITEMS; j += 2) {
				vec2 a;
				a.x = out[j]; a.y = out[j + 1];
				*reinterpret_cast<vec2*>(tile_a + t0 + j) = a;
			}
		} else {
			#pragma unroll
			for (int j = 0; j < SCAN_CARRY_ITEMS; ++j) if (t0 + j < tiles) tile_a[t0 + j] = out[j];
		}
		running = all;
		__syncthreads();   // s_h / s_a are written again in the next trip
	}
}

// ---- 5. tile sweep ----
// values and data_out may be the same array (in place): neither is __restrict__.
template <typename TC, bool OFFSETS, int CVT, int OP, bool INCL>
__global__ __launch_bounds__(SCAN_THREADS)
void clo_segscan_sweep_kernel(const TC* __restrict__ src, const sscan_u64* __restrict__ ends, const sscan_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ split, const typename clo_op_cvt<CVT>::TV* values, typename clo_op_cvt<CVT>::TS* data_out,
	typename clo_op_cvt<CVT>::TS flip, const sscan_u64* __restrict__ tile_a) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	// the tile's rows as they lie in memory until the lanes have walked them, then the rows' results
	__shared__ __attribute__((aligned(16))) TS s_val[SCAN_TILE];
	__shared__ unsigned short s_end[SCAN_TILE];   // positions in [0, nb], nb <= T: 16 bits, so that more groups fit a CU
	__shared__ unsigned s_start[SCAN_THREADS + 1];
	__shared__ unsigned s_h[SCAN_WAVES];
	__shared__ TS s_a[SCAN_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);
	const sscan_range g = sscan_tile_range(split, m, n);
	if (g.cnt == 0u || g.nb == 0u) return;   // the whole work-group: beyond the last step, or no row to write
	const unsigned cnt = g.cnt, a0 = g.a0, na = g.na, nb = g.nb;
	const sscan_u64 b0 = g.b0;
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	// rows at and beyond ct = min(e_(m-1), n) are not written
	const sscan_u64 ct = m > 0u ? sscan_min64(e.at(m - 1u), n) : 0ull;
	const unsigned nstore = (unsigned) (sscan_max64(sscan_min64(b0 + nb, ct), b0) - b0);   // the tile's rows below ct: [b0, that end)
	if (nstore == 0u) return;   // the whole work-group
	const TS carry = (TS) tile_a[blockIdx.x];

	clo_keyx kx;
	kx.sign = 0; kx.field = 0; kx.kind = 0;   // (not looked at: the rows are staged as they are)
	clo_op_stage<TV, false>(values + b0, nb, reinterpret_cast<TV*>(s_val), kx, tid);
	for (unsigned k = tid; k < na; k += SCAN_THREADS) {
		const sscan_u64 c = sscan_min64(e.at(a0 + k), n);   // a0 + k < a1 <= m
		s_end[k] = (unsigned short) (c < b0 ? 0u : (unsigned) sscan_min64(c - b0, nb));
	}
	__syncthreads();

	// where this lane's steps begin: of the first d steps of the tile, `a` close a segment
	const unsigned d = clo_op_min(tid * SCAN_ITEMS, cnt);
	unsigned a, b;
	{
		unsigned lo = d > nb ? d - nb : 0u, hi = clo_op_min(d, na);
		while (lo < hi) {
			const unsigned mid = lo + ((hi - lo) >> 1);
			if (s_end[mid] <= d - 1u - mid) lo = mid + 1u; else hi = mid;
		}
		a = lo; b = d - lo;
	}
	// what the lane's steps are is known without walking them: it closes the ends [a, the next lane's a) and takes the
	// rows between them, and end a + j closes at step j + (the lane's rows before it), whatever the other ends are
	s_start[tid] = a;
	if (tid == 0u) s_start[SCAN_THREADS] = na;
	__syncthreads();
	const unsigned steps = clo_op_min((unsigned) SCAN_ITEMS, cnt - d);
	const unsigned ne = clo_op_min(clo_op_max(s_start[tid + 1u], a) - a, steps);
	const unsigned nr = steps - ne;   // its rows [b, b + nr); b + nr <= nb
	unsigned closes = 0u;             // bit k = step k closes a segment
	#pragma unroll
	for (int j = 0; j < SCAN_ITEMS; ++j) {
		const unsigned ea = s_end[clo_op_min(a + (unsigned) j, SCAN_TILE - 1u)];
		const unsigned p = clo_op_min(ea > b ? ea - b : 0u, nr) + (unsigned) j;   // < steps where j < ne
		closes |= ((unsigned) j < ne ? 1u : 0u) << (p & 31u);
	}
	// x[k] = the value of the row step k takes, the identity where it takes none: 17 reads that do not wait for each other
	const TV* s_row = reinterpret_cast<const TV*>(s_val);
	TS x[SCAN_ITEMS];
	clo_op_seg_state<TS> s = clo_op_seg_empty<OP, TS>();
	#pragma unroll
	for (int k = 0; k < SCAN_ITEMS; ++k) {
		const bool close = (closes >> k) & 1u;
		const unsigned rs = (unsigned) k - (unsigned) __popc(closes & ((1u << k) - 1u));
		const TV raw = s_row[clo_op_min(b + rs, SCAN_TILE - 1u)];
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
	for (unsigned w = 0; w < (unsigned) SCAN_WAVES; ++w) {
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
	for (int k = 0; k < SCAN_ITEMS; ++k) {
		if ((closes >> k) & 1u) {
			open = clo_op_seg_identity<OP, TS>();
		} else if ((unsigned) k < steps) {
			const TS after = clo_op_seg_op<OP, TS>(open, x[k]);
			s_val[clo_op_min(at, SCAN_TILE - 1u)] = INCL ? after : open;
			open = after;
			++at;
		}
	}
	__syncthreads();
	clo_op_store<TS>(data_out + b0, nstore, tid, [&](unsigned i) { return OP == CLO_OP_SUM ? s_val[i] : (TS) (s_val[i] ^ flip); });
}

struct sscan_args {
	const void* src; const sscan_u64* num_in; const void* vin; void* out; sscan_u64* num_out;
	unsigned m_h, n; sscan_u64 flip;
	sscan_u64* ends; unsigned* split; unsigned* tile_h; sscan_u64* tile_a; sscan_u64* tsum; hipStream_t s;
};

template <typename TC>
int sscan_ends_launch(const sscan_args& a) {
	const unsigned tiles = (unsigned) clo_op_ends_tiles(a.m_h);
	const int vec_ok = clo_op_vec_ok<TC>(a.src);
	{
		clo_timing_scope timing("segscan_sums", a.s);
		hipLaunchKernelGGL((clo_segscan_sums_kernel<TC>), dim3(tiles), dim3(SCAN_THREADS), 0, a.s, (const TC*) a.src, a.num_in, a.m_h, vec_ok, a.tsum);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segscan_sums_scan", a.s);
		hipLaunchKernelGGL(clo_segscan_sums_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, a.s, a.tsum, tiles);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segscan_ends", a.s);
	hipLaunchKernelGGL((clo_segscan_ends_kernel<TC>), dim3(tiles), dim3(SCAN_THREADS), 0, a.s, (const TC*) a.src, a.num_in, a.m_h, vec_ok,
		(const sscan_u64*) a.tsum, a.ends);
	return (int) hipGetLastError();
}

// the launches every kind shares: ends, partition, tails, carry
template <typename TC, bool OFFSETS, int CVT, int OP>
int sscan_launch_states(const sscan_args& a, unsigned tiles) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	if constexpr (!OFFSETS) {
		const int st = sscan_ends_launch<TC>(a);
		if (st != 0) return st;
	}
	{
		clo_timing_scope timing("segscan_partition", a.s);
		hipLaunchKernelGGL((clo_segscan_partition_kernel<TC, OFFSETS>), dim3(tiles / SCAN_THREADS + 1u), dim3(SCAN_THREADS), 0, a.s,
			(const TC*) a.src, (const sscan_u64*) a.ends, a.num_in, a.m_h, a.n, tiles, a.split, a.num_out);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	if (a.n == 0u) return 0;   // no row: num_out is all there is to write
	{
		clo_timing_scope timing("segscan_tails", a.s);
		hipLaunchKernelGGL((clo_segscan_tails_kernel<TC, OFFSETS, CVT, OP>), dim3(tiles), dim3(SCAN_THREADS), 0, a.s,
			(const TC*) a.src, (const sscan_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TV*) a.vin, (TS) a.flip, a.tile_h, a.tile_a);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segscan_carry", a.s);
	hipLaunchKernelGGL((clo_segscan_carry_kernel<TS, OP>), dim3(1), dim3(SCAN_THREADS), 0, a.s, (const unsigned*) a.tile_h, a.tile_a, tiles);
	return (int) hipGetLastError();
}

template <typename TC, bool OFFSETS, int CVT, int OP>
int sscan_launch(const sscan_args& a, int inclusive) {
	typedef typename clo_op_cvt<CVT>::TV TV;
	typedef typename clo_op_cvt<CVT>::TS TS;
	const unsigned tiles = (unsigned) sscan_tiles(a.m_h, a.n);   // >= 1: m_h > 0
	const int st = sscan_launch_states<TC, OFFSETS, CVT, OP>(a, tiles);
	if (st != 0 || a.n == 0u) return st;
	clo_timing_scope timing("segscan_sweep", a.s);
	if (inclusive)
		hipLaunchKernelGGL((clo_segscan_sweep_kernel<TC, OFFSETS, CVT, OP, true>), dim3(tiles), dim3(SCAN_THREADS), 0, a.s,
			(const TC*) a.src, (const sscan_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TV*) a.vin, (TS*) a.out, (TS) a.flip,
			(const sscan_u64*) a.tile_a);
	else
		hipLaunchKernelGGL((clo_segscan_sweep_kernel<TC, OFFSETS, CVT, OP, false>), dim3(tiles), dim3(SCAN_THREADS), 0, a.s,
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
	return (value_size == 4 || value_size == 8) && (sum_size == 4 || sum_size == 8) && sum_size >= value_size ? SCAN_TILE : 0;
}

size_t clo_hip_segscan_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	const size_t tiles = sscan_tiles(numel_seg, numel);
	// the ends of the counts form, the tile boundaries' splits, the tiles' two words, the sums of the ends' scan
	return clo_op_ws_align(numel_seg * sizeof(sscan_u64)) + clo_op_ws_align((tiles + 1) * sizeof(unsigned)) + clo_op_ws_align(tiles * sizeof(unsigned))
		+ clo_op_ws_align(tiles * sizeof(sscan_u64)) + clo_op_ws_align((clo_op_ends_tiles(numel_seg) + 1) * sizeof(sscan_u64));
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
	const size_t tiles = sscan_tiles(numel_seg, numel);
	char* ws = (char*) workspace;
	a.ends = (sscan_u64*) ws;
	ws += clo_op_ws_align(numel_seg * sizeof(sscan_u64));
	a.split = (unsigned*) ws;
	ws += clo_op_ws_align((tiles + 1) * sizeof(unsigned));
	a.tile_h = (unsigned*) ws;
	ws += clo_op_ws_align(tiles * sizeof(unsigned));
	a.tile_a = (sscan_u64*) ws;
	ws += clo_op_ws_align(tiles * sizeof(sscan_u64));
	a.tsum = (sscan_u64*) ws;
	return count_size == 8 ? sscan_dispatch<uint64_t>(a, form, cvt, op, inclusive) : sscan_dispatch<uint32_t>(a, form, cvt, op, inclusive);
}

}  // extern "C"
