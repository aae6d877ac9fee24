// clo_hip_seg_device.h — what the kernels of the operations over "segments from counts or offsets" share on top of
// clo_hip_op_device.h: the 64-bit segment ends with their three launches (clo_hip_expand, segreduce,
// segsort, segscan, segarg and bucket .hip) and the merge path of segments and rows (segreduce, segscan, segarg). The
// rule is that header's: a piece is here once because its copies were the same text; what differs on purpose stays in
// its file; everything has internal linkage, and every __global__ function stays in its own file under its own name.
//
// THE MERGE PATH (Merrill & Garland's merge-based SpMV). With m = min(numel_seg, *num_in) segments whose ends are e_r
// and n rows, the m clipped ends c_r = min(e_r, n) are merged with the row indices 0 .. n - 1, an end going first when
// c_r <= j. A step of the merge either CLOSES segment r or takes row j; a tile is T = CLO_SEG_TILE steps, whatever they
// are, so that a work-group's work does not depend on how the ends are spread. None of the launches waits for another
// work-group, none uses a global atomic:
//   ENDS       the counts form only: the numel_seg inclusive ends as uint64 in the workspace, three launches
//              (clo_op_ends_launch). The offsets form is read where it lies.
//   PARTITION  one thread per tile boundary d = t * T: split[t] = how many of the first d steps close a segment, by a
//              halving over the ends; thread 0 writes num_out = e_(m-1) (clo_seg_partition).
//   SWEEP      one work-group per tile. The split is CLAMPED to what d, m and n alone allow (clo_seg_tile_clamp). The
//              tile's rows are staged in LDS by 16-byte loads, its ends as 16-bit positions relative to the tile's first
//              row (clo_seg_stage_ends). A lane finds where its CLO_SEG_ITEMS steps begin by a halving in LDS and learns
//              from the next lane's beginning how many of them close a segment (clo_seg_lane_begin); end a + j of the lane
//              then closes at step j + (the lane's rows before it), so the steps are known as a bit mask without walking
//              them (clo_seg_lane_closes), and the LDS reads of ends and those of rows do not wait for each other. What a
//              lane does with its steps, and the second walk that writes, is the operation's.
//   CARRY      one work-group: the exclusive segmented scan of the tiles' states, CLO_SEG_CARRY_TRIP tiles per trip
//              (clo_seg_carry for clo_op_seg_state; CloSegArg's aggregate has its own kernel).
// Whatever the arrays hold: the halvings are loops over [lo, hi) that shrink every trip; ends are loaded at indices below
// m only; a tile's rows are [b0, b0 + nb) with b0 + nb <= n and its closing segments [a0, a0 + na) with a0 + na <= m by
// the clamp; an end's position is clamped to [0, nb]; a lane's LDS indices are clamped below T; a lane closes at most
// ne segments with a + ne <= na. By this argument a wrong split or unsorted ends give wrong results, never an access
// outside the arrays (the tests of broken preconditions; DESIGN.md §26 for what mutation runs did and did not show).
#ifndef CLO_HIP_SEG_DEVICE_H
#define CLO_HIP_SEG_DEVICE_H

#include "clo_hip_op_device.h"

namespace {

// ---- the 64-bit segment ends of counts or offsets ----

typedef unsigned long long clo_op_u64;

__device__ __forceinline__ clo_op_u64 clo_op_min64(clo_op_u64 a, clo_op_u64 b) { return a < b ? a : b; }
__device__ __forceinline__ clo_op_u64 clo_op_max64(clo_op_u64 a, clo_op_u64 b) { return a > b ? a : b; }

constexpr int CLO_OP_WAVES = CLO_OP_THREADS / 64;
constexpr int CLO_OP_ROW_ELEMS = CLO_OP_THREADS * CLO_OP_VEC;            // 1024 counts: one coalesced stretch
constexpr int CLO_OP_ENDS_ROWS = 4;
constexpr unsigned CLO_OP_ENDS_TILE = CLO_OP_ENDS_ROWS * CLO_OP_ROW_ELEMS;   // counts per tile of the ends' scan
constexpr unsigned CLO_OP_SUMS_ITEMS = 8;
constexpr unsigned CLO_OP_SUMS_TRIP = CLO_OP_THREADS * CLO_OP_SUMS_ITEMS;    // tile sums per trip of the one-group scan
inline size_t clo_op_ends_tiles(size_t m_h) { return (m_h + CLO_OP_ENDS_TILE - 1) / CLO_OP_ENDS_TILE; }

// The next region of a workspace laid out from `base`: `count` elements of T from offset `at`, which moves past them.
// base null: only the size is wanted, and the pointer is null.
template <typename T>
inline T* clo_op_ws_take(char* base, size_t& at, size_t count) {
	T* const p = base ? reinterpret_cast<T*>(base + at) : nullptr;
	at += clo_op_ws_align(count * sizeof(T));
	return p;
}

// m = min(m_h, *num_in)
__device__ __forceinline__ unsigned clo_op_segments(const clo_op_u64* __restrict__ num_in, unsigned m_h) {
	if (!num_in) return m_h;
	const clo_op_u64 v = *num_in;
	return v < m_h ? (unsigned) v : m_h;
}

// Where the inclusive ends are: the workspace (counts form) or the offsets themselves, rebased. at(r) needs r < m_h.
template <typename TC, bool OFFSETS>
struct clo_op_ends {
	const TC* off; const clo_op_u64* ends; clo_op_u64 base;
	__device__ __forceinline__ clo_op_u64 at(unsigned r) const {
		if constexpr (OFFSETS) return (clo_op_u64) off[(size_t) r + 1u] - base;
		else return ends[r];
	}
};

template <typename TC, bool OFFSETS>
__device__ __forceinline__ clo_op_ends<TC, OFFSETS> clo_op_ends_make(const TC* __restrict__ src, const clo_op_u64* __restrict__ ends) {   // m_h > 0
	clo_op_ends<TC, OFFSETS> e;
	e.off = src; e.ends = ends;
	e.base = OFFSETS ? (clo_op_u64) src[0] : 0ull;
	return e;
}

// the tile's counts as 64-bit numbers, those at r >= m as 0: row by row, four consecutive ones per lane
template <typename TC>
__device__ __forceinline__ void clo_op_ends_load_counts(const TC* __restrict__ counts, size_t i0, unsigned m_h, unsigned m, bool vec_ok,
	clo_op_u64 (&c)[CLO_OP_VEC]) {
	TC raw[CLO_OP_VEC];
	clo_op_load4<TC>(counts, i0, m_h, vec_ok, raw);
	#pragma unroll
	for (int k = 0; k < CLO_OP_VEC; ++k) c[k] = i0 + k < m ? (clo_op_u64) raw[k] : 0ull;
}

// The bodies of the three launches that write the m_h inclusive ends of the counts form (CloSelect's count scan, in 64
// bits); the __global__ functions that call them stay in the operations' files. 1: the sum of every tile of
// CLO_OP_ENDS_TILE counts.
template <typename TC>
__device__ __forceinline__ void clo_op_ends_sums(const TC* __restrict__ counts, const clo_op_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	clo_op_u64* __restrict__ tsum) {
	__shared__ clo_op_u64 s_wave[CLO_OP_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);
	const size_t base = (size_t) blockIdx.x * CLO_OP_ENDS_TILE + (size_t) tid * CLO_OP_VEC;
	clo_op_u64 sum = 0;
	#pragma unroll
	for (int r = 0; r < CLO_OP_ENDS_ROWS; ++r) {
		clo_op_u64 c[CLO_OP_VEC];
		clo_op_ends_load_counts<TC>(counts, base + (size_t) r * CLO_OP_ROW_ELEMS, m_h, m, vec_ok != 0, c);
		sum += c[0] + c[1] + c[2] + c[3];
	}
	sum = clo_wave_reduce_sum<clo_op_u64>(sum);
	if (lane == 0) s_wave[wave] = sum;
	__syncthreads();
	if (tid == 0) tsum[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// 2: tsum[0, tiles) -> its exclusive sums in place (modulo 2^64). One work-group; the next trip's sums are requested
// before this trip's are added.
__device__ __forceinline__ void clo_op_ends_sums_scan(clo_op_u64* __restrict__ tsum, unsigned tiles) {
	__shared__ clo_op_u64 s_wave[CLO_OP_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	clo_op_u64 carry = 0;
	clo_op_u64 v[CLO_OP_SUMS_ITEMS], ahead[CLO_OP_SUMS_ITEMS];
	#pragma unroll
	for (unsigned c = 0; c < CLO_OP_SUMS_ITEMS; ++c) {
		const unsigned i = tid * CLO_OP_SUMS_ITEMS + c;
		ahead[c] = i < tiles ? tsum[i] : 0ull;
	}
	for (unsigned base = 0; base < tiles; base += CLO_OP_SUMS_TRIP) {   // tiles <= 2^20: no wrap
		clo_op_u64 sum = 0;
		#pragma unroll
		for (unsigned c = 0; c < CLO_OP_SUMS_ITEMS; ++c) {
			v[c] = ahead[c];
			sum += v[c];
			const unsigned i = base + CLO_OP_SUMS_TRIP + tid * CLO_OP_SUMS_ITEMS + c;
			ahead[c] = i < tiles ? tsum[i] : 0ull;
		}
		const clo_op_u64 incl = clo_wave_scan_inclusive<clo_op_u64>(sum, lane);
		if (lane == 63u) s_wave[wave] = incl;
		__syncthreads();
		clo_op_u64 before = 0, total = 0;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) CLO_OP_WAVES; ++w) {
			const clo_op_u64 s = s_wave[w];
			if (w < wave) before += s;
			total += s;
		}
		clo_op_u64 at = carry + before + incl - sum;
		#pragma unroll
		for (unsigned c = 0; c < CLO_OP_SUMS_ITEMS; ++c) {
			const unsigned i = base + tid * CLO_OP_SUMS_ITEMS + c;
			if (i < tiles) tsum[i] = at;
			at += v[c];
		}
		carry += total;
		__syncthreads();   // s_wave is written again
	}
}

// 3: the tiles' ends, ends[r] for every r < m_h
template <typename TC>
__device__ __forceinline__ void clo_op_ends_write(const TC* __restrict__ counts, const clo_op_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const clo_op_u64* __restrict__ tsum, clo_op_u64* __restrict__ ends) {
	constexpr int PIECES = CLO_OP_ENDS_ROWS * CLO_OP_WAVES;
	__shared__ clo_op_u64 s_piece[PIECES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);
	const size_t base = (size_t) blockIdx.x * CLO_OP_ENDS_TILE + (size_t) tid * CLO_OP_VEC;
	clo_op_u64 c[CLO_OP_ENDS_ROWS][CLO_OP_VEC], before[CLO_OP_ENDS_ROWS];
	#pragma unroll
	for (int r = 0; r < CLO_OP_ENDS_ROWS; ++r) {
		clo_op_ends_load_counts<TC>(counts, base + (size_t) r * CLO_OP_ROW_ELEMS, m_h, m, vec_ok != 0, c[r]);
		const clo_op_u64 t = c[r][0] + c[r][1] + c[r][2] + c[r][3];
		const clo_op_u64 incl = clo_wave_scan_inclusive<clo_op_u64>(t, lane);
		before[r] = incl - t;
		if (lane == 63u) s_piece[r * CLO_OP_WAVES + (int) wave] = incl;
	}
	__syncthreads();
	clo_op_u64 at = tsum[blockIdx.x];
	#pragma unroll
	for (int r = 0; r < CLO_OP_ENDS_ROWS; ++r) {
		#pragma unroll
		for (int w = 0; w < CLO_OP_WAVES; ++w) {
			const clo_op_u64 p = s_piece[r * CLO_OP_WAVES + w];
			if ((unsigned) w < wave) before[r] += p;
		}
		const size_t i0 = base + (size_t) r * CLO_OP_ROW_ELEMS;
		clo_op_u64 e[CLO_OP_VEC];
		clo_op_u64 run = at + before[r];
		#pragma unroll
		for (int k = 0; k < CLO_OP_VEC; ++k) { run += c[r][k]; e[k] = run; }
		if (i0 + CLO_OP_VEC <= m_h) {   // the workspace is 256-byte aligned and i0 a multiple of 4
			typedef clo_op_u64 vec2 __attribute__((ext_vector_type(2)));
			vec2 a, b;
			a.x = e[0]; a.y = e[1]; b.x = e[2]; b.y = e[3];
			*reinterpret_cast<vec2*>(ends + i0) = a;
			*reinterpret_cast<vec2*>(ends + i0 + 2) = b;
		} else {
			#pragma unroll
			for (int k = 0; k < CLO_OP_VEC; ++k) if (i0 + k < m_h) ends[i0 + k] = e[k];
		}
		#pragma unroll
		for (int w = 0; w < CLO_OP_WAVES; ++w) at += s_piece[r * CLO_OP_WAVES + w];
	}
}

// The three launches, for the calling file's three kernels (one-line calls of the bodies above) under its three timing
// labels: m_h counts of type TC at src -> ends[0, m_h), tsum the clo_op_ends_tiles(m_h) + 1 words of the scan. 0 or the
// launch error.
template <typename TC>
int clo_op_ends_launch(void (*sums)(const TC*, const clo_op_u64*, unsigned, int, clo_op_u64*), void (*sums_scan)(clo_op_u64*, unsigned),
	void (*write)(const TC*, const clo_op_u64*, unsigned, int, const clo_op_u64*, clo_op_u64*), const char* const (&labels)[3],
	const void* src, const clo_op_u64* num_in, unsigned m_h, clo_op_u64* tsum, clo_op_u64* ends, hipStream_t s) {
	const unsigned tiles = (unsigned) clo_op_ends_tiles(m_h);
	const int vec_ok = clo_op_vec_ok<TC>(src);
	{
		clo_timing_scope timing(labels[0], s);
		hipLaunchKernelGGL(sums, dim3(tiles), dim3(CLO_OP_THREADS), 0, s, (const TC*) src, num_in, m_h, vec_ok, tsum);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing(labels[1], s);
		hipLaunchKernelGGL(sums_scan, dim3(1), dim3(CLO_OP_THREADS), 0, s, tsum, tiles);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing(labels[2], s);
	hipLaunchKernelGGL(write, dim3(tiles), dim3(CLO_OP_THREADS), 0, s, (const TC*) src, num_in, m_h, vec_ok, (const clo_op_u64*) tsum, ends);
	return (int) hipGetLastError();
}

// ---- the merge path of segments and rows: geometry ----

constexpr int CLO_SEG_THREADS = CLO_OP_THREADS;                 // the shared helpers stride by CLO_OP_THREADS
constexpr int CLO_SEG_WAVES = CLO_SEG_THREADS / 64;
constexpr int CLO_SEG_ITEMS = 17;                               // merge steps per lane: odd, so that the lanes' LDS accesses spread over the banks
constexpr unsigned CLO_SEG_TILE = CLO_SEG_THREADS * CLO_SEG_ITEMS;   // T = 4352 merge steps, for every type
static_assert(CLO_SEG_TILE < 65536u, "an end's position in its tile is kept in 16 bits");
static_assert(CLO_SEG_ITEMS <= 32, "a lane's closing steps are a 32-bit mask");
constexpr int CLO_SEG_CARRY_ITEMS = 16;
static_assert(CLO_SEG_CARRY_ITEMS % 4 == 0, "a thread's states are loaded four and two at a time");
constexpr unsigned CLO_SEG_CARRY_TRIP = CLO_SEG_THREADS * CLO_SEG_CARRY_ITEMS;   // tile states per trip of the one-group scan

inline size_t clo_seg_tiles(size_t numel_seg, size_t numel) { return (numel_seg + numel + CLO_SEG_TILE - 1) / CLO_SEG_TILE; }

// The body of a partition kernel: one thread per tile boundary t <= tiles.
// split[t] = how many of the first d = min(t * T, m + n) merge steps close a segment; in [max(0, d - n), min(d, m)].
template <typename TC, bool OFFSETS>
__device__ __forceinline__ void clo_seg_partition(const TC* __restrict__ src, const clo_op_u64* __restrict__ ends, const clo_op_u64* __restrict__ num_in,
	unsigned m_h, unsigned n, unsigned tiles, unsigned* __restrict__ split, clo_op_u64* __restrict__ num_out) {
	const unsigned t = blockIdx.x * CLO_SEG_THREADS + threadIdx.x;
	if (t > tiles) return;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	const clo_op_u64 d = clo_op_min64((clo_op_u64) t * CLO_SEG_TILE, (clo_op_u64) m + n);
	unsigned lo = d > n ? (unsigned) (d - n) : 0u, hi = (unsigned) clo_op_min64(d, m);
	while (lo < hi) {   // at most 32 trips: hi - lo halves
		const unsigned mid = lo + ((hi - lo) >> 1);   // < hi <= m
		const clo_op_u64 c = clo_op_min64(e.at(mid), n);
		if (c <= d - 1u - mid) lo = mid + 1u; else hi = mid;
	}
	split[t] = lo;
	if (t == 0) *num_out = m > 0u ? e.at(m - 1u) : 0ull;
}

// The tile's steps [d0, d1) of the merge, cnt = d1 - d0 of them; cnt == 0 beyond the last step (m < numel_seg).
struct clo_seg_steps { clo_op_u64 d0, d1; unsigned cnt; };

__device__ __forceinline__ clo_seg_steps clo_seg_tile_steps(unsigned m, unsigned n) {
	const clo_op_u64 total = (clo_op_u64) m + n, dd0 = (clo_op_u64) blockIdx.x * CLO_SEG_TILE;
	clo_seg_steps s;
	s.d0 = clo_op_min64(dd0, total); s.d1 = clo_op_min64(dd0 + CLO_SEG_TILE, total);
	s.cnt = (unsigned) (s.d1 - s.d0);
	return s;
}

// Of the tile's steps, [a0, a0 + na) close segments and the rest take rows [b0, b0 + nb): the split clamped to what d0,
// d1, m and n alone allow (clo_op_tile_range's rule, in 64 bits: m + n may pass 2^32), so that a0 + na <= m and
// b0 + nb <= n whatever the partition found. For a tile with cnt > 0.
struct clo_seg_range { unsigned cnt, a0, na, nb; clo_op_u64 b0; };

__device__ __forceinline__ clo_seg_range clo_seg_tile_clamp(const clo_seg_steps s, const unsigned* __restrict__ split, unsigned m, unsigned n) {
	const clo_op_u64 d0 = s.d0, d1 = s.d1;
	clo_seg_range r;
	r.cnt = s.cnt;
	clo_op_u64 a0w = split[blockIdx.x], a1w = split[blockIdx.x + 1u];
	a0w = clo_op_min64(clo_op_max64(a0w, d0 > n ? d0 - n : 0ull), clo_op_min64(d0, m));
	a1w = clo_op_min64(clo_op_max64(a1w, clo_op_max64(a0w, d1 > n ? d1 - n : 0ull)), clo_op_min64(m, a0w + r.cnt));
	r.a0 = (unsigned) a0w;
	r.na = (unsigned) (a1w - a0w);
	r.nb = r.cnt - r.na;
	r.b0 = d0 - a0w;   // b0 + nb = d1 - a1 <= n
	return r;
}

// Both at once, for a kernel that has nothing to do before the clamp (segscan): cnt == 0 comes back with everything 0,
// and split is not looked at.
__device__ __forceinline__ clo_seg_range clo_seg_tile_range(const unsigned* __restrict__ split, unsigned m, unsigned n) {
	const clo_seg_steps s = clo_seg_tile_steps(m, n);
	clo_seg_range r;
	r.cnt = s.cnt;
	r.a0 = 0u; r.na = 0u; r.nb = 0u; r.b0 = 0ull;
	if (r.cnt == 0u) return r;
	return clo_seg_tile_clamp(s, split, m, n);
}

// ---- the sweep's preamble, over LDS arrays the kernel declares: s_end[CLO_SEG_TILE], s_start[CLO_SEG_THREADS + 1] ----

// The tile's ends as positions in [0, nb] relative to its first row (nb <= T: 16 bits, so that more groups fit a CU).
// A barrier follows before s_end is read.
template <typename TC, bool OFFSETS>
__device__ __forceinline__ void clo_seg_stage_ends(const clo_op_ends<TC, OFFSETS> e, const clo_seg_range g, unsigned n, unsigned short* s_end, unsigned tid) {
	for (unsigned k = tid; k < g.na; k += CLO_SEG_THREADS) {
		const clo_op_u64 c = clo_op_min64(e.at(g.a0 + k), n);   // a0 + k < a1 <= m
		s_end[k] = (unsigned short) (c < g.b0 ? 0u : (unsigned) clo_op_min64(c - g.b0, g.nb));
	}
}

// A lane's steps: it closes the ends [a, a + ne) of the tile and takes its rows [b, b + nr), b + nr <= nb; bit k of
// `closes` = step k closes a segment.
struct clo_seg_lane { unsigned a, b, steps, ne, nr, closes; };

// Where the lane's steps begin, by a halving in LDS: of the first d = tid * CLO_SEG_ITEMS steps of the tile, `a` close a
// segment. What the steps are is then known without walking them: the lane closes the ends [a, the next lane's a) and
// takes the rows between them. The whole work-group, s_end staged and a barrier passed; one barrier inside.
__device__ __forceinline__ clo_seg_lane clo_seg_lane_begin(const clo_seg_range g, const unsigned short* s_end, unsigned* s_start, unsigned tid) {
	const unsigned d = clo_op_min(tid * CLO_SEG_ITEMS, g.cnt);
	unsigned lo = d > g.nb ? d - g.nb : 0u, hi = clo_op_min(d, g.na);
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		if (s_end[mid] <= d - 1u - mid) lo = mid + 1u; else hi = mid;
	}
	clo_seg_lane l;
	l.a = lo; l.b = d - lo;
	s_start[tid] = lo;
	if (tid == 0u) s_start[CLO_SEG_THREADS] = g.na;
	__syncthreads();
	l.steps = clo_op_min((unsigned) CLO_SEG_ITEMS, g.cnt - d);
	l.ne = clo_op_min(clo_op_max(s_start[tid + 1u], l.a) - l.a, l.steps);
	l.nr = l.steps - l.ne;
	l.closes = 0u;
	return l;
}

// l.closes from CLO_SEG_ITEMS LDS reads that do not wait for each other: end a + j closes at step j + (the lane's rows
// before it), whatever the other ends are. each_end(j, the position read for end a + j) sees every read, those at
// j >= ne too (clamped below T, they are some position of the tile).
template <typename F>
__device__ __forceinline__ void clo_seg_lane_closes(clo_seg_lane& l, const unsigned short* s_end, F each_end) {
	unsigned closes = 0u;   // (a local, and the range and the ends by value above: the forms that keep the sweeps' instructions)
	#pragma unroll
	for (int j = 0; j < CLO_SEG_ITEMS; ++j) {
		const unsigned ea = s_end[clo_op_min(l.a + (unsigned) j, CLO_SEG_TILE - 1u)];
		const unsigned p = clo_op_min(ea > l.b ? ea - l.b : 0u, l.nr) + (unsigned) j;   // < steps where j < ne
		closes |= ((unsigned) j < l.ne ? 1u : 0u) << (p & 31u);
		each_end(j, ea);
	}
	l.closes = closes;
}
__device__ __forceinline__ void clo_seg_lane_closes(clo_seg_lane& l, const unsigned short* s_end) {
	clo_seg_lane_closes(l, s_end, [](int, unsigned) {});
}

// ---- the carry scan of clo_op_seg_state<TS> tile states ----

// One work-group: tile t gets the aggregate of the tiles before it that is still open, in place in tile_a
// (clo_rbk_states_kernel's walk, CLO_SEG_CARRY_TRIP states per trip); the next trip's states are requested before this
// trip's are combined. Both arrays are 256-byte aligned, so a thread's CLO_SEG_CARRY_ITEMS states go by 16-byte accesses
// where all of them exist.
template <typename TS, int OP>
__device__ __forceinline__ void clo_seg_carry(const unsigned* __restrict__ tile_h, clo_op_u64* __restrict__ tile_a, unsigned tiles) {
	__shared__ unsigned s_h[CLO_SEG_WAVES];
	__shared__ TS s_a[CLO_SEG_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	clo_op_seg_state<TS> running = clo_op_seg_empty<OP, TS>();   // the state of everything before this trip (the same in every thread)
	clo_op_seg_state<TS> ahead[CLO_SEG_CARRY_ITEMS];
	typedef unsigned vec4 __attribute__((ext_vector_type(4)));
	typedef clo_op_u64 vec2 __attribute__((ext_vector_type(2)));
	auto request = [&](unsigned first) {
		if (first + CLO_SEG_CARRY_ITEMS <= tiles) {   // `first` is a multiple of CLO_SEG_CARRY_ITEMS
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 4) {
				const vec4 h = *reinterpret_cast<const vec4*>(tile_h + first + j);
				ahead[j].h = h.x; ahead[j + 1].h = h.y; ahead[j + 2].h = h.z; ahead[j + 3].h = h.w;
			}
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 2) {
				const vec2 a = *reinterpret_cast<const vec2*>(tile_a + first + j);
				ahead[j].a = (TS) a.x; ahead[j + 1].a = (TS) a.y;
			}
		} else {
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
				ahead[j] = clo_op_seg_empty<OP, TS>();
				if (first + j < tiles) { ahead[j].h = tile_h[first + j]; ahead[j].a = (TS) tile_a[first + j]; }
			}
		}
	};
	request(tid * CLO_SEG_CARRY_ITEMS);
	for (unsigned chunk = 0; chunk < tiles; chunk += CLO_SEG_CARRY_TRIP) {
		const unsigned t0 = chunk + tid * CLO_SEG_CARRY_ITEMS;
		clo_op_seg_state<TS> st[CLO_SEG_CARRY_ITEMS];
		clo_op_seg_state<TS> mine = clo_op_seg_empty<OP, TS>();
		#pragma unroll
		for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
			st[j] = ahead[j];
			mine = clo_op_seg_combine<OP, true, TS>(mine, st[j]);
		}
		request(t0 + CLO_SEG_CARRY_TRIP);   // (this thread's own tiles of the next trip: nobody writes them before)
		const clo_op_seg_state<TS> incl = clo_op_seg_wave_scan<OP, true, TS>(mine);
		if (lane == 63u) { s_h[wave] = incl.h; s_a[wave] = incl.a; }
		__syncthreads();
		clo_op_seg_state<TS> before = running, all = running;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) CLO_SEG_WAVES; ++w) {
			clo_op_seg_state<TS> p;
			p.h = s_h[w]; p.a = s_a[w];
			if (w < wave) before = clo_op_seg_combine<OP, true, TS>(before, p);
			all = clo_op_seg_combine<OP, true, TS>(all, p);
		}
		clo_op_seg_state<TS> s = clo_op_seg_combine<OP, true, TS>(before, clo_op_seg_wave_exclusive<OP, true, TS>(incl, lane));
		clo_op_u64 out[CLO_SEG_CARRY_ITEMS];   // (tile_h is not needed again)
		#pragma unroll
		for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
			out[j] = (clo_op_u64) s.a;
			s = clo_op_seg_combine<OP, true, TS>(s, st[j]);
		}
		if (t0 + CLO_SEG_CARRY_ITEMS <= tiles) {
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 2) {
				vec2 a;
				a.x = out[j]; a.y = out[j + 1];
				*reinterpret_cast<vec2*>(tile_a + t0 + j) = a;
			}
		} else {
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) if (t0 + j < tiles) tile_a[t0 + j] = out[j];
		}
		running = all;
		__syncthreads();   // s_h / s_a are written again in the next trip
	}
}

}  // namespace

#endif
