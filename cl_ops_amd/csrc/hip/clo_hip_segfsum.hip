// clo_hip_segfsum.hip — the floating-point sum of every segment, the segments from counts or from CSR offsets
// (CloSegFSum, include/clo_segfsum.h; not upstream). With m = min(numel_seg, *num_in) segments whose ends
// are e_r (the running sums of the counts, or offsets[r + 1] - offsets[0]) and n rows of values:
//     sums_out[r] = the sum over i in [min(e_(r-1), n), min(e_r, n)) of (sum type) values_in[i],     +0 without a row,
// every addition one IEEE addition in the sum type (round to nearest even, nothing flushed), in the ORDER this file
// fixes and tests/segfsum_model.py restates: the order is the contract, and the bits of a sum depend on m, n and the
// clipped ends alone. half -> float, float -> float, float -> double, double -> double.
//
// The schedule is CloSegReduce's (clo_hip_segreduce.hip), the merge path of clo_hip_seg_device.h, which has its argument
// and the bounds of every read: ENDS, PARTITION, SWEEP, CARRY, FIXUP. The ends' launches, the partition, the tile clamp,
// the staged 16-bit end positions, the lanes' close masks, clo_op_stage and clo_op_store are that header's, unchanged.
// What is this file's is everything that adds, because the shared state, combine, DPP step and carry scan convert
// their aggregates by value, where a float needs its bits: floats cross lanes (DPP, shuffles) and lie in the workspace
// (tile_a, 64-bit words) as their bit patterns.
//   THE TREE   a lane walks its 17 steps from +0, left to right, starting over from +0 after a close (first walk);
//              the 64 lane states go through row_shr 1, 2, 4, 8, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows
//              2 and 3, each combine `r.h ? r.a : l.a + r.a` (a lane without a source adds +0, which changes no bit:
//              no partial sum is ever -0, since every one starts from +0); the four wave totals are combined left to
//              right; a lane's second walk starts from (waves before) (+) (lanes before) and adds its rows one by one,
//              storing at every close; the tiles' open aggregates go through the one-group carry scan (16 states per
//              thread left to right, the same network, four waves, the running state of the trips before FIRST); the
//              fix-up adds the carry to the first segment that closes in the tile: sums_out[r] = sums_out[r] + carry.
// No fast-math, no reassociation: this file is compiled like every other, and the additions are written one by one.
// values_in is read once. A lane closes at most na = a1 - a0 segments, so every write lands in sums_out[a0, a1), a1 <= m.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_seg_device.h"

namespace {

typedef clo_op_u64 fs_u64;

constexpr unsigned FS_NONE = 0xffffffffu;   // a tile in which no segment closes

// CloType numbers (clo_common.h)
constexpr int FS_HALF = 8, FS_FLOAT = 9, FS_DOUBLE = 10;

// ---- the four pairs: TR = a row as it lies in memory (its bits), TS = the sum type, cast = C's (TS) row, exact ----
enum { FS_H_F = 0, FS_F_F = 1, FS_F_D = 2, FS_D_D = 3 };
template <int PAIR> struct fs_pair;
template <> struct fs_pair<FS_H_F> {
	typedef uint16_t TR; typedef float TS;
	static __device__ __forceinline__ float cast(uint16_t r) { return (float) __builtin_bit_cast(_Float16, r); }
};
template <> struct fs_pair<FS_F_F> {
	typedef uint32_t TR; typedef float TS;
	static __device__ __forceinline__ float cast(uint32_t r) { return __uint_as_float(r); }
};
template <> struct fs_pair<FS_F_D> {
	typedef uint32_t TR; typedef double TS;
	static __device__ __forceinline__ double cast(uint32_t r) { return (double) __uint_as_float(r); }
};
template <> struct fs_pair<FS_D_D> {
	typedef uint64_t TR; typedef double TS;
	static __device__ __forceinline__ double cast(uint64_t r) { return __longlong_as_double((long long) r); }
};

inline int fs_pair_of(int value_type, int sum_type) {
	if (value_type == FS_HALF && sum_type == FS_FLOAT) return FS_H_F;
	if (value_type == FS_FLOAT && sum_type == FS_FLOAT) return FS_F_F;
	if (value_type == FS_FLOAT && sum_type == FS_DOUBLE) return FS_F_D;
	if (value_type == FS_DOUBLE && sum_type == FS_DOUBLE) return FS_D_D;
	return -1;
}

// ---- a sum as its bits ----
template <typename TS> struct fs_word;
template <> struct fs_word<float> {
	typedef unsigned TB;
	static __device__ __forceinline__ unsigned bits(float x) { return __float_as_uint(x); }
	static __device__ __forceinline__ float value(unsigned b) { return __uint_as_float(b); }
};
template <> struct fs_word<double> {
	typedef fs_u64 TB;
	static __device__ __forceinline__ fs_u64 bits(double x) { return (fs_u64) __double_as_longlong(x); }
	static __device__ __forceinline__ double value(fs_u64 b) { return __longlong_as_double((long long) b); }
};

// ---- the state of a stretch of steps: the closes in it, and the sum from its last close (from its start when it has
// none) to its end ----
template <typename TS>
struct fs_state { unsigned h; TS a; };

template <typename TS>
__device__ __forceinline__ fs_state<TS> fs_empty() { fs_state<TS> o; o.h = 0u; o.a = (TS) 0; return o; }

template <typename TS>
__device__ __forceinline__ fs_state<TS> fs_combine(const fs_state<TS>& l, const fs_state<TS>& r) {
	fs_state<TS> o;
	o.h = l.h + r.h;
	o.a = r.h ? r.a : l.a + r.a;
	return o;
}

// one step of the network: the state CTRL brings, (0, +0) where it brings none, joins from the left
template <int CTRL, int ROW_MASK, typename TS>
__device__ __forceinline__ void fs_step(fs_state<TS>& s) {
	typedef typename fs_word<TS>::TB TB;
	fs_state<TS> l;
	l.h = clo_op_dpp<CTRL, ROW_MASK, unsigned>(0u, s.h);
	l.a = fs_word<TS>::value(clo_op_dpp<CTRL, ROW_MASK, TB>((TB) 0, fs_word<TS>::bits(s.a)));
	s = fs_combine<TS>(l, s);
}

// inclusive segmented scan of the 64 lane states of a whole wave: clo_op_seg_wave_scan's network
template <typename TS>
__device__ __forceinline__ fs_state<TS> fs_wave_scan(fs_state<TS> s) {
	fs_step<0x111, 0xF, TS>(s);   // row_shr:1
	fs_step<0x112, 0xF, TS>(s);   // row_shr:2
	fs_step<0x114, 0xF, TS>(s);   // row_shr:4
	fs_step<0x118, 0xF, TS>(s);   // row_shr:8
	fs_step<0x142, 0xA, TS>(s);   // row_bcast:15 into rows 1 and 3
	fs_step<0x143, 0xC, TS>(s);   // row_bcast:31 into rows 2 and 3
	return s;
}

// the state of the lanes before this one: the inclusive scan moved up one lane
template <typename TS>
__device__ __forceinline__ fs_state<TS> fs_wave_exclusive(const fs_state<TS>& incl, unsigned lane) {
	typedef typename fs_word<TS>::TB TB;
	fs_state<TS> e;
	e.h = clo_op_shfl<unsigned>(incl.h, (int) lane - 1);
	e.a = fs_word<TS>::value(clo_op_shfl<TB>(fs_word<TS>::bits(incl.a), (int) lane - 1));
	return lane == 0 ? fs_empty<TS>() : e;
}

// ---- 1. the ends of the counts form: the three launches of clo_hip_seg_device.h ----

template <typename TC>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segfsum_sums_kernel(const TC* __restrict__ counts, const fs_u64* __restrict__ num_in, unsigned m_h, int vec_ok, fs_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segfsum_sums_scan_kernel(fs_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segfsum_ends_kernel(const TC* __restrict__ counts, const fs_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const fs_u64* __restrict__ tsum, fs_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. partition ----
template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segfsum_partition_kernel(const TC* __restrict__ src, const fs_u64* __restrict__ ends, const fs_u64* __restrict__ num_in, unsigned m_h,
	unsigned n, unsigned tiles, unsigned* __restrict__ split, fs_u64* __restrict__ num_out) {
	clo_seg_partition<TC, OFFSETS>(src, ends, num_in, m_h, n, tiles, split, num_out);
}

// numel_seg 0: there is nothing to read
__global__ void clo_segfsum_empty_kernel(fs_u64* __restrict__ num_out) { *num_out = 0ull; }

// ---- 3. tile sweep ----
template <typename TC, bool OFFSETS, int PAIR>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segfsum_sweep_kernel(const TC* __restrict__ src, const fs_u64* __restrict__ ends, const fs_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ split, const typename fs_pair<PAIR>::TR* __restrict__ values, typename fs_pair<PAIR>::TS* __restrict__ sums_out,
	unsigned* __restrict__ tile_h, unsigned* __restrict__ tile_first, fs_u64* __restrict__ tile_a) {
	typedef typename fs_pair<PAIR>::TR TR;
	typedef typename fs_pair<PAIR>::TS TS;
	// the tile's rows as they lie in memory until the lanes have walked them, then the sums of its segments
	__shared__ __attribute__((aligned(16))) TS s_val[CLO_SEG_TILE];
	__shared__ unsigned short s_end[CLO_SEG_TILE];   // positions in [0, nb], nb <= T: 16 bits, so that more groups fit a CU
	__shared__ unsigned s_start[CLO_SEG_THREADS + 1];
	__shared__ unsigned s_h[CLO_SEG_WAVES];
	__shared__ TS s_a[CLO_SEG_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);

	const clo_seg_steps st = clo_seg_tile_steps(m, n);
	if (st.cnt == 0u) {   // the whole work-group: beyond the last step (m < numel_seg)
		if (tid == 0u) { tile_h[blockIdx.x] = 0u; tile_first[blockIdx.x] = FS_NONE; tile_a[blockIdx.x] = 0ull; }   // (+0)
		return;
	}
	const clo_seg_range g = clo_seg_tile_clamp(st, split, m, n);
	const unsigned a0 = g.a0, na = g.na;

	clo_keyx kx;
	kx.sign = 0; kx.field = 0; kx.kind = 0;   // (not looked at: the rows are staged as they are)
	clo_op_stage<TR, false>(values + g.b0, g.nb, reinterpret_cast<TR*>(s_val), kx, tid);
	if (na > 0u) clo_seg_stage_ends<TC, OFFSETS>(clo_op_ends_make<TC, OFFSETS>(src, ends), g, n, s_end, tid);
	__syncthreads();
	clo_seg_lane l = clo_seg_lane_begin(g, s_end, s_start, tid);
	clo_seg_lane_closes(l, s_end);
	const unsigned b = l.b, steps = l.steps, closes = l.closes;
	// x[k] = the value of the row step k takes, +0 where it takes none: 17 reads that do not wait for each other.
	// The first walk: from +0, left to right, from +0 again after a close.
	const TR* s_row = reinterpret_cast<const TR*>(s_val);
	TS x[CLO_SEG_ITEMS];
	fs_state<TS> s = fs_empty<TS>();
	#pragma unroll
	for (int k = 0; k < CLO_SEG_ITEMS; ++k) {
		const bool close = (closes >> k) & 1u;
		const unsigned rs = (unsigned) k - (unsigned) __popc(closes & ((1u << k) - 1u));
		const TR raw = s_row[clo_op_min(b + rs, CLO_SEG_TILE - 1u)];
		x[k] = (!close && (unsigned) k < steps) ? fs_pair<PAIR>::cast(raw) : (TS) 0;
		s.h += close ? 1u : 0u;
		s.a = close ? (TS) 0 : s.a + x[k];
	}

	// the lanes' states through the segmented scan: the lanes, then the waves left to right
	const fs_state<TS> incl = fs_wave_scan<TS>(s);
	if (lane == 63u) { s_h[wave] = incl.h; s_a[wave] = incl.a; }
	__syncthreads();   // and every lane has its rows: s_val is free
	fs_state<TS> before = fs_empty<TS>(), all = fs_empty<TS>();
	#pragma unroll
	for (unsigned w = 0; w < (unsigned) CLO_SEG_WAVES; ++w) {
		fs_state<TS> p;
		p.h = s_h[w]; p.a = s_a[w];
		if (w < wave) before = fs_combine<TS>(before, p);
		all = fs_combine<TS>(all, p);
	}
	const fs_state<TS> in = fs_combine<TS>(before, fs_wave_exclusive<TS>(incl, lane));
	if (tid == 0u) {
		tile_h[blockIdx.x] = all.h ? 1u : 0u;
		tile_first[blockIdx.x] = na > 0u ? a0 : FS_NONE;
		tile_a[blockIdx.x] = (fs_u64) fs_word<TS>::bits(all.a);
	}
	if (na == 0u) return;   // the whole work-group

	// the second walk, from registers, with what was open before the lane: a close stores the segment's sum
	TS open = in.a;
	unsigned at = l.a;   // a step closes at most ne times, and l.a + ne <= na
	#pragma unroll
	for (int k = 0; k < CLO_SEG_ITEMS; ++k) {
		if ((closes >> k) & 1u) {
			s_val[at] = open;
			++at;
			open = (TS) 0;
		} else {
			open = open + x[k];
		}
	}
	__syncthreads();
	clo_op_store<TS>(sums_out + a0, na, tid, [&](unsigned i) { return s_val[i]; });
}

// ---- 4. carry scan: one group; tile t gets the open sum of the tiles before it, in place. clo_seg_carry's walk
// (clo_hip_seg_device.h) with this file's state, the sums as their bits in tile_a's 64-bit words ----
template <typename TS>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segfsum_carry_kernel(const unsigned* __restrict__ tile_h, fs_u64* __restrict__ tile_a, unsigned tiles) {
	typedef typename fs_word<TS>::TB TB;
	__shared__ unsigned s_h[CLO_SEG_WAVES];
	__shared__ TS s_a[CLO_SEG_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	fs_state<TS> running = fs_empty<TS>();   // the state of everything before this trip (the same in every thread)
	fs_state<TS> ahead[CLO_SEG_CARRY_ITEMS];
	typedef unsigned vec4 __attribute__((ext_vector_type(4)));
	typedef fs_u64 vec2 __attribute__((ext_vector_type(2)));
	auto request = [&](unsigned first) {
		if (first + CLO_SEG_CARRY_ITEMS <= tiles) {   // 16-byte loads: the arrays are 256-byte aligned, `first` a multiple of CLO_SEG_CARRY_ITEMS
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 4) {
				const vec4 h = *reinterpret_cast<const vec4*>(tile_h + first + j);
				ahead[j].h = h.x; ahead[j + 1].h = h.y; ahead[j + 2].h = h.z; ahead[j + 3].h = h.w;
			}
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 2) {
				const vec2 a = *reinterpret_cast<const vec2*>(tile_a + first + j);
				ahead[j].a = fs_word<TS>::value((TB) a.x); ahead[j + 1].a = fs_word<TS>::value((TB) a.y);
			}
		} else {
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
				ahead[j] = fs_empty<TS>();
				if (first + j < tiles) { ahead[j].h = tile_h[first + j]; ahead[j].a = fs_word<TS>::value((TB) tile_a[first + j]); }
			}
		}
	};
	request(tid * CLO_SEG_CARRY_ITEMS);
	for (unsigned chunk = 0; chunk < tiles; chunk += CLO_SEG_CARRY_TRIP) {
		const unsigned t0 = chunk + tid * CLO_SEG_CARRY_ITEMS;
		fs_state<TS> st[CLO_SEG_CARRY_ITEMS];
		fs_state<TS> mine = fs_empty<TS>();
		#pragma unroll
		for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {   // a thread's 16 states, left to right
			st[j] = ahead[j];
			mine = fs_combine<TS>(mine, st[j]);
		}
		request(t0 + CLO_SEG_CARRY_TRIP);   // (this thread's own tiles of the next trip: nobody writes them before)
		const fs_state<TS> incl = fs_wave_scan<TS>(mine);
		if (lane == 63u) { s_h[wave] = incl.h; s_a[wave] = incl.a; }
		__syncthreads();
		fs_state<TS> before = running, all = running;   // the trips before come FIRST
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) CLO_SEG_WAVES; ++w) {
			fs_state<TS> p;
			p.h = s_h[w]; p.a = s_a[w];
			if (w < wave) before = fs_combine<TS>(before, p);
			all = fs_combine<TS>(all, p);
		}
		fs_state<TS> s = fs_combine<TS>(before, fs_wave_exclusive<TS>(incl, lane));
		fs_u64 out[CLO_SEG_CARRY_ITEMS];   // (tile_h is not needed again)
		#pragma unroll
		for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
			out[j] = (fs_u64) fs_word<TS>::bits(s.a);
			s = fs_combine<TS>(s, st[j]);
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

// ---- 5. fix-up: the carry into tile t is added to the first segment that closes there (a segment closes in exactly
// one tile, so no two threads meet) ----
template <typename TS>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segfsum_fixup_kernel(const unsigned* __restrict__ tile_first, const fs_u64* __restrict__ tile_a, unsigned tiles, unsigned m_h,
	TS* __restrict__ sums_out) {
	typedef typename fs_word<TS>::TB TB;
	const unsigned t = blockIdx.x * CLO_SEG_THREADS + threadIdx.x;
	if (t >= tiles) return;
	const unsigned r = tile_first[t];
	if (r >= m_h) return;   // FS_NONE, or not a row of sums_out
	sums_out[r] = sums_out[r] + fs_word<TS>::value((TB) tile_a[t]);
}

// The workspace is CloSegReduce's: the ends of the counts form, the tile boundaries' splits, the tiles' three words, the
// sums of the ends' scan. Laid out from `base`, or only measured where that is null; returns the size.
struct fs_ws { fs_u64* ends; unsigned* split; unsigned* tile_h; unsigned* tile_first; fs_u64* tile_a; fs_u64* tsum; };

inline size_t fs_layout(fs_ws& w, char* base, size_t numel_seg, size_t numel) {
	const size_t tiles = clo_seg_tiles(numel_seg, numel);
	size_t at = 0;
	w.ends = clo_op_ws_take<fs_u64>(base, at, numel_seg);
	w.split = clo_op_ws_take<unsigned>(base, at, tiles + 1);
	w.tile_h = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tile_first = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tile_a = clo_op_ws_take<fs_u64>(base, at, tiles);
	w.tsum = clo_op_ws_take<fs_u64>(base, at, clo_op_ends_tiles(numel_seg) + 1);
	return at;
}

struct fs_args : fs_ws {
	const void* src; const fs_u64* num_in; const void* vin; void* sums; fs_u64* num_out;
	unsigned m_h, n; hipStream_t s;
};

constexpr const char* FS_ENDS_LABELS[3] = { "segfsum_sums", "segfsum_sums_scan", "segfsum_ends" };

template <typename TC, bool OFFSETS, int PAIR>
int fs_launch(const fs_args& a) {
	typedef typename fs_pair<PAIR>::TR TR;
	typedef typename fs_pair<PAIR>::TS TS;
	if constexpr (!OFFSETS) {
		const int st = clo_op_ends_launch<TC>(clo_segfsum_sums_kernel<TC>, clo_segfsum_sums_scan_kernel, clo_segfsum_ends_kernel<TC>, FS_ENDS_LABELS,
			a.src, a.num_in, a.m_h, a.tsum, a.ends, a.s);
		if (st != 0) return st;
	}
	const unsigned tiles = (unsigned) clo_seg_tiles(a.m_h, a.n);   // >= 1: m_h > 0
	{
		clo_timing_scope timing("segfsum_partition", a.s);
		hipLaunchKernelGGL((clo_segfsum_partition_kernel<TC, OFFSETS>), dim3(tiles / CLO_SEG_THREADS + 1u), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const fs_u64*) a.ends, a.num_in, a.m_h, a.n, tiles, a.split, a.num_out);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segfsum_sweep", a.s);
		hipLaunchKernelGGL((clo_segfsum_sweep_kernel<TC, OFFSETS, PAIR>), dim3(tiles), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const fs_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TR*) a.vin, (TS*) a.sums,
			a.tile_h, a.tile_first, a.tile_a);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segfsum_carry", a.s);
		hipLaunchKernelGGL((clo_segfsum_carry_kernel<TS>), dim3(1), dim3(CLO_SEG_THREADS), 0, a.s, (const unsigned*) a.tile_h, a.tile_a, tiles);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segfsum_fixup", a.s);
	hipLaunchKernelGGL((clo_segfsum_fixup_kernel<TS>), dim3((tiles + CLO_SEG_THREADS - 1u) / CLO_SEG_THREADS), dim3(CLO_SEG_THREADS), 0, a.s,
		(const unsigned*) a.tile_first, (const fs_u64*) a.tile_a, tiles, a.m_h, (TS*) a.sums);
	return (int) hipGetLastError();
}

template <typename TC, bool OFFSETS>
int fs_dispatch_pair(const fs_args& a, int pair) {
	switch (pair) {
		case FS_H_F: return fs_launch<TC, OFFSETS, FS_H_F>(a);
		case FS_F_F: return fs_launch<TC, OFFSETS, FS_F_F>(a);
		case FS_F_D: return fs_launch<TC, OFFSETS, FS_F_D>(a);
		case FS_D_D: return fs_launch<TC, OFFSETS, FS_D_D>(a);
		default: return CLO_HIP_EUNSUPPORTED;
	}
}

template <typename TC>
int fs_dispatch(const fs_args& a, int form, int pair) {
	return form == CLO_HIP_SEGFSUM_OFFSETS ? fs_dispatch_pair<TC, true>(a, pair) : fs_dispatch_pair<TC, false>(a, pair);
}

}  // namespace

extern "C" {

size_t clo_hip_segfsum_tile(int value_size, int sum_size) {
	return ((value_size == 2 && sum_size == 4) || (value_size == 4 && sum_size == 4) || (value_size == 4 && sum_size == 8)
		|| (value_size == 8 && sum_size == 8)) ? CLO_SEG_TILE : 0;
}

size_t clo_hip_segfsum_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	fs_ws w;
	return fs_layout(w, nullptr, numel_seg, numel);
}

int clo_hip_segfsum(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* sums_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (form != CLO_HIP_SEGFSUM_COUNTS && form != CLO_HIP_SEGFSUM_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int pair = fs_pair_of(value_type, sum_type);
	if (pair < 0) return CLO_HIP_EUNSUPPORTED;
	const size_t vs = value_type == FS_HALF ? 2 : value_type == FS_FLOAT ? 4 : 8, ss = sum_type == FS_FLOAT ? 4 : 8;
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGFSUM_OFFSETS)) return CLO_HIP_EARGS;
	if (!values_in && numel > 0) return CLO_HIP_EARGS;
	if (!sums_out && numel_seg > 0) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8) || clo_misaligned(num_in, 8)) return CLO_HIP_EARGS;
	if (clo_misaligned(counts_or_offsets, (size_t) count_size) || clo_misaligned(values_in, vs) || clo_misaligned(sums_out, ss)) return CLO_HIP_EARGS;
	if (numel_seg == 0) {
		hipLaunchKernelGGL(clo_segfsum_empty_kernel, dim3(1), dim3(1), 0, (hipStream_t) stream, (fs_u64*) num_out);
		return (int) hipGetLastError();
	}
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_segfsum_workspace_bytes(numel_seg, numel)) return CLO_HIP_EWORKSPACE;

	fs_args a;
	a.src = counts_or_offsets; a.num_in = (const fs_u64*) num_in; a.vin = values_in; a.sums = sums_out; a.num_out = (fs_u64*) num_out;
	a.m_h = (unsigned) numel_seg; a.n = (unsigned) numel; a.s = (hipStream_t) stream;
	fs_layout(a, (char*) workspace, numel_seg, numel);
	return count_size == 8 ? fs_dispatch<uint64_t>(a, form, pair) : fs_dispatch<uint32_t>(a, form, pair);
}

}  // extern "C"
