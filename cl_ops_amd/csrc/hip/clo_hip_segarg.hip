// clo_hip_segarg.hip — arg-min and arg-max per segment from counts or from CSR offsets (CloSegArg, include/clo_segarg.h;
// not upstream). With m = min(numel_seg, *num_in) segments whose ends are e_r and n rows of values, x(i)
// the order key of values_in[i] (clo_keyx_fwd; complemented for argmax):
//     idx_out[r] = the row i in [min(e_(r-1), n), min(e_r, n)) with the smallest (x(i), i) for `first`, (x(i), ~i) for `last`,
//     val_out[r] = values_in[idx_out[r]];     CLO_SEGARG_NONE and the key that comes last in the order without a row.
//
// The schedule is the merge path of clo_hip_seg_device.h, which has its argument and the bounds of every read, with
// CloSegReduce's launches (§21): ENDS (counts form), PARTITION, SWEEP, CARRY, FIXUP. What is this file's:
//   the aggregate  is (order key, j) with j = i for `first` and ~i for `last`, the smaller of two winning and the LEFT one on
//                  full equality. 4-byte values: one 64-bit word (x << 32) | j under an unsigned minimum. 8-byte values:
//                  a 64-bit key and a 32-bit j compared lexicographically. A row's index is where it lies in the merge
//                  (b0 + b + rs), so LDS stages the values alone, as they are.
//   val_out        is CARRIED, not gathered: the key is a bijection of the value's bits, so clo_keyx_inv of the winning
//                  key is values_in[idx] bit for bit and no second read of values_in is made.
//   the stretch    a tile writes: idx_out[a0, a1) and val_out[a0, a1). Every segment that closes in a tile after the
//                  first has all its rows in the tile, so its index is staged in LDS as a 16-bit position in the tile —
//                  in the array the ends' positions lay in, which nobody reads any more — and LDS is §21's: the values
//                  and two bytes per step.
//   an empty segment is known from its ENDS, never from the aggregate: in the sweep two neighbouring positions that are
//                  equal, in the fix-up the two clipped ends. A row that holds the last key of the order (row 0 under
//                  `last` packs to the all-ones word, the identity) is therefore still reported: the minimum with the
//                  identity is that row's own word.
//   the fix-up     rewrites the first segment that closes in every tile from (the carry into the tile) min (what the tile
//                  holds of it), the latter left in the workspace by the sweep: an index does not say what key it had.
// A lane closes at most na = a1 - a0 segments, so every write lands in idx_out[a0, a1) and val_out[a0, a1), a1 <= m; the
// fix-up writes row tile_first < a1 <= m; val_out is decoded from a key, so a wrong index is never dereferenced.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_seg_device.h"

namespace {

typedef clo_op_u64 arg_u64;

constexpr unsigned ARG_NOPOS = 0xffffu;                         // a closing segment without a row, among the 16-bit positions
static_assert(CLO_SEG_TILE < ARG_NOPOS, "a row's position in its tile is kept in 16 bits, and one value says `none`");
constexpr unsigned ARG_NONE = 0xffffffffu;                      // CLO_SEGARG_NONE; also: a tile in which no segment closes

// ---- the aggregate: (order key, j), the smaller wins, the left one on full equality ----
template <int VS> struct arg_agg;
template <> struct arg_agg<4> {
	typedef uint32_t TV;
	arg_u64 p;   // (x << 32) | j
	__device__ __forceinline__ static arg_agg make(TV x, unsigned j) { arg_agg o; o.p = ((arg_u64) x << 32) | j; return o; }
	__device__ __forceinline__ static arg_agg identity() { arg_agg o; o.p = ~0ull; return o; }
	__device__ __forceinline__ static arg_agg words(arg_u64 x, unsigned) { arg_agg o; o.p = x; return o; }   // as the workspace holds it
	__device__ __forceinline__ arg_u64 word() const { return p; }
	__device__ __forceinline__ TV key() const { return (TV) (p >> 32); }
	__device__ __forceinline__ unsigned j() const { return (unsigned) p; }
	__device__ __forceinline__ bool less(const arg_agg& b) const { return p < b.p; }
	template <int CTRL, int ROW_MASK>
	__device__ __forceinline__ arg_agg dpp() const { arg_agg o; o.p = clo_op_dpp<CTRL, ROW_MASK, arg_u64>(~0ull, p); return o; }
	__device__ __forceinline__ arg_agg shfl(int lane) const { arg_agg o; o.p = clo_op_shfl<arg_u64>(p, lane); return o; }
};
template <> struct arg_agg<8> {
	typedef arg_u64 TV;
	arg_u64 x;
	unsigned jj;
	__device__ __forceinline__ static arg_agg make(TV x, unsigned j) { arg_agg o; o.x = x; o.jj = j; return o; }
	__device__ __forceinline__ static arg_agg identity() { arg_agg o; o.x = ~0ull; o.jj = ~0u; return o; }
	__device__ __forceinline__ static arg_agg words(arg_u64 x, unsigned j) { arg_agg o; o.x = x; o.jj = j; return o; }
	__device__ __forceinline__ arg_u64 word() const { return x; }
	__device__ __forceinline__ TV key() const { return x; }
	__device__ __forceinline__ unsigned j() const { return jj; }
	__device__ __forceinline__ bool less(const arg_agg& b) const { return x < b.x || (x == b.x && jj < b.jj); }
	template <int CTRL, int ROW_MASK>
	__device__ __forceinline__ arg_agg dpp() const {
		arg_agg o;
		o.x = clo_op_dpp<CTRL, ROW_MASK, arg_u64>(~0ull, x);
		o.jj = clo_op_dpp<CTRL, ROW_MASK, unsigned>(~0u, jj);
		return o;
	}
	__device__ __forceinline__ arg_agg shfl(int lane) const { arg_agg o; o.x = clo_op_shfl<arg_u64>(x, lane); o.jj = clo_op_shfl<unsigned>(jj, lane); return o; }
};

template <typename A>
__device__ __forceinline__ A arg_best(const A& l, const A& r) { return r.less(l) ? r : l; }   // l on full equality

// The state of a stretch of merge steps: the closes in it, and the aggregate of the rows after its last close (clo_op_seg_state's meaning).
template <typename A> struct arg_state { unsigned h; A a; };

template <typename A>
__device__ __forceinline__ arg_state<A> arg_empty() { arg_state<A> o; o.h = 0u; o.a = A::identity(); return o; }
template <typename A>
__device__ __forceinline__ arg_state<A> arg_combine(const arg_state<A>& l, const arg_state<A>& r) {
	arg_state<A> o;
	o.h = l.h + r.h;
	o.a = r.h ? r.a : arg_best<A>(l.a, r.a);
	return o;
}
template <int CTRL, int ROW_MASK, typename A>
__device__ __forceinline__ void arg_step(arg_state<A>& s) {
	arg_state<A> l;
	l.h = clo_op_dpp<CTRL, ROW_MASK, unsigned>(0u, s.h);
	l.a = s.a.template dpp<CTRL, ROW_MASK>();
	s = arg_combine<A>(l, s);
}
// inclusive segmented scan of the 64 lane states: clo_op_seg_wave_scan's network
template <typename A>
__device__ __forceinline__ arg_state<A> arg_wave_scan(arg_state<A> s) {
	arg_step<0x111, 0xF, A>(s);   // row_shr:1
	arg_step<0x112, 0xF, A>(s);   // row_shr:2
	arg_step<0x114, 0xF, A>(s);   // row_shr:4
	arg_step<0x118, 0xF, A>(s);   // row_shr:8
	arg_step<0x142, 0xA, A>(s);   // row_bcast:15 into rows 1 and 3
	arg_step<0x143, 0xC, A>(s);   // row_bcast:31 into rows 2 and 3
	return s;
}
template <typename A>
__device__ __forceinline__ arg_state<A> arg_wave_exclusive(const arg_state<A>& incl, unsigned lane) {
	arg_state<A> e;
	e.h = clo_op_shfl<unsigned>(incl.h, (int) lane - 1);
	e.a = incl.a.shfl((int) lane - 1);
	return lane == 0 ? arg_empty<A>() : e;
}

// the states of the work-group's waves in LDS: what lies before this wave, and all of them, from `from`
template <typename A>
struct arg_waves {
	unsigned h[CLO_SEG_WAVES]; arg_u64 x[CLO_SEG_WAVES]; unsigned j[CLO_SEG_WAVES];
	__device__ __forceinline__ void put(unsigned wave, const arg_state<A>& s) { h[wave] = s.h; x[wave] = s.a.word(); j[wave] = s.a.j(); }
	struct both { arg_state<A> before, all; };
	__device__ __forceinline__ both get(unsigned wave, const arg_state<A>& from) const {
		both o;
		o.before = from; o.all = from;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) CLO_SEG_WAVES; ++w) {
			arg_state<A> p;
			p.h = h[w]; p.a = A::words(x[w], j[w]);
			if (w < wave) o.before = arg_combine<A>(o.before, p);
			o.all = arg_combine<A>(o.all, p);
		}
		return o;
	}
};

// what the kernels know of the call: how a value becomes its key and back
struct arg_key {
	clo_keyx kx;
	arg_u64 cmpl;   // all ones for argmax
};
template <typename TV>
__device__ __forceinline__ TV arg_key_of(TV v, const arg_key& k) { return (TV) (clo_keyx_fwd<TV>(v, k.kx) ^ (TV) k.cmpl); }
template <typename TV>
__device__ __forceinline__ TV arg_value_of(TV x, const arg_key& k) { return clo_keyx_inv<TV>((TV) (x ^ (TV) k.cmpl), k.kx); }

// ---- 1. the ends of the counts form: the three launches of clo_hip_seg_device.h ----

template <typename TC>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segarg_sums_kernel(const TC* __restrict__ counts, const arg_u64* __restrict__ num_in, unsigned m_h, int vec_ok, arg_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segarg_sums_scan_kernel(arg_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segarg_ends_kernel(const TC* __restrict__ counts, const arg_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const arg_u64* __restrict__ tsum, arg_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. partition ----
template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segarg_partition_kernel(const TC* __restrict__ src, const arg_u64* __restrict__ ends, const arg_u64* __restrict__ num_in, unsigned m_h,
	unsigned n, unsigned tiles, unsigned* __restrict__ split, arg_u64* __restrict__ num_out) {
	clo_seg_partition<TC, OFFSETS>(src, ends, num_in, m_h, n, tiles, split, num_out);
}

// numel_seg 0: there is nothing to read
__global__ void clo_segarg_empty_kernel(arg_u64* __restrict__ num_out) { *num_out = 0ull; }

// what a tile leaves in the workspace
struct arg_tile_ws {
	unsigned* h;        // whether a segment closes in the tile
	unsigned* first;    // the first segment that closes in it, ARG_NONE without one
	arg_u64* ax;        // the aggregate of its rows after its last close; after the carry scan: of the rows BEFORE the tile that are still open
	unsigned* aj;       // (the index word of 8-byte values; the 4-byte aggregate is ax alone)
	arg_u64* px;        // the aggregate of the rows the tile holds of segment `first`
	unsigned* pj;
};

// ---- 3. tile sweep ----
template <typename TC, bool OFFSETS, int VS, bool LAST>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segarg_sweep_kernel(const TC* __restrict__ src, const arg_u64* __restrict__ ends, const arg_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ split, const typename arg_agg<VS>::TV* __restrict__ values, unsigned* __restrict__ idx_out,
	typename arg_agg<VS>::TV* __restrict__ val_out, arg_key key, arg_tile_ws tw) {
	typedef arg_agg<VS> A;
	typedef typename A::TV TV;
	// the tile's rows as they lie in memory until the lanes have walked them, then the values of its segments
	__shared__ __attribute__((aligned(16))) TV s_val[CLO_SEG_TILE];
	// the ends' positions in [0, nb], nb <= T, until the lanes know their steps; then the winning rows' positions
	__shared__ unsigned short s_end[CLO_SEG_TILE];
	__shared__ unsigned s_start[CLO_SEG_THREADS + 1];
	__shared__ arg_waves<A> s_waves;
	__shared__ arg_u64 s_px;
	__shared__ unsigned s_pj;
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);

	const clo_seg_steps st = clo_seg_tile_steps(m, n);
	if (st.cnt == 0u) {   // the whole work-group: beyond the last step (m < numel_seg)
		if (tid == 0u) { tw.h[blockIdx.x] = 0u; tw.first[blockIdx.x] = ARG_NONE; tw.ax[blockIdx.x] = ~0ull; tw.aj[blockIdx.x] = ~0u; }
		return;
	}
	const clo_seg_range g = clo_seg_tile_clamp(st, split, m, n);
	const unsigned a0 = g.a0, na = g.na;
	const arg_u64 b0 = g.b0;

	clo_keyx raw_kx;
	raw_kx.sign = 0; raw_kx.field = 0; raw_kx.kind = 0;   // (not looked at: the rows are staged as they are)
	clo_op_stage<TV, false>(values + b0, g.nb, s_val, raw_kx, tid);
	if (na > 0u) clo_seg_stage_ends<TC, OFFSETS>(clo_op_ends_make<TC, OFFSETS>(src, ends), g, n, s_end, tid);
	__syncthreads();
	clo_seg_lane l = clo_seg_lane_begin(g, s_end, s_start, tid);
	unsigned has_row = 0u;   // bit j = the lane's j-th closing segment has a row in the tile: its end lies behind the end before it
	unsigned before = l.a > 0u ? s_end[clo_op_min(l.a - 1u, CLO_SEG_TILE - 1u)] : 0u;   // (the tile's first segment: behind the tile's first row)
	clo_seg_lane_closes(l, s_end, [&](int j, unsigned ea) {
		has_row |= (ea > before ? 1u : 0u) << j;
		before = ea;
	});
	const unsigned b = l.b, steps = l.steps, closes = l.closes;
	// x[k] = (key, j) of the row step k takes, the identity where it takes none: 17 reads that do not wait for each other
	A x[CLO_SEG_ITEMS];
	arg_state<A> s = arg_empty<A>();
	#pragma unroll
	for (int k = 0; k < CLO_SEG_ITEMS; ++k) {
		const bool close = (closes >> k) & 1u;
		const unsigned rs = (unsigned) k - (unsigned) __popc(closes & ((1u << k) - 1u));
		const TV raw = s_val[clo_op_min(b + rs, CLO_SEG_TILE - 1u)];
		const unsigned i = (unsigned) b0 + b + rs;   // the row's index in values_in: < n where the step takes a row
		x[k] = (!close && (unsigned) k < steps) ? A::make(arg_key_of<TV>(raw, key), LAST ? ~i : i) : A::identity();
		s.h += close ? 1u : 0u;
		s.a = close ? A::identity() : arg_best<A>(s.a, x[k]);
	}

	// the lanes' states through the segmented scan: the lanes, then the waves
	const arg_state<A> incl = arg_wave_scan<A>(s);
	if (lane == 63u) s_waves.put(wave, incl);
	__syncthreads();   // and every lane has its rows and its ends: s_val and s_end are free
	const typename arg_waves<A>::both waves = s_waves.get(wave, arg_empty<A>());
	const arg_state<A>& all = waves.all;
	const arg_state<A> in = arg_combine<A>(waves.before, arg_wave_exclusive<A>(incl, lane));
	if (tid == 0u) {
		tw.h[blockIdx.x] = all.h ? 1u : 0u;
		tw.first[blockIdx.x] = na > 0u ? a0 : ARG_NONE;
		tw.ax[blockIdx.x] = all.a.word();
		tw.aj[blockIdx.x] = all.a.j();
	}
	if (na == 0u) return;   // the whole work-group

	// the walk again, from registers, with what was open before the lane: a close stores the segment's winner
	A open = in.a;
	unsigned at = l.a;   // a step closes at most ne times, and l.a + ne <= na
	unsigned nth = 0u;
	const TV none_val = arg_value_of<TV>((TV) ~(TV) 0, key);
	#pragma unroll
	for (int k = 0; k < CLO_SEG_ITEMS; ++k) {
		if ((closes >> k) & 1u) {
			const bool full = (has_row >> nth) & 1u;
			const unsigned i = LAST ? ~open.j() : open.j();
			s_end[at] = (unsigned short) (full ? i - (unsigned) b0 : ARG_NOPOS);   // a row of the tile: below nb
			if (val_out) s_val[at] = full ? arg_value_of<TV>(open.key(), key) : none_val;
			if (at == 0u) { s_px = open.word(); s_pj = open.j(); }   // one lane: the tile's first segment joins the carry in the fix-up
			++at; ++nth;
			open = A::identity();
		} else {
			open = arg_best<A>(open, x[k]);
		}
	}
	__syncthreads();
	if (tid == 0u) { tw.px[blockIdx.x] = s_px; tw.pj[blockIdx.x] = s_pj; }
	clo_op_store<unsigned>(idx_out + a0, na, tid, [&](unsigned i) { const unsigned p = s_end[i]; return p == ARG_NOPOS ? ARG_NONE : (unsigned) b0 + p; });
	if (val_out) clo_op_store<TV>(val_out + a0, na, tid, [&](unsigned i) { return s_val[i]; });
}

// ---- 4. carry scan: one group; tile t gets the state of the tiles before it, in place. clo_seg_carry's walk
// (clo_hip_seg_device.h) with this file's aggregate, held as three arrays of words ----
template <int VS>
__global__ __launch_bounds__(CLO_SEG_THREADS) __attribute__((amdgpu_waves_per_eu(1, 2)))   // one work-group: its registers hold two trips' states
void clo_segarg_carry_kernel(arg_tile_ws tw, unsigned tiles) {
	typedef arg_agg<VS> A;
	__shared__ arg_waves<A> s_waves;
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	arg_state<A> running = arg_empty<A>();   // the state of everything before this trip (the same in every thread)
	// (three arrays of words, not one of states: they stay in registers)
	unsigned ahead_h[CLO_SEG_CARRY_ITEMS], ahead_j[CLO_SEG_CARRY_ITEMS];
	arg_u64 ahead_x[CLO_SEG_CARRY_ITEMS];
	typedef unsigned vec4 __attribute__((ext_vector_type(4)));
	typedef arg_u64 vec2 __attribute__((ext_vector_type(2)));
	auto request = [&](unsigned first) {
		if (first + CLO_SEG_CARRY_ITEMS <= tiles) {   // 16-byte loads: the arrays are 256-byte aligned, `first` a multiple of CLO_SEG_CARRY_ITEMS
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 4) {
				const vec4 h = *reinterpret_cast<const vec4*>(tw.h + first + j);
				ahead_h[j] = h.x; ahead_h[j + 1] = h.y; ahead_h[j + 2] = h.z; ahead_h[j + 3] = h.w;
				vec4 jj = { ~0u, ~0u, ~0u, ~0u };
				if (VS == 8) jj = *reinterpret_cast<const vec4*>(tw.aj + first + j);
				ahead_j[j] = jj.x; ahead_j[j + 1] = jj.y; ahead_j[j + 2] = jj.z; ahead_j[j + 3] = jj.w;
			}
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 2) {
				const vec2 x = *reinterpret_cast<const vec2*>(tw.ax + first + j);
				ahead_x[j] = x.x; ahead_x[j + 1] = x.y;
			}
		} else {
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
				const bool in = first + j < tiles;
				ahead_h[j] = in ? tw.h[first + j] : 0u;
				ahead_x[j] = in ? tw.ax[first + j] : ~0ull;
				ahead_j[j] = in && VS == 8 ? tw.aj[first + j] : ~0u;
			}
		}
	};
	request(tid * CLO_SEG_CARRY_ITEMS);
	for (unsigned chunk = 0; chunk < tiles; chunk += CLO_SEG_CARRY_TRIP) {
		const unsigned t0 = chunk + tid * CLO_SEG_CARRY_ITEMS;
		arg_state<A> st[CLO_SEG_CARRY_ITEMS];
		arg_state<A> mine = arg_empty<A>();
		#pragma unroll
		for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
			st[j].h = ahead_h[j];
			st[j].a = A::words(ahead_x[j], ahead_j[j]);
			mine = arg_combine<A>(mine, st[j]);
		}
		request(t0 + CLO_SEG_CARRY_TRIP);   // (this thread's own tiles of the next trip: nobody writes them before)
		const arg_state<A> incl = arg_wave_scan<A>(mine);
		if (lane == 63u) s_waves.put(wave, incl);
		__syncthreads();
		const typename arg_waves<A>::both waves = s_waves.get(wave, running);
		arg_state<A> s = arg_combine<A>(waves.before, arg_wave_exclusive<A>(incl, lane));
		arg_u64 out_x[CLO_SEG_CARRY_ITEMS];   // (tw.h is not needed again)
		unsigned out_j[CLO_SEG_CARRY_ITEMS];
		#pragma unroll
		for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
			out_x[j] = s.a.word(); out_j[j] = s.a.j();
			s = arg_combine<A>(s, st[j]);
		}
		if (t0 + CLO_SEG_CARRY_ITEMS <= tiles) {
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 2) {
				vec2 x;
				x.x = out_x[j]; x.y = out_x[j + 1];
				*reinterpret_cast<vec2*>(tw.ax + t0 + j) = x;
			}
			if (VS == 8) {
				#pragma unroll
				for (int j = 0; j < CLO_SEG_CARRY_ITEMS; j += 4) {
					vec4 jj;
					jj.x = out_j[j]; jj.y = out_j[j + 1]; jj.z = out_j[j + 2]; jj.w = out_j[j + 3];
					*reinterpret_cast<vec4*>(tw.aj + t0 + j) = jj;
				}
			}
		} else {
			#pragma unroll
			for (int j = 0; j < CLO_SEG_CARRY_ITEMS; ++j) {
				if (t0 + j < tiles) {
					tw.ax[t0 + j] = out_x[j];
					if (VS == 8) tw.aj[t0 + j] = out_j[j];
				}
			}
		}
		running = waves.all;
		__syncthreads();   // s_waves is written again in the next trip
	}
}

// ---- 5. fix-up: the first segment that closes in tile t = (the carry into the tile) best (what the tile holds of it);
// whether it has a row at all comes from its clipped ends. (A segment closes in exactly one tile, so no two threads meet.) ----
template <typename TC, bool OFFSETS, int VS, bool LAST>
__global__ __launch_bounds__(CLO_SEG_THREADS)
void clo_segarg_fixup_kernel(const TC* __restrict__ src, const arg_u64* __restrict__ ends, const arg_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	arg_tile_ws tw, unsigned tiles, unsigned* __restrict__ idx_out, typename arg_agg<VS>::TV* __restrict__ val_out, arg_key key) {
	typedef arg_agg<VS> A;
	typedef typename A::TV TV;
	const unsigned t = blockIdx.x * CLO_SEG_THREADS + threadIdx.x;
	if (t >= tiles) return;
	const unsigned r = tw.first[t];
	if (r >= clo_op_segments(num_in, m_h)) return;   // ARG_NONE, or not a segment
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	const arg_u64 from = r > 0u ? clo_op_min64(e.at(r - 1u), n) : 0ull, to = clo_op_min64(e.at(r), n);
	const A best = arg_best<A>(A::words(tw.ax[t], tw.aj[t]), A::words(tw.px[t], tw.pj[t]));   // the carry lies to the left
	const bool full = to > from;
	idx_out[r] = full ? (LAST ? ~best.j() : best.j()) : ARG_NONE;
	if (val_out) val_out[r] = arg_value_of<TV>(full ? best.key() : (TV) ~(TV) 0, key);
}

// The workspace: the ends of the counts form, the tile boundaries' splits, the tiles' four 32-bit and two 64-bit words,
// the sums of the ends' scan. Laid out from `base`, or only measured where that is null; returns the size.
struct arg_ws { arg_u64* ends; unsigned* split; arg_tile_ws tw; arg_u64* tsum; };

inline size_t arg_layout(arg_ws& w, char* base, size_t numel_seg, size_t numel) {
	const size_t tiles = clo_seg_tiles(numel_seg, numel);
	size_t at = 0;
	w.ends = clo_op_ws_take<arg_u64>(base, at, numel_seg);
	w.split = clo_op_ws_take<unsigned>(base, at, tiles + 1);
	w.tw.h = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tw.first = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tw.aj = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tw.pj = clo_op_ws_take<unsigned>(base, at, tiles);
	w.tw.ax = clo_op_ws_take<arg_u64>(base, at, tiles);
	w.tw.px = clo_op_ws_take<arg_u64>(base, at, tiles);
	w.tsum = clo_op_ws_take<arg_u64>(base, at, clo_op_ends_tiles(numel_seg) + 1);
	return at;
}

struct arg_args : arg_ws {
	const void* src; const arg_u64* num_in; const void* vin; unsigned* idx; void* val; arg_u64* num_out;
	unsigned m_h, n; arg_key key; hipStream_t s;
};

constexpr const char* ARG_ENDS_LABELS[3] = { "segarg_sums", "segarg_sums_scan", "segarg_ends" };

template <typename TC, bool OFFSETS, int VS, bool LAST>
int arg_launch(const arg_args& a) {
	typedef typename arg_agg<VS>::TV TV;
	if constexpr (!OFFSETS) {
		const int st = clo_op_ends_launch<TC>(clo_segarg_sums_kernel<TC>, clo_segarg_sums_scan_kernel, clo_segarg_ends_kernel<TC>, ARG_ENDS_LABELS,
			a.src, a.num_in, a.m_h, a.tsum, a.ends, a.s);
		if (st != 0) return st;
	}
	const unsigned tiles = (unsigned) clo_seg_tiles(a.m_h, a.n);   // >= 1: m_h > 0
	{
		clo_timing_scope timing("segarg_partition", a.s);
		hipLaunchKernelGGL((clo_segarg_partition_kernel<TC, OFFSETS>), dim3(tiles / CLO_SEG_THREADS + 1u), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const arg_u64*) a.ends, a.num_in, a.m_h, a.n, tiles, a.split, a.num_out);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segarg_sweep", a.s);
		hipLaunchKernelGGL((clo_segarg_sweep_kernel<TC, OFFSETS, VS, LAST>), dim3(tiles), dim3(CLO_SEG_THREADS), 0, a.s,
			(const TC*) a.src, (const arg_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.split, (const TV*) a.vin, a.idx, (TV*) a.val, a.key, a.tw);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segarg_carry", a.s);
		hipLaunchKernelGGL((clo_segarg_carry_kernel<VS>), dim3(1), dim3(CLO_SEG_THREADS), 0, a.s, a.tw, tiles);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segarg_fixup", a.s);
	hipLaunchKernelGGL((clo_segarg_fixup_kernel<TC, OFFSETS, VS, LAST>), dim3((tiles + CLO_SEG_THREADS - 1u) / CLO_SEG_THREADS), dim3(CLO_SEG_THREADS), 0, a.s,
		(const TC*) a.src, (const arg_u64*) a.ends, a.num_in, a.m_h, a.n, a.tw, tiles, a.idx, (TV*) a.val, a.key);
	return (int) hipGetLastError();
}

template <typename TC, bool OFFSETS>
int arg_dispatch_form(const arg_args& a, int vs, int tie) {
	if (vs == 4) return tie == CLO_HIP_SEGARG_LAST ? arg_launch<TC, OFFSETS, 4, true>(a) : arg_launch<TC, OFFSETS, 4, false>(a);
	return tie == CLO_HIP_SEGARG_LAST ? arg_launch<TC, OFFSETS, 8, true>(a) : arg_launch<TC, OFFSETS, 8, false>(a);
}

template <typename TC>
int arg_dispatch(const arg_args& a, int form, int vs, int tie) {
	return form == CLO_HIP_SEGARG_OFFSETS ? arg_dispatch_form<TC, true>(a, vs, tie) : arg_dispatch_form<TC, false>(a, vs, tie);
}

// CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7, float 9, double 10. The key transform's kind, or -1.
inline int arg_kind(int t) { return t == 5 || t == 7 ? 0 : t == 4 || t == 6 ? 1 : t == 9 || t == 10 ? 2 : -1; }
inline int arg_size(int t) { return t == 6 || t == 7 || t == 10 ? 8 : 4; }

}  // namespace

extern "C" {

size_t clo_hip_segarg_tile(int value_size) { return value_size == 4 || value_size == 8 ? CLO_SEG_TILE : 0; }

size_t clo_hip_segarg_carry_tiles(void) { return CLO_SEG_CARRY_TRIP; }

size_t clo_hip_segarg_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	arg_ws w;
	return arg_layout(w, nullptr, numel_seg, numel);
}

int clo_hip_segarg(int op, int tie, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	uint32_t* idx_out, void* val_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (op != CLO_HIP_SEGARG_ARGMIN && op != CLO_HIP_SEGARG_ARGMAX) return CLO_HIP_EARGS;
	if (tie != CLO_HIP_SEGARG_FIRST && tie != CLO_HIP_SEGARG_LAST) return CLO_HIP_EARGS;
	if (form != CLO_HIP_SEGARG_COUNTS && form != CLO_HIP_SEGARG_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int kind = arg_kind(value_type);
	if (kind < 0) return CLO_HIP_EUNSUPPORTED;
	const size_t vs = (size_t) arg_size(value_type);
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGARG_OFFSETS)) return CLO_HIP_EARGS;
	if (!values_in && numel > 0) return CLO_HIP_EARGS;
	if (!idx_out && numel_seg > 0) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8) || clo_misaligned(num_in, 8)) return CLO_HIP_EARGS;
	if (clo_misaligned(counts_or_offsets, (size_t) count_size) || clo_misaligned(values_in, vs) || clo_misaligned(idx_out, 4) || clo_misaligned(val_out, vs))
		return CLO_HIP_EARGS;
	if (numel_seg == 0) {
		hipLaunchKernelGGL(clo_segarg_empty_kernel, dim3(1), dim3(1), 0, (hipStream_t) stream, (arg_u64*) num_out);
		return (int) hipGetLastError();
	}
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_segarg_workspace_bytes(numel_seg, numel)) return CLO_HIP_EWORKSPACE;

	arg_args a;
	a.src = counts_or_offsets; a.num_in = (const arg_u64*) num_in; a.vin = values_in; a.idx = idx_out; a.val = val_out; a.num_out = (arg_u64*) num_out;
	a.m_h = (unsigned) numel_seg; a.n = (unsigned) numel; a.s = (hipStream_t) stream;
	a.key.kx = clo_keyx_make(kind, 0, (int) (8 * vs));
	a.key.cmpl = op == CLO_HIP_SEGARG_ARGMAX ? ~0ull : 0ull;
	arg_layout(a, (char*) workspace, numel_seg, numel);
	return count_size == 8 ? arg_dispatch<uint64_t>(a, form, (int) vs, tie) : arg_dispatch<uint32_t>(a, form, (int) vs, tie);
}

}  // extern "C"
