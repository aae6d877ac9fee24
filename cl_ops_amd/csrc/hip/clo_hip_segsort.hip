// clo_hip_segsort.hip — a stable sort of every segment on its own, the segments given by counts or by CSR offsets
// (CloSegSort, include/clo_segsort.h; not upstream). With m = min(numel_seg, *num_in) segments whose ends
// are e_r and n rows, segment r covers rows [min(e_(r-1), n), min(e_r, n)); inside it the keys come out ascending in the
// order clo_keyx gives, equal keys in their input order, the values (or the global row index) moving with them.
//
// A segmented merge sort over fixed tiles of T = 2048 rows. No launch waits for another work-group or uses an atomic:
//   ENDS    the counts form only: the numel_seg inclusive ends as uint64 in the workspace (clo_hip_seg_device.h).
//   HEADS   the flags (one byte per row, zeroed by a memset before) get a 1 at row s_r of every non-empty segment that
//           starts below n: one thread per segment, so that empty segments cost one thread each and nothing later. The
//           starts of non-empty segments are distinct, no two threads write one byte. Thread 0 writes num_out.
//   TILE    one work-group per tile. The rank of a row's segment inside the tile is the running count of the flags. The
//           rows are sorted on chip by (rank, order key, row in tile), a composite that is unique, so that the bitonic
//           network is stable: 64 bits for keys of up to 4 bytes, the key and a 32-bit tag for 8-byte keys. Eight
//           consecutive rows per lane; the steps of distance below 8 run in registers. Sorting by rank first leaves every
//           segment on its own rows, so position j of the tile belongs to the segment row j belonged to. Only the segment
//           of the tile's first row (A) and of its last row (B) can cross a tile boundary: two halvings in the ends give
//           their true (s, e). With blocks of W = T << p rows, pass p MOVES a segment iff the middle of some pair of
//           blocks lies strictly inside it (ss_moves: bit p of its mask); a segment inside one tile has mask 0. Every
//           move goes from the outputs to the workspace copy of the rows or back, so the tile sort writes a segment to
//           the workspace iff its mask has an odd number of bits; everything else goes to the outputs and is final. The
//           tile leaves (mask_A | mask_B, s_A, e_A, s_B, e_B) in the workspace.
//   MERGE   pass p = 0 .. P - 1, P = ceil(log2(tiles)), one work-group per OUTPUT tile; it leaves at once when bit p of
//           the tile's word is clear. Inside a moving segment the blocks of W rows are sorted; the pair [lo, lo + 2W)
//           around the tile has mid = lo + W. For A and B (read back, clamped again), when bit p is set: if the segment
//           has mid strictly inside, the tile's stretch of the merge of [max(s, lo), mid) and [mid, min(e, lo + 2W)) is
//           taken by two merge-path halvings in global memory, staged in LDS, every element ranked in the other part
//           (ties: the left part first) and written through a permutation in LDS; otherwise (the segment merges in
//           another pair and only touches this one) the tile's rows of it are copied, so that the whole segment
//           changes sides. Source: the workspace iff an odd number of moves remain, this one included.
// Whatever the arrays hold: every halving is a loop over [lo, hi) that shrinks; ends are read below m only; s and e are
// clamped to s <= e <= n; a tile touches rows [tile0, tile0 + cnt), cnt <= T, tile0 + cnt <= min(total, n); merge ranges
// are clamped by clo_op_tile_range's rule; a permutation entry is clamped below cnt before it is used.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_tile_sort_device.h"

namespace {

typedef clo_op_u64 ss_u64;

constexpr int SS_THREADS = CLO_TS_THREADS;
constexpr int SS_WAVES = CLO_TS_WAVES;
constexpr int SS_ITEMS = CLO_TS_ITEMS;
constexpr unsigned SS_TILE = CLO_TS_TILE;                // T = 2048 rows, for every type

inline size_t ss_tiles(size_t numel) { return (numel + SS_TILE - 1) / SS_TILE; }
inline int ss_passes(size_t tiles) { int p = 0; while (((size_t) 1 << p) < tiles) ++p; return p; }

// ---- 1. the ends of the counts form: the three launches of clo_hip_seg_device.h ----

template <typename TC>
__global__ __launch_bounds__(SS_THREADS)
void clo_segsort_sums_kernel(const TC* __restrict__ counts, const ss_u64* __restrict__ num_in, unsigned m_h, int vec_ok, ss_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(SS_THREADS)
void clo_segsort_sums_scan_kernel(ss_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(SS_THREADS)
void clo_segsort_ends_kernel(const TC* __restrict__ counts, const ss_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const ss_u64* __restrict__ tsum, ss_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. heads ----
template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(SS_THREADS)
void clo_segsort_heads_kernel(const TC* __restrict__ src, const ss_u64* __restrict__ ends, const ss_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	unsigned char* __restrict__ flags, ss_u64* __restrict__ num_out) {
	const ss_u64 r = (ss_u64) blockIdx.x * SS_THREADS + threadIdx.x;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	if (r == 0) *num_out = m > 0u ? e.at(m - 1u) : 0ull;
	if (r >= m) return;
	const ss_u64 s = r > 0 ? e.at((unsigned) r - 1u) : 0ull, t = e.at((unsigned) r);
	if (s < t && s < n) flags[s] = 1;   // s < n: inside the flags
}

// numel_seg 0: there is nothing to read
__global__ void clo_segsort_empty_kernel(ss_u64* __restrict__ num_out) { *num_out = 0ull; }

// ---- the segment that holds row x: (s, e) clamped to s <= e <= n, and the merge passes that move it ----
struct ss_seg { unsigned s, e, mask; };

// Bit p: pass p moves the segment [s, e). With blocks of T << p rows, a the block of its first row and b of its last:
// a pass merges the two blocks of a pair where the pair's middle, an odd multiple k of the block, lies strictly inside,
// a < k <= b; where there is such a k the whole segment moves (merged, or copied where it only touches a pair), where
// there is none (one block, or an odd block and the even one after it) the segment stays. At most 32 trips: b - a halves.
__device__ __forceinline__ unsigned ss_moves(unsigned s, unsigned e) {
	unsigned mask = 0u;
	if (s >= e) return mask;
	unsigned a = s / SS_TILE, b = (e - 1u) / SS_TILE;
	for (unsigned p = 0u; p < 32u && a != b; ++p, a >>= 1, b >>= 1)
		if (b - a >= 2u || (b & 1u) != 0u) mask |= 1u << p;
	return mask;
}

template <typename TC, bool OFFSETS>
__device__ __forceinline__ ss_seg ss_find(const clo_op_ends<TC, OFFSETS>& e, unsigned m, unsigned n, unsigned x) {
	unsigned lo = 0u, hi = m;
	while (lo < hi) {   // at most 32 trips: hi - lo halves
		const unsigned mid = lo + ((hi - lo) >> 1);   // < hi <= m
		if (e.at(mid) <= x) lo = mid + 1u; else hi = mid;
	}
	ss_seg g;
	g.s = 0u; g.e = 0u; g.mask = 0u;
	if (lo < m) {
		const ss_u64 ee = clo_op_min64(e.at(lo), n);
		const ss_u64 s = lo > 0u ? clo_op_min64(e.at(lo - 1u), ee) : 0ull;
		g.s = (unsigned) s; g.e = (unsigned) ee;
		g.mask = ss_moves(g.s, g.e);
	}
	return g;
}

// the tile's rows [tile0, tile0 + cnt) and the two segments that may leave it; cnt 0: the tile lies beyond min(total, n)
struct ss_tile { unsigned tile0, cnt; ss_seg A, B; };

// What the tile sort leaves per tile for the merge passes: the passes with work, and A and B as it found them.
constexpr unsigned SS_INFO = 8u;   // words per tile: A.mask | B.mask, A.s, A.e, B.s, B.e, three unused (32 bytes)

// info NULL: A and B by two halvings in the ends (the tile sort); else from the tile's words, clamped again
template <typename TC, bool OFFSETS>
__device__ __forceinline__ ss_tile ss_tile_of(const TC* __restrict__ src, const ss_u64* __restrict__ ends, const ss_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ info) {
	ss_tile t;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	const ss_u64 lim = clo_op_min64(m > 0u ? e.at(m - 1u) : 0ull, n);
	const ss_u64 t0 = (ss_u64) blockIdx.x * SS_TILE;
	t.tile0 = (unsigned) clo_op_min64(t0, n);
	t.cnt = t0 < lim ? (unsigned) clo_op_min64(SS_TILE, lim - t0) : 0u;
	t.A.s = t.A.e = t.A.mask = 0u;
	t.B = t.A;
	if (t.cnt > 0u && !info) {
		t.A = ss_find<TC, OFFSETS>(e, m, n, t.tile0);
		t.B = ss_find<TC, OFFSETS>(e, m, n, t.tile0 + t.cnt - 1u);
	} else if (t.cnt > 0u) {
		const unsigned* const w = info + (size_t) blockIdx.x * SS_INFO;
		t.A.e = clo_op_min(w[2], n); t.A.s = clo_op_min(w[1], t.A.e); t.A.mask = ss_moves(t.A.s, t.A.e);
		t.B.e = clo_op_min(w[4], n); t.B.s = clo_op_min(w[3], t.B.e); t.B.mask = ss_moves(t.B.s, t.B.e);
	}
	return t;
}

// ---- 3. tile sort: the network, its item and the LDS layout are clo_hip_tile_sort_device.h's ----
template <typename TK, typename TC, bool OFFSETS, int MODE>
__global__ __launch_bounds__(SS_THREADS)
void clo_segsort_tile_kernel(const TC* __restrict__ src, const ss_u64* __restrict__ ends, const ss_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned char* __restrict__ flags, const TK* __restrict__ kin, const typename clo_op_val<MODE>::T* __restrict__ vin,
	TK* __restrict__ kout, TK* __restrict__ kws, typename clo_op_val<MODE>::T* __restrict__ vout, typename clo_op_val<MODE>::T* __restrict__ vws,
	unsigned* __restrict__ info, clo_keyx kx, int kvec) {
	constexpr bool WIDE = sizeof(TK) == 8;
	__shared__ ss_u64 s_k[SS_TILE];
	__shared__ unsigned s_tag[WIDE ? SS_TILE : 1];
	__shared__ unsigned s_w[SS_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const ss_tile t = ss_tile_of<TC, OFFSETS>(src, ends, num_in, m_h, n, nullptr);
	if (tid < SS_INFO) {
		const unsigned w[SS_INFO] = { t.A.mask | t.B.mask, t.A.s, t.A.e, t.B.s, t.B.e, 0u, 0u, 0u };
		info[(size_t) blockIdx.x * SS_INFO + tid] = w[tid];
	}
	if (t.cnt == 0u) return;   // the whole work-group

	// the ranks of the lane's rows: the running count of the heads (the flags hold whole tiles: no bound to check)
	const unsigned base = tid * SS_ITEMS;
	const ss_u64 f = *reinterpret_cast<const ss_u64*>(flags + (size_t) blockIdx.x * SS_TILE + base) & 0x0101010101010101ull;
	const unsigned mine = (unsigned) __popcll(f);
	const unsigned incl = clo_wave_scan_inclusive<unsigned>(mine, lane);
	if (lane == 63u) s_w[wave] = incl;
	__syncthreads();
	unsigned before = incl - mine;
	#pragma unroll
	for (unsigned w = 0; w < (unsigned) SS_WAVES; ++w) if (w < wave) before += s_w[w];

	TK raw[SS_ITEMS];
	{
		TK a[CLO_OP_VEC], b[CLO_OP_VEC];
		clo_op_load4<TK>(kin, (size_t) t.tile0 + base, (size_t) t.tile0 + t.cnt, kvec != 0, a);
		clo_op_load4<TK>(kin, (size_t) t.tile0 + base + CLO_OP_VEC, (size_t) t.tile0 + t.cnt, kvec != 0, b);
		#pragma unroll
		for (int c = 0; c < CLO_OP_VEC; ++c) { raw[c] = a[c]; raw[c + CLO_OP_VEC] = b[c]; }
	}
	clo_ts_item v[SS_ITEMS];
	#pragma unroll
	for (int c = 0; c < SS_ITEMS; ++c) {
		const unsigned row = base + (unsigned) c;
		const unsigned rank = before + (unsigned) __popcll(f & (~0ull >> (8 * (SS_ITEMS - 1 - c))));   // <= T
		const ss_u64 ok = (ss_u64) clo_keyx_fwd<TK>(raw[c], kx);
		if (row < t.cnt) {
			if constexpr (WIDE) { v[c].k = ok; v[c].tag = (rank << 16) | row; }
			else { v[c].k = ((ss_u64) rank << 48) | (ok << 16) | row; v[c].tag = 0u; }
		} else {
			v[c].k = ~0ull; v[c].tag = 0xffffffffu;
		}
	}
	CLO_TS_SORT(WIDE, v, s_k, s_tag, tid, base);

	// position j of the tile holds a row of the segment row j belonged to: a long segment with an odd number of moves
	// ahead goes to the workspace copy, everything else to the outputs
	const bool a_ws = (__popc(t.A.mask) & 1) != 0, b_ws = (__popc(t.B.mask) & 1) != 0;
	#pragma unroll
	for (unsigned q = 0; q < (unsigned) SS_ITEMS; ++q) {
		const unsigned j = tid + q * SS_THREADS;
		if (j >= t.cnt) continue;
		const unsigned g = t.tile0 + j;
		const bool ws = (a_ws && g >= t.A.s && g < t.A.e) || (b_ws && g >= t.B.s && g < t.B.e);
		const ss_u64 k = s_k[clo_ts_at(j)];
		unsigned row;
		TK key;
		if constexpr (WIDE) { row = s_tag[clo_ts_at(j)] & 0xffffu; key = clo_keyx_inv<TK>((TK) k, kx); }
		else { row = (unsigned) k & 0xffffu; key = clo_keyx_inv<TK>((TK) (k >> 16), kx); }
		row = clo_op_min(row, t.cnt - 1u);   // (it is below cnt already: the padding sorts behind)
		(ws ? kws : kout)[g] = key;
		if constexpr (MODE == CLO_OP_ARG) (ws ? vws : vout)[g] = t.tile0 + row;
		else if constexpr (MODE != CLO_OP_KEYS) (ws ? vws : vout)[g] = vin[(size_t) t.tile0 + row];
	}
}

// ---- 4. merge passes ----
template <typename TK, int MODE>
struct ss_bufs { TK* kout; TK* kws; typename clo_op_val<MODE>::T* vout; typename clo_op_val<MODE>::T* vws; };

// the tile's rows of segment g at pass p: merged from the two blocks of the pair, or copied
template <typename TK, int MODE>
__device__ __forceinline__ void ss_merge_part(const ss_seg& g, const ss_tile& t, unsigned p, const ss_bufs<TK, MODE>& io, const clo_keyx& kx,
	TK* s_key, unsigned short* s_perm, unsigned* s_split) {
	typedef typename clo_op_val<MODE>::T TV;
	const unsigned tid = threadIdx.x;
	if (((g.mask >> p) & 1u) == 0u) return;   // the whole work-group, here and below
	const unsigned o0 = clo_op_max(g.s, t.tile0), o1 = clo_op_min(g.e, t.tile0 + t.cnt);
	if (o0 >= o1) return;
	const unsigned cnt = o1 - o0;   // <= T
	const bool from_ws = (__popc(g.mask >> p) & 1) != 0;   // the moves from this pass on: the last one lands in the outputs
	const TK* const ksrc = from_ws ? io.kws : io.kout;
	TK* const kdst = from_ws ? io.kout : io.kws;
	const TV* const vsrc = from_ws ? io.vws : io.vout;
	TV* const vdst = from_ws ? io.vout : io.vws;
	const ss_u64 w = (ss_u64) SS_TILE << p;
	const ss_u64 lo = (ss_u64) t.tile0 & ~(2ull * w - 1ull), mid = lo + w, hi = lo + 2ull * w;
	if (!((ss_u64) g.s < mid && (ss_u64) g.e > mid)) {   // crosses lo or hi only: copied
		for (unsigned i = tid; i < cnt; i += SS_THREADS) {
			kdst[o0 + i] = ksrc[o0 + i];
			if constexpr (MODE != CLO_OP_KEYS) vdst[o0 + i] = vsrc[o0 + i];
		}
		return;
	}
	// left part [first, mid), right part [mid, last), both inside [0, n): mid < e <= n
	const unsigned first = (unsigned) clo_op_max64(g.s, lo), um = (unsigned) mid, last = (unsigned) clo_op_min64(g.e, hi);
	const unsigned na = um - first, nb = last - um;
	const unsigned d0 = o0 - first, d1 = o1 - first;   // o0 >= first, o1 <= last
	if (tid < 2u) s_split[tid] = clo_op_path<TK, true>(ksrc + first, ksrc + um, na, nb, tid == 0u ? d0 : d1, kx);
	__syncthreads();
	unsigned a0 = s_split[0], a1 = s_split[1];
	a0 = clo_op_min(clo_op_max(a0, d0 > nb ? d0 - nb : 0u), clo_op_min(d0, na));
	a1 = clo_op_min(clo_op_max(a1, clo_op_max(a0, d1 > nb ? d1 - nb : 0u)), clo_op_min(na, a0 + cnt));
	const unsigned na_t = a1 - a0, nb_t = cnt - na_t, b0 = d0 - a0;   // b0 + nb_t = d1 - a1 <= nb
	const unsigned ga = first + a0, gb = um + b0;
	for (unsigned i = tid; i < cnt; i += SS_THREADS) s_key[i] = i < na_t ? ksrc[ga + i] : ksrc[gb + (i - na_t)];
	__syncthreads();
	for (unsigned i = tid; i < cnt; i += SS_THREADS) {
		const TK x = clo_keyx_fwd<TK>(s_key[i], kx);
		unsigned pos;
		if (i < na_t) {   // how many of the right part lie strictly below
			unsigned l = 0u, h = nb_t;
			while (l < h) { const unsigned c = l + ((h - l) >> 1); if (clo_keyx_fwd<TK>(s_key[na_t + c], kx) < x) l = c + 1u; else h = c; }
			pos = i + l;
		} else {          // how many of the left part do not lie above
			unsigned l = 0u, h = na_t;
			while (l < h) { const unsigned c = l + ((h - l) >> 1); if (clo_keyx_fwd<TK>(s_key[c], kx) <= x) l = c + 1u; else h = c; }
			pos = (i - na_t) + l;
		}
		s_perm[pos] = (unsigned short) i;   // pos < na_t + nb_t = cnt
	}
	__syncthreads();
	for (unsigned i = tid; i < cnt; i += SS_THREADS) {
		const unsigned j = clo_op_min((unsigned) s_perm[i], cnt - 1u);   // a permutation when both parts are sorted
		kdst[o0 + i] = s_key[j];
		if constexpr (MODE != CLO_OP_KEYS) vdst[o0 + i] = vsrc[j < na_t ? ga + j : gb + (j - na_t)];
	}
}

template <typename TK, typename TC, bool OFFSETS, int MODE>
__global__ __launch_bounds__(SS_THREADS)
void clo_segsort_merge_kernel(const TC* __restrict__ src, const ss_u64* __restrict__ ends, const ss_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	const unsigned* __restrict__ info, ss_bufs<TK, MODE> io, unsigned p, clo_keyx kx) {
	__shared__ TK s_key[SS_TILE];
	__shared__ unsigned short s_perm[SS_TILE];
	__shared__ unsigned s_split[2];
	if (((info[(size_t) blockIdx.x * SS_INFO] >> p) & 1u) == 0u) return;   // no row of the tile moves in this pass
	const ss_tile t = ss_tile_of<TC, OFFSETS>(src, ends, num_in, m_h, n, info);
	if (t.cnt == 0u) return;
	ss_merge_part<TK, MODE>(t.A, t, p, io, kx, s_key, s_perm, s_split);
	if (t.B.s != t.A.s || t.B.e != t.A.e) {
		__syncthreads();   // the LDS arrays are used again
		ss_merge_part<TK, MODE>(t.B, t, p, io, kx, s_key, s_perm, s_split);
	}
}

struct ss_args {
	const void* src; const ss_u64* num_in; const void* kin; const void* vin; void* kout; void* vout; ss_u64* num_out;
	unsigned m_h, n; clo_keyx kx;
	ss_u64* ends; ss_u64* tsum; unsigned char* flags; unsigned* info; void* kws; void* vws; hipStream_t s;
};

#define SS_CHECK_LAUNCH() do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int) e_; } while (0)

constexpr const char* SS_ENDS_LABELS[3] = { "segsort_sums", "segsort_sums_scan", "segsort_ends" };

template <typename TK, typename TC, bool OFFSETS, int MODE>
int ss_launch(const ss_args& a) {
	typedef typename clo_op_val<MODE>::T TV;
	if constexpr (!OFFSETS) {
		const int st = clo_op_ends_launch<TC>(clo_segsort_sums_kernel<TC>, clo_segsort_sums_scan_kernel, clo_segsort_ends_kernel<TC>, SS_ENDS_LABELS,
			a.src, a.num_in, a.m_h, a.tsum, a.ends, a.s);
		if (st != 0) return st;
	}
	const unsigned tiles = (unsigned) ss_tiles(a.n);
	if (tiles > 0u) {
		clo_timing_scope timing("segsort_zero", a.s);
		const hipError_t e = hipMemsetAsync(a.flags, 0, (size_t) tiles * SS_TILE, a.s);
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("segsort_heads", a.s);
		hipLaunchKernelGGL((clo_segsort_heads_kernel<TC, OFFSETS>), dim3((a.m_h + SS_THREADS - 1u) / SS_THREADS), dim3(SS_THREADS), 0, a.s,
			(const TC*) a.src, (const ss_u64*) a.ends, a.num_in, a.m_h, a.n, a.flags, a.num_out);
		SS_CHECK_LAUNCH();
	}
	if (tiles == 0u) return 0;
	{
		clo_timing_scope timing("segsort_tile", a.s);
		hipLaunchKernelGGL((clo_segsort_tile_kernel<TK, TC, OFFSETS, MODE>), dim3(tiles), dim3(SS_THREADS), 0, a.s,
			(const TC*) a.src, (const ss_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned char*) a.flags, (const TK*) a.kin, (const TV*) a.vin,
			(TK*) a.kout, (TK*) a.kws, (TV*) a.vout, (TV*) a.vws, a.info, a.kx, clo_op_vec_ok<TK>(a.kin));
		SS_CHECK_LAUNCH();
	}
	ss_bufs<TK, MODE> io;
	io.kout = (TK*) a.kout; io.kws = (TK*) a.kws; io.vout = (TV*) a.vout; io.vws = (TV*) a.vws;
	const int passes = ss_passes(tiles);
	for (int p = 0; p < passes; ++p) {
		clo_timing_scope timing("segsort_merge", a.s);
		hipLaunchKernelGGL((clo_segsort_merge_kernel<TK, TC, OFFSETS, MODE>), dim3(tiles), dim3(SS_THREADS), 0, a.s,
			(const TC*) a.src, (const ss_u64*) a.ends, a.num_in, a.m_h, a.n, (const unsigned*) a.info, io, (unsigned) p, a.kx);
		SS_CHECK_LAUNCH();
	}
	return 0;
}

template <typename TK, typename TC, bool OFFSETS>
int ss_dispatch_mode(const ss_args& a, int mode) {
	switch (mode) {
		case CLO_OP_KEYS: return ss_launch<TK, TC, OFFSETS, CLO_OP_KEYS>(a);
		case CLO_OP_V4: return ss_launch<TK, TC, OFFSETS, CLO_OP_V4>(a);
		case CLO_OP_V8: return ss_launch<TK, TC, OFFSETS, CLO_OP_V8>(a);
		default: return ss_launch<TK, TC, OFFSETS, CLO_OP_ARG>(a);
	}
}

template <typename TK>
int ss_dispatch(const ss_args& a, int form, int count_size, int mode) {
	if (form == CLO_HIP_SEGSORT_OFFSETS)
		return count_size == 8 ? ss_dispatch_mode<TK, uint64_t, true>(a, mode) : ss_dispatch_mode<TK, uint32_t, true>(a, mode);
	return count_size == 8 ? ss_dispatch_mode<TK, uint64_t, false>(a, mode) : ss_dispatch_mode<TK, uint32_t, false>(a, mode);
}

// CloType numbers (clo_common.h): char 0, uchar 1, short 2, ushort 3, int 4, uint 5, long 6, ulong 7, half 8, float 9, double 10
inline int ss_key_size(int t) { return t < 0 || t > 10 ? 0 : t == 8 ? 2 : t == 9 ? 4 : t == 10 ? 8 : 1 << (t >> 1); }
inline int ss_key_kind(int t) { return t >= 8 ? 2 : (t & 1) ? 0 : 1; }

// the parts of the workspace, in order
struct ss_layout { size_t ends, tsum, flags, info, kws, kws2, vws, total; };
inline ss_layout ss_layout_of(size_t numel_seg, size_t numel, int key_size, int value_size) {
	ss_layout l;
	const size_t tiles = ss_tiles(numel);
	size_t at = 0;
	l.ends = at; at += clo_op_ws_align(numel_seg * sizeof(ss_u64));
	l.tsum = at; at += clo_op_ws_align((clo_op_ends_tiles(numel_seg) + 1) * sizeof(ss_u64));
	l.flags = at; at += clo_op_ws_align(tiles * SS_TILE);
	l.info = at; at += clo_op_ws_align(tiles * SS_INFO * sizeof(unsigned));
	l.kws = at; at += clo_op_ws_align(numel * (size_t) key_size);
	l.kws2 = at; at += value_size == 4 ? clo_op_ws_align(numel * (size_t) key_size) : 0;   // the arg form without keys_out
	l.vws = at; at += clo_op_ws_align(numel * (size_t) value_size);
	l.total = at;
	return l;
}

}  // namespace

extern "C" {

size_t clo_hip_segsort_tile(int key_size, int value_size) {
	return clo_op_key_size_ok(key_size) && clo_op_value_size_ok(value_size) ? SS_TILE : 0;
}

size_t clo_hip_segsort_workspace_bytes(size_t numel_seg, size_t numel, int key_size, int value_size) {
	if (numel_seg == 0 && numel == 0) return 0;
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return ss_layout_of(numel_seg, numel, key_size, value_size).total;
}

int clo_hip_segsort(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, uint64_t* num_out, size_t numel_seg, size_t numel, int key_type, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (form != CLO_HIP_SEGSORT_COUNTS && form != CLO_HIP_SEGSORT_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int ks = ss_key_size(key_type);
	if (ks == 0 || !clo_op_value_size_ok(value_size)) return CLO_HIP_EUNSUPPORTED;
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGSORT_OFFSETS)) return CLO_HIP_EARGS;
	if (!keys_in && numel > 0) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	if (value_size == 8 && !values_in) return CLO_HIP_EARGS;
	const bool arg = value_size == 4 && !values_in;
	if (!keys_out && !arg) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8) || clo_misaligned(num_in, 8)) return CLO_HIP_EARGS;
	if (clo_misaligned(counts_or_offsets, (size_t) count_size) || clo_misaligned(keys_in, (size_t) ks) || clo_misaligned(keys_out, (size_t) ks)) return CLO_HIP_EARGS;
	if (value_size > 0 && (clo_misaligned(values_in, (size_t) value_size) || clo_misaligned(values_out, (size_t) value_size))) return CLO_HIP_EARGS;
	if (numel_seg == 0) {
		hipLaunchKernelGGL(clo_segsort_empty_kernel, dim3(1), dim3(1), 0, (hipStream_t) stream, (ss_u64*) num_out);
		return (int) hipGetLastError();
	}
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	const ss_layout l = ss_layout_of(numel_seg, numel, ks, value_size);
	if (workspace_bytes < l.total) return CLO_HIP_EWORKSPACE;

	char* const ws = (char*) workspace;
	ss_args a;
	a.src = counts_or_offsets; a.num_in = (const ss_u64*) num_in; a.kin = keys_in; a.vin = values_in;
	a.kout = keys_out ? keys_out : (void*) (ws + l.kws2);   // the arg form without keys_out: the keys still ping-pong
	a.vout = values_out; a.num_out = (ss_u64*) num_out;
	a.m_h = (unsigned) numel_seg; a.n = (unsigned) numel; a.s = (hipStream_t) stream;
	a.kx = clo_keyx_make(ss_key_kind(key_type), 0, 8 * ks);
	a.ends = (ss_u64*) (ws + l.ends); a.tsum = (ss_u64*) (ws + l.tsum);
	a.flags = (unsigned char*) (ws + l.flags); a.info = (unsigned*) (ws + l.info);
	a.kws = ws + l.kws; a.vws = ws + l.vws;
	const int mode = clo_op_mode(value_size, arg);
	switch (ks) {
		case 1: return ss_dispatch<uint8_t>(a, form, count_size, mode);
		case 2: return ss_dispatch<uint16_t>(a, form, count_size, mode);
		case 4: return ss_dispatch<uint32_t>(a, form, count_size, mode);
		default: return ss_dispatch<uint64_t>(a, form, count_size, mode);
	}
}

}  // extern "C"
