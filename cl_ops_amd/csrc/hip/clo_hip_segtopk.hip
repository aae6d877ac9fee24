// clo_hip_segtopk.hip — the k smallest or largest rows of every segment, the segments given by counts or by CSR offsets
// (CloSegTopK, include/clo_segtopk.h; not upstream). With m = min(numel_seg, *num_in) segments whose ends
// are e_r and n rows, segment r covers rows [min(e_(r-1), n), min(e_r, n)); its first c_r = min(k, len_r) rows in the
// stable sort by x = clo_keyx_fwd(key) ^ flip (flip = 0 for "smallest", all ones for "largest") go to out[r * k + j].
//
// CloSegSort's tile sort (clo_hip_tile_sort_device.h) over fixed tiles of T = 2048 rows, and a tree of small merges of
// at most 2 k candidates for the segments that cross a tile boundary. No launch waits for another work-group or uses
// an atomic:
//   ENDS     the counts form only: the numel_seg inclusive ends as uint64 in the workspace (clo_hip_seg_device.h).
//   HEADS    one thread per segment r < m: a 1 in the flags (one byte per row, zeroed by a memset before) and r in the
//            segment numbers (four bytes per row, read only where the flag is 1) at row s_r of every non-empty segment
//            that starts below n, and counts_out[r] = min(k, len_r) for every segment, empty ones too. One thread per
//            tile: the segments of the tile's first row (A) and of its last row (B) by two halvings in the ends, as
//            clamped (s, e, r), the tile's row count, and the mask of the combine levels in which the tile is a
//            destination. Thread 0 writes num_out. (The threads are the same launch: thread i does segment i and tile i.)
//   TILE     one work-group per tile. The rows are sorted on chip by (rank of the segment in the tile, x, row in tile).
//            Position j of the sorted tile belongs to the piece row j belonged to; the position of a piece's head is
//            kept per rank in LDS, so q = j - head is the row's place in its piece. Only A (when it starts before the
//            tile) and B (when it ends behind it) cross a boundary: their first min(k, piece) rows go, as (x, global
//            row), to the tile's candidate slot 0 (A) or 1 (B) in the workspace. Every other piece is a whole segment:
//            its rows with q < k go to out[r * k + q], r read from the segment numbers at the head and clamped below m.
//   COMBINE  level p = 0 .. P - 1, P = ceil(log2(tiles)), one work-group per tile; it leaves at once when bit p of the
//            tile's mask is clear. A segment over tiles a .. b has one sorted list per tile: slot 1 of a, slot 0 of the
//            others. At level p, tile t with (t - a) % 2^(p+1) == 0 and t + 2^p <= b replaces its list by the first k
//            of the merge of its list with that of tile t + 2^p, ties to the left list (its rows have the lower
//            indices). A list's length is known from (s, e) alone: min(k, the segment's rows in the tiles it stands
//            for). Both lists are staged in LDS before anything is written, so the update is in place. At the last
//            level of the segment, a + 2^(p+1) > b, tile a writes to out[r * k ..] instead: keys back through
//            clo_keyx_inv, values gathered by the row.
// Whatever the arrays hold: every halving is a loop over [lo, hi) that shrinks; ends are read below m only; s and e are
// clamped to s <= e <= n wherever they are read, the tile's count to T and n; r is clamped below m; q, and a merged
// position, is below k before it is used, so that every write to the outputs lies in [0, m * k); a list has at most k
// entries and a slot holds k; a candidate's row is clamped below n before values_in is read.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_tile_sort_device.h"

namespace {

typedef clo_op_u64 st_u64;

constexpr int ST_THREADS = CLO_TS_THREADS;
constexpr int ST_WAVES = CLO_TS_WAVES;
constexpr int ST_ITEMS = CLO_TS_ITEMS;
constexpr unsigned ST_TILE = CLO_TS_TILE;
constexpr unsigned ST_K_MAX = ST_TILE / 2u;   // two candidate lists fit the LDS a tile's keys take

inline size_t st_tiles(size_t numel) { return (numel + ST_TILE - 1) / ST_TILE; }
inline int st_levels(size_t tiles) { int p = 0; while (((size_t) 1 << p) < tiles) ++p; return p; }

// ---- 1. the ends of the counts form: the three launches of clo_hip_seg_device.h ----

template <typename TC>
__global__ __launch_bounds__(ST_THREADS)
void clo_segtopk_sums_kernel(const TC* __restrict__ counts, const st_u64* __restrict__ num_in, unsigned m_h, int vec_ok, st_u64* __restrict__ tsum) {
	clo_op_ends_sums<TC>(counts, num_in, m_h, vec_ok, tsum);
}

__global__ __launch_bounds__(ST_THREADS)
void clo_segtopk_sums_scan_kernel(st_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

template <typename TC>
__global__ __launch_bounds__(ST_THREADS)
void clo_segtopk_ends_kernel(const TC* __restrict__ counts, const st_u64* __restrict__ num_in, unsigned m_h, int vec_ok,
	const st_u64* __restrict__ tsum, st_u64* __restrict__ ends) {
	clo_op_ends_write<TC>(counts, num_in, m_h, vec_ok, tsum, ends);
}

// ---- 2. heads, counts_out and the tiles' words ----

// a segment as the kernels after the heads see it: rows [s, e), s <= e <= n, and its number
struct st_seg { unsigned s, e, r; };

// What the heads leave per tile: A.s, A.e, A.r, B.s, B.e, B.r, the mask of its combine levels, its row count (32 bytes).
constexpr unsigned ST_INFO = 8u;

// Tile t is a destination of segment g at level p: (t - a) % 2^(p+1) == 0 and t + 2^p <= b, over tiles a .. b.
__device__ __forceinline__ bool st_is_dest(const st_seg& g, unsigned t, unsigned p) {
	if (g.s >= g.e) return false;
	const unsigned a = g.s / ST_TILE, b = (g.e - 1u) / ST_TILE;
	if (t < a || t >= b) return false;
	return ((st_u64) (t - a) & ((2ull << p) - 1ull)) == 0ull && (st_u64) t + (1ull << p) <= (st_u64) b;
}

// at most 32 trips; once a level fails, every higher one does
__device__ __forceinline__ unsigned st_dest_mask(const st_seg& g, unsigned t) {
	unsigned mask = 0u;
	for (unsigned p = 0u; p < 32u && st_is_dest(g, t, p); ++p) mask |= 1u << p;
	return mask;
}

template <typename TC, bool OFFSETS>
__device__ __forceinline__ st_seg st_find(const clo_op_ends<TC, OFFSETS>& e, unsigned m, unsigned n, unsigned x) {
	unsigned lo = 0u, hi = m;
	while (lo < hi) {   // at most 32 trips: hi - lo halves
		const unsigned mid = lo + ((hi - lo) >> 1);   // < hi <= m
		if (e.at(mid) <= x) lo = mid + 1u; else hi = mid;
	}
	st_seg g;
	g.s = 0u; g.e = 0u; g.r = 0u;
	if (lo < m) {
		const st_u64 ee = clo_op_min64(e.at(lo), n);
		const st_u64 s = lo > 0u ? clo_op_min64(e.at(lo - 1u), ee) : 0ull;
		g.s = (unsigned) s; g.e = (unsigned) ee; g.r = lo;
	}
	return g;
}

template <typename TC, bool OFFSETS>
__global__ __launch_bounds__(ST_THREADS)
void clo_segtopk_heads_kernel(const TC* __restrict__ src, const st_u64* __restrict__ ends, const st_u64* __restrict__ num_in, unsigned m_h, unsigned n,
	unsigned tiles, unsigned k, unsigned char* __restrict__ flags, unsigned* __restrict__ segid, unsigned* __restrict__ info,
	unsigned* __restrict__ counts_out, st_u64* __restrict__ num_out) {
	const st_u64 i = (st_u64) blockIdx.x * ST_THREADS + threadIdx.x;
	const unsigned m = clo_op_segments(num_in, m_h);
	const clo_op_ends<TC, OFFSETS> e = clo_op_ends_make<TC, OFFSETS>(src, ends);
	const st_u64 total = m > 0u ? e.at(m - 1u) : 0ull;
	if (i == 0) *num_out = total;
	if (i < m) {
		const unsigned r = (unsigned) i;
		const st_u64 s = r > 0u ? e.at(r - 1u) : 0ull, t = e.at(r);
		if (s < t && s < n) { flags[s] = 1; segid[s] = r; }   // s < n: inside the flags and the segment numbers
		if (k > 0u) {
			const st_u64 cs = clo_op_min64(s, n), ct = clo_op_min64(t, n);
			counts_out[r] = ct > cs ? (unsigned) clo_op_min64(ct - cs, k) : 0u;
		}
	}
	if (i < tiles && k > 0u) {
		const st_u64 lim = clo_op_min64(total, n), t0 = i * ST_TILE;
		const unsigned cnt = t0 < lim ? (unsigned) clo_op_min64(ST_TILE, lim - t0) : 0u;
		st_seg A, B;
		A.s = A.e = A.r = 0u;
		B = A;
		if (cnt > 0u) {
			A = st_find<TC, OFFSETS>(e, m, n, (unsigned) t0);
			B = st_find<TC, OFFSETS>(e, m, n, (unsigned) t0 + cnt - 1u);
		}
		unsigned* const w = info + (size_t) i * ST_INFO;
		w[0] = A.s; w[1] = A.e; w[2] = A.r; w[3] = B.s; w[4] = B.e; w[5] = B.r;
		w[6] = st_dest_mask(A, (unsigned) i) | st_dest_mask(B, (unsigned) i);
		w[7] = cnt;
	}
}

// numel_seg 0: there is nothing to read
__global__ void clo_segtopk_empty_kernel(st_u64* __restrict__ num_out) { *num_out = 0ull; }

// the tile's words, clamped again: never trusted
struct st_tile { unsigned tile0, cnt, mask; st_seg A, B; };

__device__ __forceinline__ st_tile st_tile_of(const unsigned* __restrict__ info, unsigned n, unsigned m) {
	st_tile t;
	const unsigned* const w = info + (size_t) blockIdx.x * ST_INFO;
	const st_u64 t0 = (st_u64) blockIdx.x * ST_TILE;
	t.tile0 = (unsigned) clo_op_min64(t0, n);
	t.cnt = m > 0u ? clo_op_min(clo_op_min(w[7], ST_TILE), n - t.tile0) : 0u;
	t.A.e = clo_op_min(w[1], n); t.A.s = clo_op_min(w[0], t.A.e); t.A.r = clo_op_min(w[2], m > 0u ? m - 1u : 0u);
	t.B.e = clo_op_min(w[4], n); t.B.s = clo_op_min(w[3], t.B.e); t.B.r = clo_op_min(w[5], m > 0u ? m - 1u : 0u);
	t.mask = w[6];
	return t;
}

// where the outputs and the candidate lists are, and what selects
template <typename TK, int MODE>
struct st_io {
	const typename clo_op_val<MODE>::T* vin; TK* kout; typename clo_op_val<MODE>::T* vout;
	TK* ck; unsigned* cr;   // the candidates: per tile two slots of k entries (x, global row)
	unsigned k; TK flip;
};

// out[at] = the row `row` whose order key is x
template <typename TK, int MODE>
__device__ __forceinline__ void st_emit(const st_io<TK, MODE>& io, size_t at, TK x, unsigned row, const clo_keyx& kx) {
	if (io.kout) io.kout[at] = clo_keyx_inv<TK>((TK) (x ^ io.flip), kx);
	if constexpr (MODE == CLO_OP_ARG) io.vout[at] = row;
	else if constexpr (MODE != CLO_OP_KEYS) io.vout[at] = io.vin[row];
}

// ---- 3. tile sort and emit ----
template <typename TK, int MODE>
__global__ __launch_bounds__(ST_THREADS)
void clo_segtopk_tile_kernel(const st_u64* __restrict__ num_in, unsigned m_h, unsigned n, const unsigned* __restrict__ info,
	const unsigned char* __restrict__ flags, const unsigned* __restrict__ segid, const TK* __restrict__ kin, st_io<TK, MODE> io, clo_keyx kx, int kvec) {
	constexpr bool WIDE = sizeof(TK) == 8;
	__shared__ st_u64 s_k[ST_TILE];
	__shared__ unsigned s_tag[WIDE ? ST_TILE : 1];
	// By rank - 1: the row in the tile of the piece's head (rank 0, the piece without a head in the tile, begins at row 0).
	// The waves' head counts lie in its first bytes until the barrier that follows their last read: with them in an array
	// of their own the kernel's LDS would pass the 20 480 bytes at which a CU holds eight work-groups.
	__shared__ unsigned short s_head[ST_TILE];
	unsigned* const s_w = reinterpret_cast<unsigned*>(s_head);
	static_assert(ST_WAVES * sizeof(unsigned) <= sizeof(unsigned short) * ST_TILE, "the waves' counts fit");
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned m = clo_op_segments(num_in, m_h);
	const st_tile t = st_tile_of(info, n, m);
	if (t.cnt == 0u) return;   // the whole work-group

	// the ranks of the lane's rows: the running count of the heads (the flags hold whole tiles: no bound to check)
	const unsigned base = tid * ST_ITEMS;
	const st_u64 f = *reinterpret_cast<const st_u64*>(flags + (size_t) blockIdx.x * ST_TILE + base) & 0x0101010101010101ull;
	const unsigned mine = (unsigned) __popcll(f);
	const unsigned incl = clo_wave_scan_inclusive<unsigned>(mine, lane);
	if (lane == 63u) s_w[wave] = incl;
	__syncthreads();
	unsigned before = incl - mine;
	#pragma unroll
	for (unsigned w = 0; w < (unsigned) ST_WAVES; ++w) if (w < wave) before += s_w[w];
	__syncthreads();   // s_w becomes s_head

	TK raw[ST_ITEMS];
	{
		TK a[CLO_OP_VEC], b[CLO_OP_VEC];
		clo_op_load4<TK>(kin, (size_t) t.tile0 + base, (size_t) t.tile0 + t.cnt, kvec != 0, a);
		clo_op_load4<TK>(kin, (size_t) t.tile0 + base + CLO_OP_VEC, (size_t) t.tile0 + t.cnt, kvec != 0, b);
		#pragma unroll
		for (int c = 0; c < CLO_OP_VEC; ++c) { raw[c] = a[c]; raw[c + CLO_OP_VEC] = b[c]; }
	}
	clo_ts_item v[ST_ITEMS];
	#pragma unroll
	for (int c = 0; c < ST_ITEMS; ++c) {
		const unsigned row = base + (unsigned) c;
		const unsigned rank = before + (unsigned) __popcll(f & (~0ull >> (8 * (ST_ITEMS - 1 - c))));   // <= T
		if ((f >> (8 * c)) & 1ull) s_head[rank - 1u] = (unsigned short) row;   // rank >= 1 here, <= T; one head per rank
		const st_u64 ok = (st_u64) (TK) (clo_keyx_fwd<TK>(raw[c], kx) ^ io.flip);
		if (row < t.cnt) {
			if constexpr (WIDE) { v[c].k = ok; v[c].tag = (rank << 16) | row; }
			else { v[c].k = ((st_u64) rank << 48) | (ok << 16) | row; v[c].tag = 0u; }
		} else {
			v[c].k = ~0ull; v[c].tag = 0xffffffffu;
		}
	}
	CLO_TS_SORT(WIDE, v, s_k, s_tag, tid, base);   // (its barriers are s_head's too)

	// A crosses the tile's first boundary when it starts before the tile, B the last when it ends behind it: their
	// rows are candidates. Everything else is a whole segment and final.
	const bool a_multi = t.A.s < t.tile0, b_multi = (st_u64) t.B.e > (st_u64) t.tile0 + ST_TILE;
	const unsigned b_from = clo_op_max(t.B.s, t.tile0);
	#pragma unroll
	for (unsigned q = 0; q < (unsigned) ST_ITEMS; ++q) {
		const unsigned j = tid + q * ST_THREADS;
		if (j >= t.cnt) continue;
		const unsigned g = t.tile0 + j;
		const st_u64 kk = s_k[clo_ts_at(j)];
		unsigned row, rank;
		TK x;
		if constexpr (WIDE) { const unsigned tag = s_tag[clo_ts_at(j)]; row = tag & 0xffffu; rank = tag >> 16; x = (TK) kk; }
		else { row = (unsigned) kk & 0xffffu; rank = (unsigned) (kk >> 48); x = (TK) (kk >> 16); }
		row = t.tile0 + clo_op_min(row, t.cnt - 1u);   // (it is below cnt already: the padding sorts behind)
		if (a_multi && g < t.A.e) {
			if (j < io.k) {
				const size_t at = ((size_t) blockIdx.x * 2u) * io.k + j;
				io.ck[at] = x; io.cr[at] = row;
			}
		} else if (b_multi && g >= b_from) {
			const unsigned qb = g - b_from;
			if (qb < io.k) {
				const size_t at = ((size_t) blockIdx.x * 2u + 1u) * io.k + qb;
				io.ck[at] = x; io.cr[at] = row;
			}
		} else {
			const unsigned head = rank == 0u ? 0u : clo_op_min((unsigned) s_head[clo_op_min(rank, ST_TILE) - 1u], j);
			const unsigned qf = j - head;
			if (qf < io.k) {
				const unsigned r = clo_op_min(rank == 0u ? t.A.r : segid[(size_t) t.tile0 + head], m - 1u);   // m > 0: cnt > 0
				st_emit<TK, MODE>(io, (size_t) r * io.k + qf, x, row, kx);
			}
		}
	}
}

// ---- 4. combine levels ----

// segment g's list of tile t becomes the first k of its merge with the list of tile t + 2^p
template <typename TK, int MODE>
__device__ __forceinline__ void st_combine_part(const st_seg& g, unsigned p, unsigned n, const st_io<TK, MODE>& io, const clo_keyx& kx,
	TK* s_x, unsigned* s_row) {
	const unsigned tid = threadIdx.x, t = blockIdx.x;
	if (!st_is_dest(g, t, p)) return;   // the whole work-group, here and below
	const unsigned a = g.s / ST_TILE, b = (g.e - 1u) / ST_TILE;   // a <= t < b
	const unsigned u = t + (1u << p);                             // <= b: a tile of the workspace
	const st_u64 w = (st_u64) ST_TILE << p;
	const st_u64 lt = (st_u64) t * ST_TILE, ut = (st_u64) u * ST_TILE;   // ut < e, and ut > s
	const unsigned nl = (unsigned) clo_op_min64(io.k, clo_op_min64(g.e, lt + w) - clo_op_max64(g.s, lt));
	const unsigned nr = (unsigned) clo_op_min64(io.k, clo_op_min64(g.e, ut + w) - ut);
	const size_t left = ((size_t) t * 2u + (t == a ? 1u : 0u)) * io.k, right = ((size_t) u * 2u) * io.k;
	const unsigned cnt = nl + nr;   // <= 2 k
	for (unsigned i = tid; i < cnt; i += ST_THREADS) {
		const size_t at = i < nl ? left + i : right + (i - nl);
		s_x[i] = io.ck[at]; s_row[i] = io.cr[at];
	}
	__syncthreads();
	const bool last = t == a && (st_u64) a + (2ull << p) > (st_u64) b;
	for (unsigned i = tid; i < cnt; i += ST_THREADS) {
		const TK x = s_x[i];
		unsigned pos;
		if (i < nl) {   // how many of the right list lie strictly below
			unsigned l = 0u, h = nr;
			while (l < h) { const unsigned c = l + ((h - l) >> 1); if (s_x[nl + c] < x) l = c + 1u; else h = c; }
			pos = i + l;
		} else {        // how many of the left list do not lie above
			unsigned l = 0u, h = nl;
			while (l < h) { const unsigned c = l + ((h - l) >> 1); if (s_x[c] <= x) l = c + 1u; else h = c; }
			pos = (i - nl) + l;
		}
		if (pos >= io.k) continue;
		const unsigned row = clo_op_min(s_row[i], n - 1u);   // n > 0: the segment has rows
		if (last) st_emit<TK, MODE>(io, (size_t) g.r * io.k + pos, x, row, kx);
		else { io.ck[left + pos] = x; io.cr[left + pos] = row; }
	}
}

template <typename TK, int MODE>
__global__ __launch_bounds__(ST_THREADS)
void clo_segtopk_combine_kernel(const st_u64* __restrict__ num_in, unsigned m_h, unsigned n, const unsigned* __restrict__ info,
	st_io<TK, MODE> io, unsigned p, clo_keyx kx) {
	__shared__ TK s_x[2u * ST_K_MAX];
	__shared__ unsigned s_row[2u * ST_K_MAX];
	if (((info[(size_t) blockIdx.x * ST_INFO + 6u] >> p) & 1u) == 0u) return;   // no list of the tile grows at this level
	const unsigned m = clo_op_segments(num_in, m_h);
	const st_tile t = st_tile_of(info, n, m);
	if (t.cnt == 0u || io.k > ST_K_MAX) return;
	st_combine_part<TK, MODE>(t.A, p, n, io, kx, s_x, s_row);
	if (t.B.s != t.A.s || t.B.e != t.A.e) {
		__syncthreads();   // the LDS arrays are used again
		st_combine_part<TK, MODE>(t.B, p, n, io, kx, s_x, s_row);
	}
}

struct st_args {
	const void* src; const st_u64* num_in; const void* kin; const void* vin; void* kout; void* vout; unsigned* counts_out; st_u64* num_out;
	unsigned m_h, n, k; bool largest; clo_keyx kx;
	st_u64* ends; st_u64* tsum; unsigned char* flags; unsigned* segid; unsigned* info; void* ck; unsigned* cr; hipStream_t s;
};

#define ST_CHECK_LAUNCH() do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int) e_; } while (0)

constexpr const char* ST_ENDS_LABELS[3] = { "segtopk_sums", "segtopk_sums_scan", "segtopk_ends" };

// the launches that read the segment description: the only ones that know the count type and the form
template <typename TC, bool OFFSETS>
int st_launch_heads(const st_args& a, unsigned tiles) {
	if constexpr (!OFFSETS) {
		const int st = clo_op_ends_launch<TC>(clo_segtopk_sums_kernel<TC>, clo_segtopk_sums_scan_kernel, clo_segtopk_ends_kernel<TC>, ST_ENDS_LABELS,
			a.src, a.num_in, a.m_h, a.tsum, a.ends, a.s);
		if (st != 0) return st;
	}
	if (tiles > 0u) {
		clo_timing_scope timing("segtopk_zero", a.s);
		const hipError_t e = hipMemsetAsync(a.flags, 0, (size_t) tiles * ST_TILE, a.s);
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("segtopk_heads", a.s);
	const unsigned threads = a.m_h > tiles ? a.m_h : tiles;
	hipLaunchKernelGGL((clo_segtopk_heads_kernel<TC, OFFSETS>), dim3((threads + ST_THREADS - 1u) / ST_THREADS), dim3(ST_THREADS), 0, a.s,
		(const TC*) a.src, (const st_u64*) a.ends, a.num_in, a.m_h, a.n, tiles, a.k, a.flags, a.segid, a.info, a.counts_out, a.num_out);
	ST_CHECK_LAUNCH();
	return 0;
}

template <typename TK, int MODE>
int st_launch_rows(const st_args& a, unsigned tiles) {
	typedef typename clo_op_val<MODE>::T TV;
	st_io<TK, MODE> io;
	io.vin = (const TV*) a.vin; io.kout = (TK*) a.kout; io.vout = (TV*) a.vout;
	io.ck = (TK*) a.ck; io.cr = a.cr; io.k = a.k; io.flip = a.largest ? (TK) ~(TK) 0 : (TK) 0;
	{
		clo_timing_scope timing("segtopk_tile", a.s);
		hipLaunchKernelGGL((clo_segtopk_tile_kernel<TK, MODE>), dim3(tiles), dim3(ST_THREADS), 0, a.s,
			a.num_in, a.m_h, a.n, (const unsigned*) a.info, (const unsigned char*) a.flags, (const unsigned*) a.segid, (const TK*) a.kin, io, a.kx,
			clo_op_vec_ok<TK>(a.kin));
		ST_CHECK_LAUNCH();
	}
	const int levels = st_levels(tiles);
	for (int p = 0; p < levels; ++p) {
		clo_timing_scope timing("segtopk_combine", a.s);
		hipLaunchKernelGGL((clo_segtopk_combine_kernel<TK, MODE>), dim3(tiles), dim3(ST_THREADS), 0, a.s,
			a.num_in, a.m_h, a.n, (const unsigned*) a.info, io, (unsigned) p, a.kx);
		ST_CHECK_LAUNCH();
	}
	return 0;
}

template <typename TK>
int st_dispatch_mode(const st_args& a, unsigned tiles, int mode) {
	switch (mode) {
		case CLO_OP_KEYS: return st_launch_rows<TK, CLO_OP_KEYS>(a, tiles);
		case CLO_OP_V4: return st_launch_rows<TK, CLO_OP_V4>(a, tiles);
		case CLO_OP_V8: return st_launch_rows<TK, CLO_OP_V8>(a, tiles);
		default: return st_launch_rows<TK, CLO_OP_ARG>(a, tiles);
	}
}

// CloType numbers (clo_common.h): char 0, uchar 1, short 2, ushort 3, int 4, uint 5, long 6, ulong 7, half 8, float 9, double 10
inline int st_key_size(int t) { return t < 0 || t > 10 ? 0 : t == 8 ? 2 : t == 9 ? 4 : t == 10 ? 8 : 1 << (t >> 1); }
inline int st_key_kind(int t) { return t >= 8 ? 2 : (t & 1) ? 0 : 1; }

// the parts of the workspace, in order
struct st_layout { size_t ends, tsum, flags, segid, info, ck, cr, total; };
inline st_layout st_layout_of(size_t numel_seg, size_t numel, size_t k, int key_size) {
	st_layout l;
	const size_t tiles = st_tiles(numel);
	size_t at = 0;
	l.ends = at; at += clo_op_ws_align(numel_seg * sizeof(st_u64));
	l.tsum = at; at += clo_op_ws_align((clo_op_ends_tiles(numel_seg) + 1) * sizeof(st_u64));
	l.flags = at; at += clo_op_ws_align(tiles * ST_TILE);
	l.segid = at; at += clo_op_ws_align(tiles * ST_TILE * sizeof(unsigned));
	l.info = at; at += clo_op_ws_align(tiles * ST_INFO * sizeof(unsigned));
	l.ck = at; at += clo_op_ws_align(tiles * 2 * k * (size_t) key_size);
	l.cr = at; at += clo_op_ws_align(tiles * 2 * k * sizeof(unsigned));
	l.total = at;
	return l;
}

}  // namespace

extern "C" {

size_t clo_hip_segtopk_tile(int key_size, int value_size) {
	return clo_op_key_size_ok(key_size) && clo_op_value_size_ok(value_size) ? ST_TILE : 0;
}

size_t clo_hip_segtopk_k_max(int key_size, int value_size) {
	return clo_op_key_size_ok(key_size) && clo_op_value_size_ok(value_size) ? ST_K_MAX : 0;
}

size_t clo_hip_segtopk_workspace_bytes(size_t numel_seg, size_t numel, size_t k, int key_size, int value_size) {
	if (numel_seg == 0 && numel == 0) return 0;
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return st_layout_of(numel_seg, numel, k, key_size).total;
}

int clo_hip_segtopk(int which, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, uint32_t* counts_out, uint64_t* num_out, size_t numel_seg, size_t numel, size_t k, int key_type, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (which != CLO_HIP_SEGTOPK_SMALLEST && which != CLO_HIP_SEGTOPK_LARGEST) return CLO_HIP_EARGS;
	if (form != CLO_HIP_SEGTOPK_COUNTS && form != CLO_HIP_SEGTOPK_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int ks = st_key_size(key_type);
	if (ks == 0 || !clo_op_value_size_ok(value_size)) return CLO_HIP_EUNSUPPORTED;
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (k > ST_K_MAX || (unsigned long long) numel_seg * k > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGTOPK_OFFSETS)) return CLO_HIP_EARGS;
	if (!keys_in && numel > 0) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	if (value_size == 8 && !values_in) return CLO_HIP_EARGS;
	const bool arg = value_size == 4 && !values_in;
	if (!keys_out && !arg) return CLO_HIP_EARGS;
	if (!counts_out && numel_seg > 0 && k > 0) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8) || clo_misaligned(num_in, 8) || clo_misaligned(counts_out, 4)) return CLO_HIP_EARGS;
	if (clo_misaligned(counts_or_offsets, (size_t) count_size) || clo_misaligned(keys_in, (size_t) ks) || clo_misaligned(keys_out, (size_t) ks)) return CLO_HIP_EARGS;
	if (value_size > 0 && (clo_misaligned(values_in, (size_t) value_size) || clo_misaligned(values_out, (size_t) value_size))) return CLO_HIP_EARGS;
	if (numel_seg == 0) {
		hipLaunchKernelGGL(clo_segtopk_empty_kernel, dim3(1), dim3(1), 0, (hipStream_t) stream, (st_u64*) num_out);
		return (int) hipGetLastError();
	}
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	const st_layout l = st_layout_of(numel_seg, numel, k, ks);
	if (workspace_bytes < l.total) return CLO_HIP_EWORKSPACE;

	char* const ws = (char*) workspace;
	st_args a;
	a.src = counts_or_offsets; a.num_in = (const st_u64*) num_in; a.kin = keys_in; a.vin = values_in;
	a.kout = keys_out; a.vout = values_out; a.counts_out = counts_out; a.num_out = (st_u64*) num_out;
	a.m_h = (unsigned) numel_seg; a.n = (unsigned) numel; a.k = (unsigned) k; a.largest = which == CLO_HIP_SEGTOPK_LARGEST;
	a.s = (hipStream_t) stream;
	a.kx = clo_keyx_make(st_key_kind(key_type), 0, 8 * ks);
	a.ends = (st_u64*) (ws + l.ends); a.tsum = (st_u64*) (ws + l.tsum);
	a.flags = (unsigned char*) (ws + l.flags); a.segid = (unsigned*) (ws + l.segid); a.info = (unsigned*) (ws + l.info);
	a.ck = ws + l.ck; a.cr = (unsigned*) (ws + l.cr);
	const unsigned tiles = (unsigned) st_tiles(numel);
	int st;
	if (form == CLO_HIP_SEGTOPK_OFFSETS) st = count_size == 8 ? st_launch_heads<uint64_t, true>(a, tiles) : st_launch_heads<uint32_t, true>(a, tiles);
	else st = count_size == 8 ? st_launch_heads<uint64_t, false>(a, tiles) : st_launch_heads<uint32_t, false>(a, tiles);
	if (st != 0 || tiles == 0u || k == 0) return st;   // k == 0: num_out alone
	const int mode = clo_op_mode(value_size, arg);
	switch (ks) {
		case 1: return st_dispatch_mode<uint8_t>(a, tiles, mode);
		case 2: return st_dispatch_mode<uint16_t>(a, tiles, mode);
		case 4: return st_dispatch_mode<uint32_t>(a, tiles, mode);
		default: return st_dispatch_mode<uint64_t>(a, tiles, mode);
	}
}

}  // extern "C"
