// clo_hip_join.hip — the equi-join of two sorted key arrays as pairs of row indices (CloJoin, include/clo_join.h; not
// upstream): inner, left, right and full outer, the rows in ascending key order.
//
// Every element of the stable merge of A and B is an EMITTER of a number of consecutive result rows. With x its key,
// [lbA, ubA) the run of x in A and [lbB, ubB) the run of x in B:
//   A[i], ubB > lbB    ubB - lbB rows (i, lbB + r), r the row's rank within the emitter
//   A[i], ubB == lbB   one row (i, NONE) for left and full joins, none otherwise
//   B[j], ubA == lbA   one row (NONE, j) for right and full joins, none otherwise
//   B[j], ubA > lbA    none: the A rows of x, which the merge puts before it, have emitted the pairs.
// The emitters in merge order give the rows in the order of the contract: keys ascending, i before j inside a key.
//
// Five launches, none of which waits for another work-group and none of which uses a global atomic:
//   PARTITION  the merge's diagonal search, one thread per tile boundary of the merged sequence -> split[tiles + 1];
//   COUNT      one work-group per merged tile: stages its ranges of A and B in LDS, merges, finds every element's run
//              bounds as the set operations do (inside the tile from the staged keys; the runs of the tile's first and
//              last key, which alone can reach outside it, by four lanes' searches in global memory) and from them the
//              rows it emits. Writes the tile's rows (64 bits) and the number of its emitters that emit at all, and,
//              unless only the count is wanted, one 16-byte entry per such emitter, compacted at the front of the tile's
//              part of the table: the inclusive end of its rows WITHIN the tile (64 bits), idx_a and the first idx_b.
//              An element that emits nothing — every row of B in an inner join, every row without a partner — leaves
//              no trace;
//   SCAN       one work-group: the tiles' rows and emitters -> exclusive offsets in place, *num_out = K (never clamped),
//              and the companion count min(K, capacity) behind the row offsets, which is all the write looks at;
//   FIRST      one thread per boundary t * T of the OUTPUT tiles: first[t] = the number of emitters whose rows end at or
//              before row t * T — a search for the merged tile among the row offsets, then among that tile's entries;
//   WRITE      one work-group per output tile of T rows, so that the work follows the rows and not the inputs: a row
//              with 2^20 matches is written by 2^20 / T work-groups. Every emitter has a row, so at most T of them end
//              inside the tile: each marks the row after its end in LDS, and a max scan gives every row its emitter and
//              rank (CloExpand's schedule, restated; its fallback for more ends than marks cannot occur here).
// Whatever the arrays hold: splits are clamped, every search reads inside [0, na), [0, nb), the staged range or the
// workspace's arrays; COUNT decides from the same data the counts and the entries, so the offsets and the table agree;
// what comes out of the workspace is clamped (first[], a tile's emitters, an entry's place, idx_a below na, idx_b below
// nb) and a row is stored only below the capacity.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

typedef unsigned long long join_u64;

constexpr int JOIN_THREADS = 256;
static_assert(JOIN_THREADS == CLO_OP_THREADS, "the shared helpers stride by CLO_OP_THREADS");
constexpr int JOIN_WAVES = JOIN_THREADS / 64;
constexpr int join_items(int key_size) { return key_size <= 2 ? 17 : 9; }
constexpr size_t join_tile(int key_size) { return (size_t) JOIN_THREADS * join_items(key_size); }
constexpr size_t JOIN_MIN_TILE = join_tile(8);                  // sizes the workspace, whose getter does not know the key size
constexpr unsigned JOIN_SCAN_ITEMS = 8;
constexpr unsigned JOIN_OUT_LOG2 = 11;
constexpr unsigned JOIN_OUT_TILE = 1u << JOIN_OUT_LOG2;          // T: result rows per work-group of the write
constexpr unsigned JOIN_OUT_PER_THREAD = JOIN_OUT_TILE / JOIN_THREADS;
static_assert(((join_u64) (JOIN_OUT_TILE + 1u) << JOIN_OUT_LOG2) < (1ull << 32), "a mark, (emitter << 11 | row), is one word");
constexpr unsigned JOIN_NONE = 0xffffffffu;

// one emitter: the inclusive end of its rows within its merged tile, idx_a (or NONE) and the idx_b of its first row (or NONE)
struct __attribute__((aligned(16))) join_entry { join_u64 end; unsigned da, db; };
static_assert(sizeof(join_entry) == 16, "one 16-byte store");

inline bool join_emits_a(int kind) { return kind == CLO_HIP_JOIN_LEFT || kind == CLO_HIP_JOIN_FULL; }
inline bool join_emits_b(int kind) { return kind == CLO_HIP_JOIN_RIGHT || kind == CLO_HIP_JOIN_FULL; }

// the largest K of a join of these sizes, saturating: one key everywhere, or nothing shared
inline size_t join_max_rows(int kind, size_t na, size_t nb) {
	size_t prod = 0;
	if (na > 0 && nb > 0) prod = na > SIZE_MAX / nb ? SIZE_MAX : na * nb;
	size_t alone = 0;
	if (join_emits_a(kind)) alone += na;
	if (join_emits_b(kind)) alone = alone + nb < alone ? SIZE_MAX : alone + nb;
	return prod > alone ? prod : alone;
}

// The first index in [lo, hi) whose key is not below x (UPPER: is above x), hi if there is none. Reads k[lo, hi) only.
template <typename TK, bool XF, bool UPPER>
__device__ __forceinline__ unsigned join_bound(const TK* k, unsigned lo, unsigned hi, TK x, const clo_keyx& kx) {
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		TK y = k[mid];
		if constexpr (XF) y = clo_keyx_fwd<TK>(y, kx);
		if (UPPER ? y <= x : y < x) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

template <typename TK>
__global__ __launch_bounds__(JOIN_THREADS)
void clo_join_partition_kernel(const TK* __restrict__ ka, const TK* __restrict__ kb, unsigned na, unsigned nb, unsigned tiles,
	clo_keyx kx, unsigned* __restrict__ split) {
	clo_op_partition<TK, join_tile((int) sizeof(TK))>(ka, kb, na, nb, tiles, kx, split);
}

// The exclusive sum of v over the work-group's threads and the sum of all, in 64 bits. One barrier; s_wave must not be
// written again before every thread has left.
__device__ __forceinline__ join_u64 join_block_scan(join_u64 v, join_u64* s_wave, unsigned tid, join_u64& total) {
	const join_u64 inc = clo_wave_scan_inclusive<join_u64>(v, 0u);
	if ((tid & 63u) == 63u) s_wave[tid >> 6] = inc;
	__syncthreads();
	join_u64 before = 0;
	total = 0;
	#pragma unroll
	for (unsigned w = 0; w < (unsigned) JOIN_WAVES; ++w) {
		const join_u64 s = s_wave[w];
		if (w < (tid >> 6)) before += s;
		total += s;
	}
	return before + inc - v;
}

// Lane 0 of wave w loads the key next to the tile that decides whether a run reaches outside it: w = 0 A[a0 - 1], 1
// B[b0 - 1], 2 A[a1], 3 B[b1] (unsigned order; ok: there is one). Requested before the tile is staged.
template <typename TK>
__device__ __forceinline__ TK join_neighbour(const TK* __restrict__ ka, const TK* __restrict__ kb, unsigned na, unsigned nb,
	const clo_op_range& r, const clo_keyx& kx, unsigned tid, bool& ok) {
	ok = false;
	if ((tid & 63u) != 0) return (TK) 0;
	const unsigned w = tid >> 6, a1 = r.a0 + r.na_t, b1 = r.b0 + r.nb_t;
	const TK* k = (w & 1u) ? kb : ka;
	const unsigned i = w == 0 ? r.a0 - 1u : w == 1 ? r.b0 - 1u : w == 2 ? a1 : b1;
	ok = w == 0 ? r.a0 > 0 : w == 1 ? r.b0 > 0 : w == 2 ? a1 < na : b1 < nb;
	return ok ? clo_keyx_fwd<TK>(k[i], kx) : (TK) 0;
}

// After the tile's keys are staged (A at s_keys[0, na_t), B behind it, unsigned order) and a barrier: merges this
// thread's ITEMS elements and says for each how many rows it emits (rows[i]) and what they hold: idx_a da[i] and the
// idx_b of the first of them db[i], either of which may be NONE. Elements past the tile's count emit nothing. One
// barrier inside. s_g: four words of LDS. Whatever the keys hold, da[i] < na or NONE and db[i] + rows[i] <= nb or db[i]
// NONE.
template <typename TK, int ITEMS>
__device__ __forceinline__ void join_decide(const TK* __restrict__ ka, const TK* __restrict__ kb, unsigned na, unsigned nb,
	const clo_op_range& r, const TK* s_keys, unsigned* s_g, TK nbr, bool nbr_ok, bool emits_a, bool emits_b, const clo_keyx& kx, unsigned tid,
	unsigned (&rows)[ITEMS], unsigned (&da)[ITEMS], unsigned (&db)[ITEMS]) {
	constexpr unsigned TILE = (unsigned) JOIN_THREADS * ITEMS;
	const unsigned na_t = r.na_t, nb_t = r.nb_t, cnt = r.cnt, a0 = r.a0, b0 = r.b0;
	const TK* sa = s_keys;
	const TK* sb = s_keys + na_t;
	// the tile's first and last key (cnt > 0): only their runs can begin before the tile or end after it
	const TK a_lo = s_keys[0], a_hi = s_keys[na_t > 0 ? na_t - 1u : 0u], b_lo = s_keys[clo_op_min(na_t, TILE - 1u)], b_hi = s_keys[cnt - 1u];
	const TK kfirst = na_t == 0 ? b_lo : nb_t == 0 ? a_lo : (a_lo < b_lo ? a_lo : b_lo);
	const TK klast = na_t == 0 ? b_hi : nb_t == 0 ? a_hi : (a_hi > b_hi ? a_hi : b_hi);
	if ((tid & 63u) == 0) {
		const unsigned w = tid >> 6, a1 = a0 + na_t, b1 = b0 + nb_t;
		unsigned g;
		if (w == 0) { g = a0; if (nbr_ok && nbr == kfirst) g = join_bound<TK, true, false>(ka, 0u, a0 - 1u, kfirst, kx); }
		else if (w == 1) { g = b0; if (nbr_ok && nbr == kfirst) g = join_bound<TK, true, false>(kb, 0u, b0 - 1u, kfirst, kx); }
		else if (w == 2) { g = a1; if (nbr_ok && nbr == klast) g = join_bound<TK, true, true>(ka, a1 + 1u, na, klast, kx); }
		else { g = b1; if (nbr_ok && nbr == klast) g = join_bound<TK, true, true>(kb, b1 + 1u, nb, klast, kx); }
		s_g[w] = g;
	}
	// this thread's ITEMS elements start at diagonal tid * ITEMS of the tile; past cnt nothing is valid
	const unsigned diag = clo_op_min(tid * ITEMS, cnt);
	unsigned ai = clo_op_path<TK, false>(sa, sb, na_t, nb_t, diag, kx);
	unsigned bi = diag - ai;
	__syncthreads();
	const unsigned g_lba = s_g[0], g_lbb = s_g[1], g_uba = s_g[2], g_ubb = s_g[3];

	TK x = s_keys[clo_op_min(ai, TILE - 1u)], y = s_keys[clo_op_min(na_t + bi, TILE - 1u)];
	// the keys just before them, pa = A[ai - 1] and pb = B[bi - 1] where there are such: carried along in registers
	bool has_pa = ai > 0, has_pb = bi > 0;
	TK pa = s_keys[has_pa ? ai - 1u : 0u], pb = s_keys[has_pb ? na_t + bi - 1u : 0u];
	bool c_valid = false, c_ub_valid = false;   // the bounds of c_key inside the tile, found once per distinct key
	TK c_key = 0;
	unsigned c_lba = 0, c_lbb = 0, c_ubb = 0;
	#pragma unroll
	for (int i = 0; i < ITEMS; ++i) {
		// x is looked at only while ai < na_t, y only while bi < nb_t
		const bool from_a = bi >= nb_t || (ai < na_t && x <= y);
		const TK key = from_a ? x : y;
		rows[i] = 0u;
		da[i] = JOIN_NONE;
		db[i] = JOIN_NONE;
		if (tid * ITEMS + i < cnt) {
			if (!c_valid || key != c_key) {
				// everything of A below ai is <= key, everything of B below bi is <= key (< key for an element of A)
				c_lba = (has_pa && pa == key) ? join_bound<TK, false, false>(sa, 0u, ai - 1u, key, kx) : ai;
				c_lbb = (has_pb && pb == key) ? join_bound<TK, false, false>(sb, 0u, bi - 1u, key, kx) : bi;
				c_key = key;
				c_valid = true;
				c_ub_valid = false;
			}
			const bool is_first = key == kfirst, is_last = key == klast;
			const unsigned lba = is_first ? g_lba : a0 + c_lba, lbb = is_first ? g_lbb : b0 + c_lbb;
			if (from_a) {
				if (!c_ub_valid) {   // B[bi] is the first key of B not below this one
					c_ubb = (bi < nb_t && y == key) ? join_bound<TK, false, true>(sb, bi + 1u, nb_t, key, kx) : bi;
					c_ub_valid = true;
				}
				const unsigned ubb = is_last ? g_ubb : b0 + c_ubb;   // <= nb
				const unsigned n = ubb > lbb ? ubb - lbb : 0u;
				da[i] = a0 + ai;
				if (n > 0u) { rows[i] = n; db[i] = lbb; }
				else rows[i] = emits_a ? 1u : 0u;
			} else {             // A[ai] is the first key of A above this one
				const unsigned uba = is_last ? g_uba : a0 + ai;
				if (!(uba > lba) && emits_b) { rows[i] = 1u; db[i] = b0 + bi; }
			}
		}
		if (from_a) { pa = x; has_pa = true; ++ai; } else { pb = y; has_pb = true; ++bi; }
		const TK next = s_keys[clo_op_min(from_a ? ai : na_t + bi, TILE - 1u)];
		if (from_a) x = next; else y = next;
	}
}

// The tile's rows and its emitters (the elements that emit at least one row) go through ONE 64-bit scan: the rows above
// bit JOIN_ECNT_BITS, the emitters below it. A tile has at most 4352 emitters and 4352 * (2^32 - 1) rows.
constexpr unsigned JOIN_ECNT_BITS = 13;
static_assert(join_tile(1) < (1u << JOIN_ECNT_BITS) && join_tile(8) < (1u << JOIN_ECNT_BITS), "a tile's emitters fit the low bits");

// Writes the tile's rows (tsum) and emitters (ecnt) and, unless table is NULL (the count form), the entries of its
// emitters, compacted in merge order at the front of the tile's TILE entries of the table.
template <typename TK>
__global__ __launch_bounds__(JOIN_THREADS)
void clo_join_count_kernel(const TK* __restrict__ ka, unsigned na, const TK* __restrict__ kb, unsigned nb,
	const unsigned* __restrict__ split, join_u64* __restrict__ tsum, unsigned* __restrict__ ecnt, join_entry* __restrict__ table,
	int emits_a, int emits_b, clo_keyx kx) {
	constexpr int ITEMS = join_items((int) sizeof(TK));
	constexpr unsigned TILE = (unsigned) join_tile((int) sizeof(TK));
	__shared__ __attribute__((aligned(16))) TK s_keys[TILE];
	__shared__ unsigned s_g[4];
	__shared__ join_u64 s_wave[JOIN_WAVES];
	const unsigned tid = threadIdx.x;
	const clo_op_range r = clo_op_tile_range<TILE>(split, na, nb);
	bool nbr_ok;
	const TK nbr = join_neighbour<TK>(ka, kb, na, nb, r, kx, tid, nbr_ok);
	clo_op_stage<TK, true>(ka + r.a0, r.na_t, s_keys, kx, tid);
	clo_op_stage<TK, true>(kb + r.b0, r.nb_t, s_keys + r.na_t, kx, tid);
	__syncthreads();
	unsigned rows[ITEMS], da[ITEMS], db[ITEMS];
	join_decide<TK, ITEMS>(ka, kb, na, nb, r, s_keys, s_g, nbr, nbr_ok, emits_a != 0, emits_b != 0, kx, tid, rows, da, db);
	join_u64 sum = 0;
	#pragma unroll
	for (int i = 0; i < ITEMS; ++i) sum += ((join_u64) rows[i] << JOIN_ECNT_BITS) | (rows[i] > 0u ? 1u : 0u);
	join_u64 total;
	const join_u64 before = join_block_scan(sum, s_wave, tid, total);
	if (tid == 0) {
		tsum[blockIdx.x] = total >> JOIN_ECNT_BITS;
		ecnt[blockIdx.x] = (unsigned) total & ((1u << JOIN_ECNT_BITS) - 1u);
	}
	if (table) {
		join_u64 at = before >> JOIN_ECNT_BITS;
		unsigned pos = (unsigned) before & ((1u << JOIN_ECNT_BITS) - 1u);   // < the tile's emitters <= cnt
		join_entry* mine = table + (size_t) blockIdx.x * TILE;                // the last tile: d0 + pos < d0 + cnt = na + nb
		#pragma unroll
		for (int i = 0; i < ITEMS; ++i) {
			at += rows[i];
			if (rows[i] > 0u) {   // only an element below cnt emits
				join_entry e;
				e.end = at; e.da = da[i]; e.db = db[i];
				mine[pos++] = e;
			}
		}
	}
}

// tsum[0, tiles) and ecnt[0, tiles) -> their exclusive sums in place; *num_out = K, the sum of all rows; tsum[tiles] =
// min(K, cap), the rows to write; ecnt[tiles] = the emitters of all tiles. One work-group. tiles 0: only num_out.
__global__ __launch_bounds__(JOIN_THREADS)
void clo_join_scan_kernel(join_u64* __restrict__ tsum, unsigned* __restrict__ ecnt, unsigned tiles, join_u64 cap, join_u64* __restrict__ num_out) {
	constexpr unsigned SWEEP = JOIN_THREADS * JOIN_SCAN_ITEMS;
	__shared__ join_u64 s_wave[JOIN_WAVES];
	const unsigned tid = threadIdx.x;
	join_u64 carry = 0;     // at most (numel_a + numel_b) * numel_b < 2^64
	join_u64 ecarry = 0;    // at most numel_a + numel_b
	for (unsigned base = 0; base < tiles; base += SWEEP) {
		join_u64 v[JOIN_SCAN_ITEMS], sum = 0, esum = 0;
		unsigned w[JOIN_SCAN_ITEMS];
		#pragma unroll
		for (unsigned c = 0; c < JOIN_SCAN_ITEMS; ++c) {
			const unsigned i = base + tid * JOIN_SCAN_ITEMS + c;   // < tiles + SWEEP: no wrap, tiles < 2^21
			v[c] = i < tiles ? tsum[i] : 0ull;
			w[c] = i < tiles ? ecnt[i] : 0u;
			sum += v[c];
			esum += w[c];
		}
		join_u64 total, etotal;
		join_u64 at = carry + join_block_scan(sum, s_wave, tid, total);
		__syncthreads();   // s_wave is written again
		join_u64 eat = ecarry + join_block_scan(esum, s_wave, tid, etotal);
		#pragma unroll
		for (unsigned c = 0; c < JOIN_SCAN_ITEMS; ++c) {
			const unsigned i = base + tid * JOIN_SCAN_ITEMS + c;
			if (i < tiles) { tsum[i] = at; ecnt[i] = (unsigned) eat; }
			at += v[c];
			eat += w[c];
		}
		carry += total;
		ecarry += etotal;
		__syncthreads();   // s_wave is written again
	}
	if (tid == 0) {
		*num_out = carry;
		if (tiles > 0u) { tsum[tiles] = carry < cap ? carry : cap; ecnt[tiles] = (unsigned) ecarry; }
	}
}

__device__ __forceinline__ join_u64 join_min64(join_u64 a, join_u64 b) { return a < b ? a : b; }

// What the scan left: off[t] the rows before merged tile t, eoff[t] the emitters before it (t <= tiles: all of them),
// and the tiles' entries. Emitter g in [0, eoff[tiles]) is entry g - eoff[t] of the tile t it falls in; its rows end
// at off[t] + that entry's end.
template <unsigned TILE>
struct join_table {
	const join_u64* off; const unsigned* eoff; const join_entry* table; unsigned tiles, n;

	// how many of x[lo, hi) are <= v, the x ascending
	template <typename T>
	__device__ __forceinline__ static unsigned below(const T* x, unsigned lo, unsigned hi, T v) {
		while (lo < hi) {
			const unsigned mid = lo + ((hi - lo) >> 1);
			if (x[mid] <= v) lo = mid + 1u; else hi = mid;
		}
		return lo;
	}
	// the emitters of tile t, never more than a tile has elements
	__device__ __forceinline__ unsigned count(unsigned t) const { const unsigned a = eoff[t], b = eoff[t + 1u]; return b > a ? clo_op_min(b - a, TILE) : 0u; }
	// where entry l of tile t lies, clamped into the table's n entries
	__device__ __forceinline__ unsigned index(unsigned t, unsigned l) const { return (unsigned) join_min64((join_u64) t * TILE + l, (join_u64) n - 1u); }
	// the number of emitters whose rows end at or before row x
	__device__ __forceinline__ unsigned first(join_u64 x) const {
		const unsigned hi = below<join_u64>(off, 0u, tiles, x);   // the tiles that begin at or before x
		if (hi == 0u) return 0u;
		const unsigned t = hi - 1u, c = count(t);
		const join_u64 base = off[t];
		unsigned lo = 0, up = c;
		while (lo < up) {
			const unsigned mid = lo + ((up - lo) >> 1);
			if (base + table[index(t, mid)].end <= x) lo = mid + 1u; else up = mid;
		}
		return eoff[t] + lo;
	}
};

template <unsigned TILE>
__global__ __launch_bounds__(JOIN_THREADS)
void clo_join_first_kernel(const join_u64* __restrict__ off, const unsigned* __restrict__ eoff, const join_entry* __restrict__ table,
	unsigned tiles, unsigned n, unsigned out_tiles, unsigned* __restrict__ first) {
	const unsigned t = blockIdx.x * JOIN_THREADS + threadIdx.x;
	if (t > out_tiles) return;
	const join_table<TILE> e = { off, eoff, table, tiles, n };
	first[t] = e.first((join_u64) t << JOIN_OUT_LOG2);
}

// inclusive max scan of the 64 lanes of a wave: clo_wave_scan_inclusive's network with max, whose identity is 0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned join_max_step(unsigned x) { return clo_op_max(x, clo_op_dpp<CTRL, ROW_MASK, unsigned>(0u, x)); }
__device__ __forceinline__ unsigned join_wave_max_scan(unsigned x) {
	x = join_max_step<0x111, 0xF>(x);   // row_shr:1
	x = join_max_step<0x112, 0xF>(x);   // row_shr:2
	x = join_max_step<0x114, 0xF>(x);   // row_shr:4
	x = join_max_step<0x118, 0xF>(x);   // row_shr:8
	x = join_max_step<0x142, 0xA>(x);   // row_bcast:15 into rows 1 and 3
	x = join_max_step<0x143, 0xC>(x);   // row_bcast:31 into rows 2 and 3
	return x;
}

// One work-group per T rows of the result. Every emitter has at least one row, so at most T of them end inside the
// tile: emitter f0 + k, whose rows end at row `at` of the tile, marks row `at` — the first row of emitter f0 + k + 1 —
// with (k + 1) << 11 | at, and an inclusive max scan over the rows gives every row its emitter and where that began
// (CloExpand's schedule, restated). s_entry[k] is where emitter f0 + k's entry lies, for the ne + 1 emitters of the tile.
template <typename TK>
__global__ __launch_bounds__(JOIN_THREADS)
void clo_join_write_kernel(const TK* __restrict__ ka, unsigned na, const TK* __restrict__ kb, unsigned nb,
	const join_u64* __restrict__ off, const unsigned* __restrict__ eoff, const join_entry* __restrict__ table, unsigned tiles,
	const unsigned* __restrict__ first, unsigned* __restrict__ ia_out, unsigned* __restrict__ ib_out, TK* __restrict__ kout, unsigned capacity) {
	constexpr unsigned TILE = (unsigned) join_tile((int) sizeof(TK));
	__shared__ __attribute__((aligned(16))) unsigned s_row[JOIN_OUT_TILE];
	__shared__ unsigned s_entry[JOIN_OUT_TILE + 1];
	__shared__ unsigned s_wave[JOIN_WAVES];
	__shared__ join_u64 s_start0;
	typedef unsigned vec4 __attribute__((ext_vector_type(4)));
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const join_table<TILE> e = { off, eoff, table, tiles, na + nb };   // na + nb > 0
	// the rows there are to write: the scan's companion count, min(K, capacity). (The stores below have a clamp of
	// their own, and the grid has no work-group beyond the capacity.)
	const join_u64 lim = off[tiles];
	const join_u64 row0 = (join_u64) blockIdx.x << JOIN_OUT_LOG2;
	if (row0 >= lim) return;   // the whole work-group
	const unsigned cnt = lim - row0 < JOIN_OUT_TILE ? (unsigned) (lim - row0) : JOIN_OUT_TILE;
	// the tile's emitters: what FIRST found, clamped to the emitters there are, ordered, and at most T of them
	const unsigned all = eoff[tiles];
	const unsigned f0 = clo_op_min(first[blockIdx.x], all);
	const unsigned f1 = clo_op_min(clo_op_max(first[blockIdx.x + 1u], f0), all);
	const unsigned ne = clo_op_min(f1 - f0, JOIN_OUT_TILE);   // the ends in (row0, row0 + T]
	// the merged tiles they lie in (the same for every thread)
	const unsigned t_lo = clo_op_max(join_table<TILE>::template below<unsigned>(eoff, 0u, tiles, f0), 1u) - 1u;
	const unsigned t_hi = clo_op_max(join_table<TILE>::template below<unsigned>(eoff, t_lo, tiles, f0 + ne), t_lo + 1u) - 1u;

	if (ne > 0u) {
		#pragma unroll
		for (unsigned i = 0; i < JOIN_OUT_PER_THREAD / 4u; ++i) reinterpret_cast<vec4*>(s_row)[tid + i * JOIN_THREADS] = vec4(0u);
		__syncthreads();
	}
	for (unsigned k = tid; k <= ne; k += JOIN_THREADS) {
		const unsigned g = f0 + k;   // <= all
		const unsigned t = clo_op_max(join_table<TILE>::template below<unsigned>(eoff, t_lo, t_hi + 1u, g), t_lo + 1u) - 1u;
		const unsigned l = clo_op_min(g - eoff[t], TILE - 1u);   // (g == all: an entry no row below lim belongs to)
		const unsigned idx = e.index(t, l);
		s_entry[k] = idx;
		if (k == 0u) s_start0 = off[t] + (l > 0u && idx > 0u ? table[idx - 1u].end : 0ull);   // where emitter f0 began
		if (k < ne) {
			const join_u64 at = off[t] + table[idx].end - row0;   // an end below row0 wraps to above T
			if (at < JOIN_OUT_TILE) atomicMax(&s_row[(unsigned) at], ((k + 1u) << JOIN_OUT_LOG2) | (unsigned) at);
		}
	}
	__syncthreads();
	if (ne > 0u) {
		// the inclusive max scan over the rows: 8 consecutive rows per thread, the lanes, the waves
		unsigned v[JOIN_OUT_PER_THREAD];
		#pragma unroll
		for (unsigned i = 0; i < JOIN_OUT_PER_THREAD / 4u; ++i) {
			const vec4 x = reinterpret_cast<const vec4*>(s_row)[tid * (JOIN_OUT_PER_THREAD / 4u) + i];
			v[4 * i] = x.x; v[4 * i + 1] = x.y; v[4 * i + 2] = x.z; v[4 * i + 3] = x.w;
		}
		#pragma unroll
		for (unsigned i = 1; i < JOIN_OUT_PER_THREAD; ++i) v[i] = clo_op_max(v[i], v[i - 1]);
		const unsigned incl = join_wave_max_scan(v[JOIN_OUT_PER_THREAD - 1]);
		if (lane == 63u) s_wave[wave] = incl;
		unsigned carry = clo_op_shfl<unsigned>(incl, (int) lane - 1);
		if (lane == 0u) carry = 0u;
		__syncthreads();
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) JOIN_WAVES; ++w) {
			const unsigned s = s_wave[w];
			if (w < wave) carry = clo_op_max(carry, s);
		}
		#pragma unroll
		for (unsigned i = 0; i < JOIN_OUT_PER_THREAD / 4u; ++i) {
			vec4 x;
			x.x = clo_op_max(v[4 * i], carry); x.y = clo_op_max(v[4 * i + 1], carry);
			x.z = clo_op_max(v[4 * i + 2], carry); x.w = clo_op_max(v[4 * i + 3], carry);
			reinterpret_cast<vec4*>(s_row)[tid * (JOIN_OUT_PER_THREAD / 4u) + i] = x;
		}
		__syncthreads();
	}

	const join_u64 start0 = s_start0;
	for (unsigned j = tid; j < cnt; j += JOIN_THREADS) {
		const unsigned mark = ne > 0u ? s_row[j] : 0u;
		const unsigned k = mark >> JOIN_OUT_LOG2;   // <= ne
		const unsigned rank = k == 0u ? (unsigned) (row0 + j - start0) : j - (mark & (JOIN_OUT_TILE - 1u));
		const join_entry* en = table + s_entry[k];
		// every index is clamped below its side's numel: nothing else is written or gathered by
		const unsigned da = en->da, db = en->db;
		const unsigned ia = da == JOIN_NONE || na == 0u ? JOIN_NONE : clo_op_min(da, na - 1u);
		unsigned ib = JOIN_NONE;
		if (db != JOIN_NONE && nb > 0u) {
			const join_u64 b = (join_u64) db + rank;
			ib = b < nb ? (unsigned) b : nb - 1u;
		}
		const join_u64 row = row0 + j;
		if (row < capacity) {
			if (ia_out) ia_out[row] = ia;
			if (ib_out) ib_out[row] = ib;
			if (kout) kout[row] = ia != JOIN_NONE ? ka[ia] : ib != JOIN_NONE ? kb[ib] : (TK) 0;
		}
	}
}

struct join_args {
	const void* ka; const void* kb; unsigned* ia; unsigned* ib; void* kout; join_u64* num_out;
	unsigned na, nb, cap, out_tiles; int kind; clo_keyx kx;
	unsigned* split; join_u64* off; unsigned* eoff; join_entry* table; unsigned* first; hipStream_t s;
};

inline int join_scan_launch(join_u64* tsum, unsigned* ecnt, unsigned tiles, unsigned cap, join_u64* num_out, hipStream_t s) {
	clo_timing_scope timing("join_scan", s);
	hipLaunchKernelGGL(clo_join_scan_kernel, dim3(1), dim3(JOIN_THREADS), 0, s, tsum, ecnt, tiles, (join_u64) cap, num_out);
	return (int) hipGetLastError();
}

template <typename TK>
int join_launch(const join_args& a) {
	constexpr unsigned TILE = (unsigned) join_tile((int) sizeof(TK));
	const unsigned n = a.na + a.nb, tiles = (unsigned) (((size_t) n + TILE - 1) / TILE);
	const bool write = a.out_tiles > 0u;
	{
		clo_timing_scope timing("join_partition", a.s);
		hipLaunchKernelGGL((clo_join_partition_kernel<TK>), dim3(tiles / JOIN_THREADS + 1u), dim3(JOIN_THREADS), 0, a.s,
			(const TK*) a.ka, (const TK*) a.kb, a.na, a.nb, tiles, a.kx, a.split);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("join_count", a.s);
		hipLaunchKernelGGL((clo_join_count_kernel<TK>), dim3(tiles), dim3(JOIN_THREADS), 0, a.s,
			(const TK*) a.ka, a.na, (const TK*) a.kb, a.nb, (const unsigned*) a.split, a.off, a.eoff, write ? a.table : (join_entry*) nullptr,
			(int) join_emits_a(a.kind), (int) join_emits_b(a.kind), a.kx);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	const int st = join_scan_launch(a.off, a.eoff, tiles, a.cap, a.num_out, a.s);
	if (st != 0 || !write) return st;
	{
		clo_timing_scope timing("join_first", a.s);
		hipLaunchKernelGGL((clo_join_first_kernel<TILE>), dim3(a.out_tiles / JOIN_THREADS + 1u), dim3(JOIN_THREADS), 0, a.s,
			(const join_u64*) a.off, (const unsigned*) a.eoff, (const join_entry*) a.table, tiles, n, a.out_tiles, a.first);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("join_write", a.s);
	hipLaunchKernelGGL((clo_join_write_kernel<TK>), dim3(a.out_tiles), dim3(JOIN_THREADS), 0, a.s,
		(const TK*) a.ka, a.na, (const TK*) a.kb, a.nb, (const join_u64*) a.off, (const unsigned*) a.eoff, (const join_entry*) a.table, tiles,
		(const unsigned*) a.first, a.ia, a.ib, (TK*) a.kout, a.cap);
	return (int) hipGetLastError();
}

inline size_t join_max_tiles(size_t n) { return (n + JOIN_MIN_TILE - 1) / JOIN_MIN_TILE; }
// the output tiles a join of these sizes can fill, whatever the capacity (which is below 2^32)
inline size_t join_max_out_tiles(int kind, size_t na, size_t nb) {
	const size_t k = join_max_rows(kind, na, nb), rows = k < 0xffffffffull ? k : 0xffffffffull;
	return (rows + JOIN_OUT_TILE - 1) / JOIN_OUT_TILE;
}

}  // namespace

extern "C" {

size_t clo_hip_join_tile(int key_size) { return clo_op_key_size_ok(key_size) ? join_tile(key_size) : 0; }
size_t clo_hip_join_out_tile(void) { return JOIN_OUT_TILE; }

size_t clo_hip_join_workspace_bytes(int kind, size_t numel_a, size_t numel_b) {
	const size_t n = numel_a + numel_b;
	if (n == 0 || n < numel_a || kind < CLO_HIP_JOIN_INNER || kind > CLO_HIP_JOIN_FULL) return 0;
	// the merged tiles' split points; their row offsets and the companion count; their emitter offsets; one entry per
	// merged element; one word per boundary of the output tiles that a join of these sizes can reach
	const size_t t = join_max_tiles(n);
	return clo_op_ws_align((t + 1) * sizeof(unsigned)) + clo_op_ws_align((t + 1) * sizeof(join_u64)) + clo_op_ws_align((t + 1) * sizeof(unsigned))
		+ clo_op_ws_align(n * sizeof(join_entry)) + clo_op_ws_align((join_max_out_tiles(kind, numel_a, numel_b) + 1) * sizeof(unsigned));
}

int clo_hip_join(int kind, const void* keys_a, size_t numel_a, const void* keys_b, size_t numel_b,
	uint32_t* idx_a_out, uint32_t* idx_b_out, void* keys_out, size_t capacity, uint64_t* num_out, int key_size, int key_kind,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (kind < CLO_HIP_JOIN_INNER || kind > CLO_HIP_JOIN_FULL) return CLO_HIP_EARGS;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull || capacity > 0xffffffffull) return CLO_HIP_EARGS;
	if ((numel_a > 0 && !keys_a) || (numel_b > 0 && !keys_b)) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8)) return CLO_HIP_EARGS;
	if (capacity > 0 && !idx_a_out && !idx_b_out && !keys_out) return CLO_HIP_EARGS;
	if (clo_misaligned(keys_a, (size_t) key_size) || clo_misaligned(keys_b, (size_t) key_size) || clo_misaligned(keys_out, (size_t) key_size)
		|| clo_misaligned(idx_a_out, 4) || clo_misaligned(idx_b_out, 4)) return CLO_HIP_EARGS;
	const size_t n = numel_a + numel_b;
	if (n == 0) return join_scan_launch(nullptr, nullptr, 0u, 0u, (join_u64*) num_out, (hipStream_t) stream);   // num_out = 0
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_join_workspace_bytes(kind, numel_a, numel_b)) return CLO_HIP_EWORKSPACE;

	join_args a;
	a.ka = keys_a; a.kb = keys_b; a.ia = idx_a_out; a.ib = idx_b_out; a.kout = keys_out; a.num_out = (join_u64*) num_out;
	a.na = (unsigned) numel_a; a.nb = (unsigned) numel_b; a.cap = (unsigned) capacity; a.kind = kind;
	a.kx = clo_keyx_make(key_kind, 0, 8 * key_size);
	a.s = (hipStream_t) stream;
	// no row at or above min(capacity, the largest K of these sizes) is ever written
	const size_t out_max = join_max_out_tiles(kind, numel_a, numel_b), out_cap = (capacity + JOIN_OUT_TILE - 1) / JOIN_OUT_TILE;
	a.out_tiles = (idx_a_out || idx_b_out || keys_out) ? (unsigned) (out_cap < out_max ? out_cap : out_max) : 0u;
	const size_t t = join_max_tiles(n);
	char* ws = (char*) workspace;
	a.split = (unsigned*) ws;
	ws += clo_op_ws_align((t + 1) * sizeof(unsigned));
	a.off = (join_u64*) ws;
	ws += clo_op_ws_align((t + 1) * sizeof(join_u64));
	a.eoff = (unsigned*) ws;
	ws += clo_op_ws_align((t + 1) * sizeof(unsigned));
	a.table = (join_entry*) ws;
	ws += clo_op_ws_align(n * sizeof(join_entry));
	a.first = (unsigned*) ws;
	return clo_op_by_key_size(key_size, [&](auto tk) { return join_launch<decltype(tk)>(a); });
}

}  // extern "C"
