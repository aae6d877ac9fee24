// clo_hip_topk.hip — the k smallest or largest keys, with values carried along or the indices written (CloTopK,
// include/clo_topk.h; not upstream), without a sort and without a host wait.
//
// Everything works on x = clo_keyx_fwd(key) ^ flip, flip = 0 for "smallest" and all ones for "largest": the m chosen
// elements are the first m of the stable ascending sort by x. Radix select on x, most significant digit first, 8 bits
// per digit (key_size sweeps), then select's count / scan / apply with the ties cut at an exact rank:
//   DIGIT  (per digit) a fixed grid walks the tiles grid-stride; a key whose higher digits equal the prefix found so far
//          is counted under its digit in LDS (32 copies of the 256 counters, copy = lane mod 32, digit-major: the layout
//          of clo_hist_kernel's COPIES form, conflict-free whatever the keys), and the group's counters are ADDED onto
//          the digit's 256-word table in the workspace (cleared by a fill on the stream). Every sweep reads all n keys:
//          the time does not depend on the data.
//   PICK   (per digit) one work-group scans the table, finds the digit that holds the remaining rank and writes the
//          longer prefix and the new remaining rank for the next sweep. After the last digit the prefix is T, the m-th
//          x, the remaining rank r (0-based) says that r + 1 of the elements equal to T are taken, and kth_out gets T
//          mapped back to the key's bits.
//   COUNT  one work-group per tile: how many x < T and how many x == T -> lt[tile], eq[tile];
//   SCAN   one work-group turns both into exclusive offsets in place, the totals behind them;
//   APPLY  keeps an element iff x < T, or x == T and (eq offset of the tile + its rank among the tile's equal ones)
//          <= r; the kept rows are compacted in LDS in input order and stored from row lt offset + min(eq offset, r + 1)
//          on, every store index clamped below m;
//   SORT   ("sorted" only, m <= TOPK_SORTED_MAX) one work-group sorts (x, row) of rows [0, m) in LDS with a bitonic
//          network — the pairs are all distinct, so the result is the stable order — and permutes the rows in place.
// No work-group waits for another; global atomics go to the digit tables alone; nothing is allocated; the host never
// waits. Whatever the arrays hold: loads are bounded by numel, LDS slots by the tile's element count, stores by m.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

constexpr int TOPK_THREADS = 256;
constexpr int TOPK_WAVES = TOPK_THREADS / 64;
constexpr int TOPK_VEC = 4;
constexpr int TOPK_ROW_ELEMS = TOPK_THREADS * TOPK_VEC;   // 1024
static_assert(TOPK_THREADS == CLO_OP_THREADS && TOPK_VEC == CLO_OP_VEC, "the shared helpers' work-group and vector");
constexpr unsigned TOPK_SCAN_ITEMS = 8;                   // the scan sweeps TOPK_THREADS * TOPK_SCAN_ITEMS tiles per trip
static_assert(TOPK_THREADS * TOPK_SCAN_ITEMS == CLO_HIP_TOPK_SCAN_TRIP, "the header names the scan's trip");
constexpr int TOPK_DIGIT_BITS = 8;
constexpr int TOPK_DIGITS = 1 << TOPK_DIGIT_BITS;         // one counter per thread in PICK and in the flush
static_assert(TOPK_DIGITS == TOPK_THREADS, "PICK and the flush take one digit per thread");
constexpr int TOPK_COPIES_LOG2 = 5;                       // 256 digits x 32 copies x 4 bytes = 32 KiB: four groups per CU
constexpr int TOPK_GROUPS_PER_CU = 4;
constexpr int TOPK_SORT_THREADS = 1024;
constexpr unsigned TOPK_SORTED_MAX = 4096;                // (x, row) of 8-byte keys: 48 KiB of the 64 KiB a group declares

// rows per tile: select's shape, the compacted rows of a tile lie in LDS
constexpr int topk_rows(int key_size, int value_size) { return (key_size > value_size ? key_size : value_size) <= 4 ? 8 : 4; }
constexpr size_t topk_tile(int key_size, int value_size) { return (size_t) topk_rows(key_size, value_size) * TOPK_ROW_ELEMS; }

// the modes CLO_OP_KEYS, V4, V8 and ARG (clo_hip_op_device.h); the table keeps a name of its own here because the
// kernels' symbols spell it
template <int MODE> struct topk_val : clo_op_val<MODE> {};

// What PICK hands on: the digits found so far (right-aligned) and the remaining 0-based rank among the keys that
// share them. state[p] is read by digit sweep p and by PICK p; state[passes] = (T, r) by COUNT and APPLY.
struct topk_state { unsigned long long prefix; unsigned rank, pad; };

// ---- the workspace (every part a multiple of CLO_HIP_WORKSPACE_ALIGN) ----
constexpr size_t TOPK_WS_TABLES = 8 * TOPK_DIGITS * sizeof(unsigned);     // one table per digit of the widest key
constexpr size_t TOPK_WS_STATES = 256;                                    // 9 states of 16 bytes
constexpr size_t TOPK_WS_SORTKEYS = (size_t) TOPK_SORTED_MAX * 8;         // the compacted keys of a "sorted" call without keys_out
constexpr size_t TOPK_WS_COUNTS = TOPK_WS_TABLES + TOPK_WS_STATES + TOPK_WS_SORTKEYS;
static_assert(sizeof(topk_state) == 16 && 9 * sizeof(topk_state) <= TOPK_WS_STATES, "the states fit");

// x of a key: the order-key function of merge, search and select, complemented for "largest"
template <typename TK, int KIND>
__device__ __forceinline__ TK topk_order(TK key, TK flip) {
	if constexpr (KIND == 2) {
		// clo_keyx_fwd's kind 2 without its comparison (a scalar register pair per element in the unrolled tiles): a
		// negative key has every bit flipped, any other the sign bit
		constexpr TK SIGN = (TK) ((TK) 1 << (8 * sizeof(TK) - 1));
		typedef typename std::make_signed<TK>::type TS;
		return (TK) (key ^ (TK) ((TK) ((TS) key >> (8 * sizeof(TK) - 1)) | SIGN) ^ flip);
	} else {
		const clo_keyx kx = { 1ull << (8 * sizeof(TK) - 1), sizeof(TK) == 8 ? ~0ull : ((1ull << (8 * (sizeof(TK) & 7))) - 1ull), KIND };
		return (TK) (clo_keyx_fwd<TK>(key, kx) ^ flip);
	}
}

// ---- 1. digit sweep ----
// shift: the digit's position in x. first: the most significant digit, every key counts and state is not read.
template <typename TK, int KIND>
__global__ __launch_bounds__(TOPK_THREADS)
void clo_topk_digit_kernel(const TK* __restrict__ keys, size_t n, unsigned tiles, TK flip, int shift, int first, int kvec,
	const topk_state* __restrict__ state, unsigned* __restrict__ table) {
	constexpr int ROWS = topk_rows((int) sizeof(TK), 0);
	constexpr size_t TILE = (size_t) ROWS * TOPK_ROW_ELEMS;
	__shared__ unsigned s_cnt[TOPK_DIGITS << TOPK_COPIES_LOG2];
	const unsigned tid = threadIdx.x, copy = tid & ((1u << TOPK_COPIES_LOG2) - 1u);
	const unsigned long long prefix = first ? 0ull : state->prefix;
	const int above = first ? 0 : shift + TOPK_DIGIT_BITS;   // (below the key's width when not first)
	for (unsigned i = tid; i < (unsigned) (TOPK_DIGITS << TOPK_COPIES_LOG2); i += TOPK_THREADS) s_cnt[i] = 0u;
	__syncthreads();
	for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (the same for the whole group)
		const size_t base = (size_t) tile * TILE + (size_t) tid * TOPK_VEC;
		TK k[ROWS][TOPK_VEC];
		#pragma unroll
		for (int r = 0; r < ROWS; ++r) clo_op_load4<TK>(keys, base + (size_t) r * TOPK_ROW_ELEMS, n, kvec != 0, k[r]);
		#pragma unroll
		for (int r = 0; r < ROWS; ++r) {
			#pragma unroll
			for (int c = 0; c < TOPK_VEC; ++c) {
				const unsigned long long x = (unsigned long long) topk_order<TK, KIND>(k[r][c], flip);
				const bool valid = base + (size_t) r * TOPK_ROW_ELEMS + c < n && (first || (x >> above) == prefix);
				const unsigned d = (unsigned) (x >> shift) & (unsigned) (TOPK_DIGITS - 1);
				if (valid) atomicAdd(&s_cnt[(d << TOPK_COPIES_LOG2) + copy], 1u);
			}
		}
	}
	// the flush: a digit's copies summed (rotated by the digit), what is not zero added onto the table
	__syncthreads();
	constexpr unsigned CM = (1u << TOPK_COPIES_LOG2) - 1u;
	unsigned h = 0;
	for (unsigned c = 0; c <= CM; ++c) h += s_cnt[(tid << TOPK_COPIES_LOG2) + ((c + tid) & CM)];
	if (h != 0u) (void) __hip_atomic_fetch_add(table + tid, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 2. pick: the digit d with (count of digits below d) <= rank < (that + count of d); out = (prefix << 8 | d, rank -
// count below). The counts come from the sweep over the same keys, so one digit holds the rank; if none does (the keys
// were rewritten under the call) digit 255 and rank 0 are handed on: every later step stays in bounds for any (T, r).
// last: out is (T, r), and *kth_out = T mapped back to the key's bits. ----
__global__ __launch_bounds__(TOPK_THREADS)
void clo_topk_pick_kernel(const unsigned* __restrict__ table, const topk_state* __restrict__ in, topk_state* __restrict__ out,
	unsigned rank0, int first, int last, int key_size, int key_kind, unsigned long long flip, void* __restrict__ kth_out) {
	__shared__ unsigned s_wave[TOPK_WAVES];
	__shared__ unsigned s_pick[2];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned long long prefix = first ? 0ull : in->prefix;
	const unsigned rank = first ? rank0 : in->rank;
	const unsigned c = table[tid];
	const unsigned incl = clo_wave_scan_inclusive<unsigned>(c, lane);
	if (lane == 63u) s_wave[wave] = incl;
	if (tid == 0) { s_pick[0] = (unsigned) (TOPK_DIGITS - 1); s_pick[1] = 0u; }
	__syncthreads();
	unsigned below = incl - c;   // the sum of all counts is at most numel < 2^32
	#pragma unroll
	for (unsigned w = 0; w < (unsigned) TOPK_WAVES; ++w) if (w < wave) below += s_wave[w];
	if (below <= rank && rank - below < c) { s_pick[0] = tid; s_pick[1] = rank - below; }
	__syncthreads();
	if (tid == 0) {
		const unsigned long long x = (prefix << TOPK_DIGIT_BITS) | s_pick[0];
		out->prefix = x;
		out->rank = s_pick[1];
		out->pad = 0u;
		if (last && kth_out) {
			const clo_keyx kx = { 1ull << (8 * key_size - 1), key_size == 8 ? ~0ull : ((1ull << (8 * (key_size & 7))) - 1ull), key_kind };
			const unsigned long long key = clo_keyx_inv<unsigned long long>((x ^ flip) & kx.field, kx);
			if (key_size == 1) *static_cast<uint8_t*>(kth_out) = (uint8_t) key;
			else if (key_size == 2) *static_cast<uint16_t*>(kth_out) = (uint16_t) key;
			else if (key_size == 4) *static_cast<uint32_t*>(kth_out) = (uint32_t) key;
			else *static_cast<unsigned long long*>(kth_out) = key;
		}
	}
}

// ---- 3. count sweep: lt[tile] = how many x < T, eq[tile] = how many x == T ----
template <typename TK, int KIND>
__global__ __launch_bounds__(TOPK_THREADS)
void clo_topk_count_kernel(const TK* __restrict__ keys, size_t n, int rows, TK flip, int kvec, const topk_state* __restrict__ state,
	unsigned* __restrict__ lt, unsigned* __restrict__ eq) {
	__shared__ unsigned s_wave[2][TOPK_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const TK t = (TK) state->prefix;
	const size_t base = (size_t) blockIdx.x * (size_t) rows * TOPK_ROW_ELEMS + (size_t) tid * TOPK_VEC;
	unsigned nlt = 0, neq = 0;
	for (int r0 = 0; r0 < rows; r0 += 4) {   // rows is 4 or 8
		TK k[4][TOPK_VEC];
		#pragma unroll
		for (int r = 0; r < 4; ++r) clo_op_load4<TK>(keys, base + (size_t) (r0 + r) * TOPK_ROW_ELEMS, n, kvec != 0, k[r]);
		#pragma unroll
		for (int r = 0; r < 4; ++r) {
			#pragma unroll
			for (int c = 0; c < TOPK_VEC; ++c) {
				const TK x = topk_order<TK, KIND>(k[r][c], flip);
				const bool in = base + (size_t) (r0 + r) * TOPK_ROW_ELEMS + c < n;
				nlt += in && x < t ? 1u : 0u;
				neq += in && x == t ? 1u : 0u;
			}
		}
	}
	nlt = clo_wave_reduce_sum<unsigned>(nlt);
	neq = clo_wave_reduce_sum<unsigned>(neq);
	if (lane == 0) { s_wave[0][wave] = nlt; s_wave[1][wave] = neq; }
	__syncthreads();
	if (tid == 0) {
		unsigned a = 0, b = 0;
		#pragma unroll
		for (int w = 0; w < TOPK_WAVES; ++w) { a += s_wave[0][w]; b += s_wave[1][w]; }
		lt[blockIdx.x] = a;   // a + b <= the tile's element count
		eq[blockIdx.x] = b;
	}
}

// ---- 4. count scan: blockIdx.x 0 scans lt, 1 scans eq: count[0, tiles) -> exclusive sums in place, count[tiles] = the
// sum of all. One work-group each; the plain form of select's scan, which requests its counts a trip ahead. ----
__global__ __launch_bounds__(TOPK_THREADS)
void clo_topk_scan_kernel(unsigned* __restrict__ lt, unsigned* __restrict__ eq, unsigned tiles) {
	constexpr unsigned TRIP = TOPK_THREADS * TOPK_SCAN_ITEMS;
	__shared__ unsigned s_wave[TOPK_WAVES];
	unsigned* const count = blockIdx.x == 0 ? lt : eq;
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	unsigned carry = 0;   // the sum of all counts is at most numel < 2^32
	unsigned v[TOPK_SCAN_ITEMS];
	for (unsigned base = 0; base < tiles; base += TRIP) {
		unsigned sum = 0;
		#pragma unroll
		for (unsigned c = 0; c < TOPK_SCAN_ITEMS; ++c) {
			const unsigned long long i = (unsigned long long) base + tid * TOPK_SCAN_ITEMS + c;
			v[c] = i < tiles ? count[i] : 0u;
			sum += v[c];
		}
		const unsigned incl = clo_wave_scan_inclusive<unsigned>(sum, lane);
		if (lane == 63u) s_wave[wave] = incl;
		__syncthreads();
		unsigned before = 0, total = 0;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) TOPK_WAVES; ++w) {
			const unsigned s = s_wave[w];
			if (w < wave) before += s;
			total += s;
		}
		unsigned at = carry + before + incl - sum;
		#pragma unroll
		for (unsigned c = 0; c < TOPK_SCAN_ITEMS; ++c) {
			const unsigned long long i = (unsigned long long) base + tid * TOPK_SCAN_ITEMS + c;
			if (i < tiles) count[i] = at;
			at += v[c];
		}
		carry += total;
		__syncthreads();   // s_wave is written again
	}
	if (tid == 0) count[tiles] = carry;
}

// One scan of the tile in input order (row, wave, lane, element): at[r] becomes the number of set bits of the tile before
// this lane's four elements of row r; returns the tile's total. s_piece: ROWS * TOPK_WAVES words.
template <int ROWS>
__device__ __forceinline__ unsigned topk_tile_scan(const unsigned (&bits)[ROWS], unsigned (&at)[ROWS], unsigned* s_piece, unsigned lane, unsigned wave) {
	constexpr int PIECES = ROWS * TOPK_WAVES;
	static_assert(PIECES <= 64, "one piece per lane");
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const unsigned c = (unsigned) __popc(bits[r]);
		const unsigned incl = clo_wave_scan_inclusive<unsigned>(c, lane);
		at[r] = incl - c;
		if (lane == 63u) s_piece[r * TOPK_WAVES + wave] = incl;
	}
	__syncthreads();
	const unsigned piece = lane < (unsigned) PIECES ? s_piece[lane] : 0u;
	const unsigned piece_incl = clo_wave_scan_inclusive<unsigned>(piece, lane);
	const unsigned total = (unsigned) __builtin_amdgcn_readlane((int) piece_incl, 63);
	// (through the permute network, not readlane: 2 x ROWS scalars more than the comparison forms have to spare)
	const int piece_excl = (int) (piece_incl - piece);
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) at[r] += (unsigned) __shfl(piece_excl, r * TOPK_WAVES + (int) wave, 64);
	__syncthreads();   // s_piece may be written again
	return total;
}

// ---- 5. apply sweep ----
template <typename TK, int KIND, int MODE>
__global__ __launch_bounds__(TOPK_THREADS)
void clo_topk_apply_kernel(const TK* __restrict__ keys, const typename topk_val<MODE>::T* __restrict__ values,
	TK* __restrict__ kout, typename topk_val<MODE>::T* __restrict__ vout, size_t n, unsigned m, TK flip, int kvec, int vvec,
	const topk_state* __restrict__ state, const unsigned* __restrict__ lt, const unsigned* __restrict__ eq) {
	typedef typename topk_val<MODE>::T TV;
	constexpr int ROWS = topk_rows((int) sizeof(TK), topk_val<MODE>::size);
	constexpr unsigned TILE = (unsigned) ROWS * TOPK_ROW_ELEMS;
	constexpr bool VALS = MODE == CLO_OP_V4 || MODE == CLO_OP_V8;
	constexpr size_t ELEM = MODE != CLO_OP_KEYS && sizeof(TV) > sizeof(TK) ? sizeof(TV) : sizeof(TK);
	__shared__ __attribute__((aligned(16))) unsigned char s_buf[TILE * ELEM];
	__shared__ unsigned s_piece[ROWS * TOPK_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = (unsigned) __builtin_amdgcn_readfirstlane((int) (tid >> 6));
	const size_t tile_start = (size_t) blockIdx.x * TILE, base = tile_start + (size_t) tid * TOPK_VEC;
	const bool want_keys = kout != nullptr;
	const TK t = (TK) state->prefix;
	// how many of the equal elements are taken: r + 1 (64 bits: r may be 2^32 - 1 on garbage)
	const unsigned long long take = (unsigned long long) state->rank + 1ull;
	const unsigned long long eq_at = eq[blockIdx.x], lt_at = lt[blockIdx.x];

	TK k[ROWS][TOPK_VEC];
	TV v[VALS ? ROWS : 1][TOPK_VEC];
	unsigned bits[ROWS], eqb[ROWS], at[ROWS];
	unsigned any_eq = 0;
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const size_t i0 = base + (size_t) r * TOPK_ROW_ELEMS;
		clo_op_load4<TK>(keys, i0, n, kvec != 0, k[r]);
		if constexpr (VALS) clo_op_load4<TV>(values, i0, n, vvec != 0, v[r]);
		bits[r] = 0u; eqb[r] = 0u;
		#pragma unroll
		for (int c = 0; c < TOPK_VEC; ++c) {
			const TK x = topk_order<TK, KIND>(k[r][c], flip);
			bits[r] |= (x < t ? 1u : 0u) << c;
			eqb[r] |= (x == t ? 1u : 0u) << c;
		}
		// the elements that exist: one mask per row, not a comparison per element
		const unsigned in = i0 >= n ? 0u : n - i0 >= (size_t) TOPK_VEC ? 15u : (1u << (unsigned) (n - i0)) - 1u;
		bits[r] &= in; eqb[r] &= in;
		any_eq |= eqb[r];
	}
	// The equal elements: the tile's first (take - eq_at) of them are kept. All of them where the cut lies behind the
	// tile, none where it lies before it; only the tile that holds the cut ranks them (the same for the whole group).
	if (eq_at < take) {
		const unsigned long long room = take - eq_at;   // >= 1
		const unsigned eq_tile = (unsigned) __syncthreads_count(any_eq != 0u) ? 1u : 0u;
		if (eq_tile != 0u) {
			if (room >= (unsigned long long) TILE) {
				#pragma unroll
				for (int r = 0; r < ROWS; ++r) bits[r] |= eqb[r];
			} else {
				(void) topk_tile_scan<ROWS>(eqb, at, s_piece, lane, wave);
				#pragma unroll
				for (int r = 0; r < ROWS; ++r) {
					#pragma unroll
					for (int c = 0; c < TOPK_VEC; ++c) {
						const unsigned rank = at[r] + (unsigned) __popc(eqb[r] & ((1u << c) - 1u));
						if ((eqb[r] >> c & 1u) && rank < (unsigned) room) bits[r] |= 1u << c;
					}
				}
			}
		}
	}
	const unsigned kept = topk_tile_scan<ROWS>(bits, at, s_piece, lane, wave);   // <= the tile's element count

	// rows [keep_at, keep_at + keep_rows) of [0, m)
	const unsigned long long mm = m;
	unsigned long long keep_at = lt_at + (eq_at < take ? eq_at : take);
	if (keep_at > mm) keep_at = mm;
	const unsigned keep_rows = (unsigned) (mm - keep_at < kept ? mm - keep_at : kept);

	auto compact = [&](auto* s, auto* out, auto value) {
		#pragma unroll
		for (int r = 0; r < ROWS; ++r) {
			#pragma unroll
			for (int c = 0; c < TOPK_VEC; ++c) {
				const unsigned idx = (unsigned) r * TOPK_ROW_ELEMS + tid * TOPK_VEC + (unsigned) c;
				const unsigned rank = at[r] + (unsigned) __popc(bits[r] & ((1u << c) - 1u));   // < kept <= TILE
				if (bits[r] >> c & 1u) s[rank] = value(r, c, idx);
			}
		}
		__syncthreads();
		clo_op_store(out + (size_t) keep_at, keep_rows, tid, [&](unsigned j) { return s[j]; });
	};
	if (want_keys) {
		compact(reinterpret_cast<TK*>(s_buf), kout, [&](int r, int c, unsigned) { return k[r][c]; });
		if constexpr (MODE != CLO_OP_KEYS) __syncthreads();   // the values take the keys' place
	}
	if constexpr (VALS) compact(reinterpret_cast<TV*>(s_buf), vout, [&](int r, int c, unsigned) { return v[r][c]; });
	if constexpr (MODE == CLO_OP_ARG) compact(reinterpret_cast<TV*>(s_buf), vout, [&](int, int, unsigned idx) { return (TV) (tile_start + idx); });
}

// ---- 6. "sorted": rows [0, m), m <= TOPK_SORTED_MAX, sorted by (x, row) in LDS by one work-group, in place. ksrc: the
// compacted keys (kout itself, or the workspace copy where kout is NULL). Keys are equal iff their bits are, so the
// sorted keys are written from the sorted x; a lane gathers the values of its rows before anything is stored. ----
template <typename TK, int VS>
__global__ __launch_bounds__(TOPK_SORT_THREADS)
void clo_topk_sort_kernel(const TK* ksrc, TK* kout, void* vout_, unsigned m, TK flip, int key_kind) {
	typedef typename topk_val<VS == 8 ? CLO_OP_V8 : CLO_OP_V4>::T TV;
	constexpr unsigned PER = TOPK_SORTED_MAX / TOPK_SORT_THREADS;
	__shared__ TK s_x[TOPK_SORTED_MAX];
	__shared__ unsigned s_row[TOPK_SORTED_MAX];
	TV* const vout = static_cast<TV*>(vout_);
	const unsigned tid = threadIdx.x;
	const clo_keyx kx = { 1ull << (8 * sizeof(TK) - 1), sizeof(TK) == 8 ? ~0ull : ((1ull << (8 * (sizeof(TK) & 7))) - 1ull), key_kind };
	if (m > TOPK_SORTED_MAX) m = TOPK_SORTED_MAX;
	unsigned p2 = 1;
	while (p2 < m) p2 <<= 1;   // <= TOPK_SORTED_MAX, a power of two
	// the padding sorts behind every row: all ones and a row number >= m
	for (unsigned i = tid; i < p2; i += TOPK_SORT_THREADS) {
		s_x[i] = i < m ? (TK) (clo_keyx_fwd<TK>(ksrc[i], kx) ^ flip) : (TK) ~(TK) 0;
		s_row[i] = i;
	}
	__syncthreads();
	for (unsigned size = 2; size <= p2; size <<= 1) {
		for (unsigned j = size >> 1; j > 0; j >>= 1) {
			for (unsigned q = tid; q < (p2 >> 1); q += TOPK_SORT_THREADS) {
				const unsigned a = ((q & ~(j - 1u)) << 1) | (q & (j - 1u)), b = a | j;
				const bool up = (a & size) == 0u;
				const TK xa = s_x[a], xb = s_x[b];
				const unsigned ra = s_row[a], rb = s_row[b];
				const bool a_after_b = xa > xb || (xa == xb && ra > rb);
				if (a_after_b == up) { s_x[a] = xb; s_x[b] = xa; s_row[a] = rb; s_row[b] = ra; }
			}
			__syncthreads();
		}
	}
	if constexpr (VS != 0) {
		TV v[PER];
		#pragma unroll
		for (unsigned c = 0; c < PER; ++c) {
			const unsigned j = tid + c * TOPK_SORT_THREADS;
			v[c] = j < m ? vout[clo_op_min(s_row[j], m - 1u)] : (TV) 0;
		}
		__syncthreads();   // every gather has returned before a row is overwritten
		#pragma unroll
		for (unsigned c = 0; c < PER; ++c) {
			const unsigned j = tid + c * TOPK_SORT_THREADS;
			if (j < m) vout[j] = v[c];
		}
	}
	if (kout) {
		for (unsigned j = tid; j < m; j += TOPK_SORT_THREADS) kout[j] = clo_keyx_inv<TK>((TK) (s_x[j] ^ flip), kx);
	}
}

struct topk_args {
	const void* keys; const void* values; void* kout; void* vout; void* kth;
	size_t n; unsigned m; int desc, sorted, kind; unsigned char* ws; hipStream_t s;
};

inline int topk_cus() {   // of the current device, as the stream is taken to be
	int dev = 0, c = 0;
	if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) return 256;
	return c;
}

// the groups a digit sweep launches where the tile count does not limit it
inline size_t topk_sweep_groups() { return (size_t) topk_cus() * TOPK_GROUPS_PER_CU; }

#define TOPK_CHECK_LAUNCH() do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int) e_; } while (0)

template <typename TK, int KIND>
int topk_find(const topk_args& a, TK flip) {
	constexpr int PASSES = (int) sizeof(TK);
	constexpr size_t TILE = topk_tile((int) sizeof(TK), 0);
	unsigned* const tables = reinterpret_cast<unsigned*>(a.ws);
	topk_state* const state = reinterpret_cast<topk_state*>(a.ws + TOPK_WS_TABLES);
	const unsigned tiles = (unsigned) ((a.n + TILE - 1) / TILE);
	size_t groups = topk_sweep_groups();
	if (groups > tiles) groups = tiles;
	const int kvec = clo_op_vec_ok<TK>(a.keys);
	const hipError_t e = hipMemsetAsync(tables, 0, (size_t) PASSES * TOPK_DIGITS * sizeof(unsigned), a.s);
	if (e != hipSuccess) return (int) e;
	for (int p = 0; p < PASSES; ++p) {
		const int shift = 8 * (PASSES - 1 - p);
		{
			clo_timing_scope timing("topk_digit", a.s);
			hipLaunchKernelGGL((clo_topk_digit_kernel<TK, KIND>), dim3((unsigned) groups), dim3(TOPK_THREADS), 0, a.s,
				(const TK*) a.keys, a.n, tiles, flip, shift, p == 0, kvec, (const topk_state*) (state + p), tables + p * TOPK_DIGITS);
			TOPK_CHECK_LAUNCH();
		}
		clo_timing_scope timing("topk_pick", a.s);
		hipLaunchKernelGGL(clo_topk_pick_kernel, dim3(1), dim3(TOPK_THREADS), 0, a.s, (const unsigned*) (tables + p * TOPK_DIGITS),
			(const topk_state*) (state + p), state + p + 1, a.m - 1u, p == 0, p == PASSES - 1, (int) sizeof(TK), a.kind,
			(unsigned long long) flip, a.kth);
		TOPK_CHECK_LAUNCH();
	}
	return 0;
}

template <typename TK, int VS>
int topk_sort_launch(const topk_args& a, const TK* ksrc, TK flip) {
	clo_timing_scope timing("topk_sort", a.s);
	hipLaunchKernelGGL((clo_topk_sort_kernel<TK, VS>), dim3(1), dim3(TOPK_SORT_THREADS), 0, a.s, ksrc, (TK*) a.kout, a.vout, a.m, flip, a.kind);
	return (int) hipGetLastError();
}

template <typename TK, int KIND, int MODE>
int topk_launch(const topk_args& a) {
	typedef typename topk_val<MODE>::T TV;
	constexpr int PASSES = (int) sizeof(TK);
	constexpr int ROWS = topk_rows((int) sizeof(TK), topk_val<MODE>::size);
	constexpr size_t TILE = (size_t) ROWS * TOPK_ROW_ELEMS;
	const TK flip = a.desc ? (TK) ~(TK) 0 : (TK) 0;
	const int st = topk_find<TK, KIND>(a, flip);
	if (st != 0 || (!a.kout && !a.vout)) return st;   // kth_out alone: the digit passes are all there is

	const topk_state* const found = reinterpret_cast<const topk_state*>(a.ws + TOPK_WS_TABLES) + PASSES;
	const unsigned tiles = (unsigned) ((a.n + TILE - 1) / TILE);
	unsigned* const lt = reinterpret_cast<unsigned*>(a.ws + TOPK_WS_COUNTS);
	unsigned* const eq = lt + (tiles + 1u);
	const int kvec = clo_op_vec_ok<TK>(a.keys), vvec = clo_op_vec_ok<TV>(a.values);
	// a "sorted" call without keys_out: the sort reads the compacted keys from the workspace
	TK* const kdst = a.kout ? (TK*) a.kout : a.sorted ? reinterpret_cast<TK*>(a.ws + TOPK_WS_TABLES + TOPK_WS_STATES) : nullptr;
	{
		clo_timing_scope timing("topk_count", a.s);
		hipLaunchKernelGGL((clo_topk_count_kernel<TK, KIND>), dim3(tiles), dim3(TOPK_THREADS), 0, a.s,
			(const TK*) a.keys, a.n, ROWS, flip, kvec, found, lt, eq);
		TOPK_CHECK_LAUNCH();
	}
	{
		clo_timing_scope timing("topk_scan", a.s);
		hipLaunchKernelGGL(clo_topk_scan_kernel, dim3(2), dim3(TOPK_THREADS), 0, a.s, lt, eq, tiles);
		TOPK_CHECK_LAUNCH();
	}
	{
		clo_timing_scope timing("topk_apply", a.s);
		hipLaunchKernelGGL((clo_topk_apply_kernel<TK, KIND, MODE>), dim3(tiles), dim3(TOPK_THREADS), 0, a.s,
			(const TK*) a.keys, (const TV*) a.values, kdst, (TV*) a.vout, a.n, a.m, flip, kvec, vvec, found,
			(const unsigned*) lt, (const unsigned*) eq);
		TOPK_CHECK_LAUNCH();
	}
	if (!a.sorted) return 0;
	return topk_sort_launch<TK, topk_val<MODE>::size>(a, kdst, flip);
}

template <typename TK, int KIND>
int topk_dispatch_mode(const topk_args& a, int mode) {
	switch (mode) {
		case CLO_OP_KEYS: return topk_launch<TK, KIND, CLO_OP_KEYS>(a);
		case CLO_OP_V4: return topk_launch<TK, KIND, CLO_OP_V4>(a);
		case CLO_OP_V8: return topk_launch<TK, KIND, CLO_OP_V8>(a);
		default: return topk_launch<TK, KIND, CLO_OP_ARG>(a);
	}
}

template <typename TK>
int topk_dispatch(const topk_args& a, int mode) {
	if (a.kind == 1) return topk_dispatch_mode<TK, 1>(a, mode);
	if constexpr (sizeof(TK) > 1) {
		if (a.kind == 2) return topk_dispatch_mode<TK, 2>(a, mode);
	}
	return topk_dispatch_mode<TK, 0>(a, mode);
}

}  // namespace

extern "C" {

size_t clo_hip_topk_tile(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return topk_tile(key_size, value_size);
}

size_t clo_hip_topk_sweep_groups(void) { return topk_sweep_groups(); }

size_t clo_hip_topk_sorted_max(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return TOPK_SORTED_MAX;
}

size_t clo_hip_topk_workspace_bytes(size_t numel, int key_size, int value_size) {
	const size_t tile = clo_hip_topk_tile(key_size, value_size);
	if (numel == 0 || tile == 0) return 0;
	// the digit tables, the states, the sort's keys; then two counts per tile and the two totals, 4 bytes each
	return TOPK_WS_COUNTS + clo_op_ws_align(((numel - 1) / tile + 2) * 2 * sizeof(unsigned));
}

int clo_hip_topk(int which, int order, const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* kth_out,
	size_t numel, size_t k, int key_size, int key_kind, int value_size, void* workspace, size_t workspace_bytes, void* stream) {
	if (which != CLO_HIP_TOPK_SMALLEST && which != CLO_HIP_TOPK_LARGEST) return CLO_HIP_EARGS;
	if (order != CLO_HIP_TOPK_INPUT && order != CLO_HIP_TOPK_SORTED) return CLO_HIP_EARGS;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!keys_out && !values_out && !kth_out) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	const bool arg = value_size > 0 && !values_in;
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	if (numel > 0 && !keys_in) return CLO_HIP_EARGS;
	if (clo_misaligned(keys_in, (size_t) key_size) || clo_misaligned(keys_out, (size_t) key_size) || clo_misaligned(kth_out, (size_t) key_size)) return CLO_HIP_EARGS;
	if (value_size > 0 && (clo_misaligned(values_in, (size_t) value_size) || clo_misaligned(values_out, (size_t) value_size))) return CLO_HIP_EARGS;
	const size_t m = k < numel ? k : numel;
	if (order == CLO_HIP_TOPK_SORTED && m > TOPK_SORTED_MAX) return CLO_HIP_EARGS;
	if (m == 0) return 0;   // nothing is chosen, nothing is written, nothing is enqueued
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_topk_workspace_bytes(numel, key_size, value_size)) return CLO_HIP_EWORKSPACE;

	topk_args a;
	a.keys = keys_in; a.values = values_in; a.kout = keys_out; a.vout = values_out; a.kth = kth_out;
	a.n = numel; a.m = (unsigned) m; a.desc = which == CLO_HIP_TOPK_LARGEST; a.sorted = order == CLO_HIP_TOPK_SORTED; a.kind = key_kind;
	a.ws = (unsigned char*) workspace; a.s = (hipStream_t) stream;
	const int mode = clo_op_mode(value_size, arg);
	return clo_op_by_key_size(key_size, [&](auto tk) { return topk_dispatch<decltype(tk)>(a, mode); });
}

}  // extern "C"
