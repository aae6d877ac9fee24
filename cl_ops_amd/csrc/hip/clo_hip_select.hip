// clo_hip_select.hip — stable selection and partition by flags or by comparison with a threshold (CloSelect,
// include/clo_select.h; not upstream), with values carried along or the indices written.
//
// Element i is KEPT iff flags[i] != 0 ("flagged"), or iff keys[i] <pred> threshold in the by-key sort's order. select
// writes the kept elements in input order to rows [0, k); partition writes the rejected ones behind them, to rows [k,
// numel), in input order too. k goes to num_out.
//
// Three launches, none of which waits for another work-group, none of which uses an atomic (§10's form):
//   COUNT  one work-group per tile loads what the decision needs — the flag bytes alone, or the keys and the threshold —
//          decides keep for every element and writes the tile's kept count -> count[tiles];
//   SCAN   one work-group turns the counts into exclusive offsets in place, leaves the total k in count[tiles] and
//          writes num_out = min(k, numel);
//   APPLY  the same loads and the same decision function (sel_decide), plus keys and values; the kept rows are
//          compacted in LDS in input order (the rejected ones behind them for a partition) and stored at the tile's
//          offset, the rejected ones at k + (tile start - offset), every store index below numel.
// A tile is 256 threads x 4 consecutive elements x ROWS rows (§10's shape): a lane's four elements come in one vector
// load where the array's start allows it, a row is one coalesced stretch of 1024 elements. Inside a tile the order is
// row, wave, lane, element, which is the input order: a wave scans its 64 lane counts of a row (clo_wave_scan_inclusive),
// the ROWS x 4 wave totals are the pieces every wave scans again for itself after the tile's one barrier.
// Whatever the arrays hold: both sweeps read the same bytes and so agree; the loads are bounded by numel, the LDS slots
// by the tile's element count, and APPLY clamps every global row range to [0, numel).
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_VEC = 4;
constexpr int SEL_ROW_ELEMS = SEL_THREADS * SEL_VEC;   // 1024
static_assert(SEL_THREADS == CLO_OP_THREADS && SEL_VEC == CLO_OP_VEC, "the shared helpers' work-group and vector");
constexpr int SEL_CHUNK_ROWS = 4;                      // the count sweep takes the rows of a tile four at a time
constexpr unsigned SEL_SCAN_ITEMS = 8;                 // the scan sweeps SEL_THREADS * SEL_SCAN_ITEMS counts per trip
static_assert(SEL_THREADS * SEL_SCAN_ITEMS == CLO_HIP_SELECT_SCAN_TRIP, "the header names the scan's trip");

// rows per tile: the compacted rows of a tile lie in LDS, keys first and values after them in the same 32 KiB
constexpr int sel_rows(int key_size, int value_size) { return (key_size > value_size ? key_size : value_size) <= 4 ? 8 : 4; }
constexpr size_t sel_tile(int key_size, int value_size) { return (size_t) sel_rows(key_size, value_size) * SEL_ROW_ELEMS; }

// the modes CLO_OP_KEYS, V4, V8 and ARG (clo_hip_op_device.h); the table keeps a name of its own here because the
// kernels' symbols spell it
template <int MODE> struct sel_val : clo_op_val<MODE> {};

// The order-key function of merge and search (clo_keyx_fwd), its kind known when the kernel is compiled.
template <typename TK, int KIND>
__device__ __forceinline__ TK sel_order(TK x) {
	const clo_keyx kx = { 1ull << (8 * sizeof(TK) - 1), sizeof(TK) == 8 ? ~0ull : ((1ull << (8 * (sizeof(TK) & 7))) - 1ull), KIND };
	return clo_keyx_fwd<TK>(x, kx);
}

// What the decision needs: the flags (pred flagged) or the keys and the threshold in unsigned order (a comparison).
template <typename TK>
struct sel_pred {
	const TK* keys; const unsigned char* flags; size_t n; TK thr; int pred; bool kvec, fvec;
};

template <typename TK, int KIND>
__device__ __forceinline__ sel_pred<TK> sel_pred_make(const TK* __restrict__ keys, const void* __restrict__ fot, size_t n, int pred, int kvec, int fvec) {
	sel_pred<TK> q;
	q.keys = keys; q.n = n; q.pred = pred; q.kvec = kvec != 0; q.fvec = fvec != 0;
	q.flags = static_cast<const unsigned char*>(fot);
	q.thr = pred == CLO_HIP_SELECT_FLAGGED ? (TK) 0 : sel_order<TK, KIND>(*static_cast<const TK*>(fot));
	return q;
}

// THE decision, inlined into both sweeps: the keep bits of the four elements from i0 (bit c: element i0 + c exists and
// is kept). A comparison loads the keys and leaves them, with their original bits, in k; FLAGGED loads the four flag
// bytes alone and does not touch k. No branch but those of the loads: the rows of a tile are requested together.
template <typename TK, int KIND, bool FLAGGED>
__device__ __forceinline__ unsigned sel_decide(const sel_pred<TK>& q, size_t i0, TK (&k)[SEL_VEC]) {
	unsigned bits = 0;
	if constexpr (FLAGGED) {
		unsigned char f[SEL_VEC];
		clo_op_load4<unsigned char>(q.flags, i0, q.n, q.fvec, f);
		#pragma unroll
		for (int c = 0; c < SEL_VEC; ++c) bits |= (f[c] != 0 ? 1u : 0u) << c;   // past the end: read as 0
	} else {
		clo_op_load4<TK>(q.keys, i0, q.n, q.kvec, k);
		// which of below / equal / above the threshold the predicate keeps (wave-uniform)
		const bool below = q.pred == CLO_HIP_SELECT_LT || q.pred == CLO_HIP_SELECT_LE || q.pred == CLO_HIP_SELECT_NE;
		const bool equal = q.pred == CLO_HIP_SELECT_LE || q.pred == CLO_HIP_SELECT_GE || q.pred == CLO_HIP_SELECT_EQ;
		const bool above = q.pred == CLO_HIP_SELECT_GT || q.pred == CLO_HIP_SELECT_GE || q.pred == CLO_HIP_SELECT_NE;
		const TK t = q.thr;
		#pragma unroll
		for (int c = 0; c < SEL_VEC; ++c) {
			const TK x = sel_order<TK, KIND>(k[c]);
			const bool keep = (x < t ? below : x == t ? equal : above) && i0 + c < q.n;
			bits |= (keep ? 1u : 0u) << c;
		}
	}
	return bits;
}

// ---- 1. count sweep ----
template <typename TK, int KIND, bool FLAGGED>
__device__ __forceinline__ unsigned sel_count_tile(const sel_pred<TK>& q, size_t base, int chunks) {
	unsigned kept = 0;
	for (int ch = 0; ch < chunks; ++ch) {
		#pragma unroll
		for (int r = 0; r < SEL_CHUNK_ROWS; ++r) {
			TK k[SEL_VEC];
			kept += (unsigned) __popc(sel_decide<TK, KIND, FLAGGED>(q, base + (size_t) (ch * SEL_CHUNK_ROWS + r) * SEL_ROW_ELEMS, k));
		}
	}
	return kept;
}

template <typename TK, int KIND>
__global__ __launch_bounds__(SEL_THREADS)
void clo_select_count_kernel(const TK* __restrict__ keys, const void* __restrict__ fot, size_t n, int pred, int chunks,
	int kvec, int fvec, unsigned* __restrict__ count) {
	__shared__ unsigned s_wave[SEL_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const sel_pred<TK> q = sel_pred_make<TK, KIND>(keys, fot, n, pred, kvec, fvec);
	const size_t base = (size_t) blockIdx.x * (size_t) chunks * (SEL_CHUNK_ROWS * SEL_ROW_ELEMS) + (size_t) tid * SEL_VEC;
	unsigned kept = pred == CLO_HIP_SELECT_FLAGGED ? sel_count_tile<TK, KIND, true>(q, base, chunks) : sel_count_tile<TK, KIND, false>(q, base, chunks);
	kept = clo_wave_reduce_sum<unsigned>(kept);
	if (lane == 0) s_wave[wave] = kept;
	__syncthreads();
	if (tid == 0) {
		unsigned total = 0;
		#pragma unroll
		for (int w = 0; w < SEL_WAVES; ++w) total += s_wave[w];
		count[blockIdx.x] = total;   // <= the tile's element count
	}
}

// ---- 2. count scan: count[0, tiles) -> its exclusive sums in place, count[tiles] = the sum of all, *num_out = min(sum,
// numel). One work-group; the next trip's counts are requested before this trip's are summed. tiles 0: only num_out. ----
__global__ __launch_bounds__(SEL_THREADS)
void clo_select_scan_kernel(unsigned* __restrict__ count, unsigned tiles, unsigned long long numel, unsigned long long* __restrict__ num_out) {
	constexpr unsigned TRIP = SEL_THREADS * SEL_SCAN_ITEMS;
	__shared__ unsigned s_wave[SEL_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	unsigned carry = 0;   // the sum of all counts is at most numel < 2^32
	unsigned v[SEL_SCAN_ITEMS], ahead[SEL_SCAN_ITEMS];
	#pragma unroll
	for (unsigned c = 0; c < SEL_SCAN_ITEMS; ++c) {
		const unsigned i = tid * SEL_SCAN_ITEMS + c;
		ahead[c] = i < tiles ? count[i] : 0u;
	}
	for (unsigned base = 0; base < tiles; base += TRIP) {
		unsigned sum = 0;
		#pragma unroll
		for (unsigned c = 0; c < SEL_SCAN_ITEMS; ++c) {
			v[c] = ahead[c];
			sum += v[c];
			const unsigned long long i = (unsigned long long) base + TRIP + tid * SEL_SCAN_ITEMS + c;
			ahead[c] = i < tiles ? count[i] : 0u;
		}
		const unsigned incl = clo_wave_scan_inclusive<unsigned>(sum, lane);
		if (lane == 63u) s_wave[wave] = incl;
		__syncthreads();
		unsigned before = 0, total = 0;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) SEL_WAVES; ++w) {
			const unsigned s = s_wave[w];
			if (w < wave) before += s;
			total += s;
		}
		unsigned at = carry + before + incl - sum;
		#pragma unroll
		for (unsigned c = 0; c < SEL_SCAN_ITEMS; ++c) {
			const unsigned i = base + tid * SEL_SCAN_ITEMS + c;   // < tiles + TRIP: no wrap, tiles <= 2^22
			if (i < tiles) count[i] = at;
			at += v[c];
		}
		carry += total;
		__syncthreads();   // s_wave is written again
	}
	if (tid == 0) {
		if (tiles > 0) count[tiles] = carry;
		*num_out = carry < numel ? carry : numel;
	}
}

// Where the tile's rows go. The kept rows of tile t start at row offset[t]; the rejected ones of a partition at k + (the
// rejected rows before the tile) = k + (tile start - offset[t]). Both are clamped to [0, numel).
struct sel_place { unsigned keep_at, keep_rows, rej_at, rej_rows; };

// ---- 3. apply sweep ----
template <typename TK, int KIND, int MODE>
__global__ __launch_bounds__(SEL_THREADS)
void clo_select_apply_kernel(const TK* __restrict__ keys, const typename sel_val<MODE>::T* __restrict__ values, const void* __restrict__ fot,
	TK* __restrict__ kout, typename sel_val<MODE>::T* __restrict__ vout, size_t n, int pred, int op, int kvec, int fvec, int vvec,
	const unsigned* __restrict__ offset, unsigned tiles) {
	typedef typename sel_val<MODE>::T TV;
	constexpr int ROWS = sel_rows((int) sizeof(TK), sel_val<MODE>::size);
	constexpr unsigned TILE = (unsigned) ROWS * SEL_ROW_ELEMS;
	constexpr int PIECES = ROWS * SEL_WAVES;
	constexpr bool VALS = MODE == CLO_OP_V4 || MODE == CLO_OP_V8;
	constexpr size_t ELEM = MODE != CLO_OP_KEYS && sizeof(TV) > sizeof(TK) ? sizeof(TV) : sizeof(TK);
	static_assert(PIECES <= 64, "one piece per lane");
	__shared__ __attribute__((aligned(16))) unsigned char s_buf[TILE * ELEM];
	__shared__ unsigned s_piece[PIECES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = (unsigned) __builtin_amdgcn_readfirstlane((int) (tid >> 6));
	const size_t tile_start = (size_t) blockIdx.x * TILE, base = tile_start + (size_t) tid * SEL_VEC;
	const unsigned cnt = n - tile_start < (size_t) TILE ? (unsigned) (n - tile_start) : TILE;   // tile_start < n
	const bool partition = op == CLO_HIP_SELECT_PARTITION;
	const bool want_keys = kout != nullptr;
	const sel_pred<TK> q = sel_pred_make<TK, KIND>(keys, fot, n, pred, kvec, fvec);

	TK k[ROWS][SEL_VEC];
	TV v[VALS ? ROWS : 1][SEL_VEC];
	unsigned bits[ROWS], at[ROWS];
	if (pred == CLO_HIP_SELECT_FLAGGED) {
		const size_t n_keys = want_keys ? n : 0;   // flagged without keys_out: nothing of the keys is read
		#pragma unroll
		for (int r = 0; r < ROWS; ++r) {
			const size_t i0 = base + (size_t) r * SEL_ROW_ELEMS;
			bits[r] = sel_decide<TK, KIND, true>(q, i0, k[r]);
			clo_op_load4<TK>(keys, i0, n_keys, kvec != 0, k[r]);
			if constexpr (VALS) clo_op_load4<TV>(values, i0, n, vvec != 0, v[r]);
		}
	} else {
		#pragma unroll
		for (int r = 0; r < ROWS; ++r) {
			const size_t i0 = base + (size_t) r * SEL_ROW_ELEMS;
			bits[r] = sel_decide<TK, KIND, false>(q, i0, k[r]);
			if constexpr (VALS) clo_op_load4<TV>(values, i0, n, vvec != 0, v[r]);
		}
	}
	// a lane's rank inside its wave's row; the wave totals are the tile's pieces
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const unsigned c = (unsigned) __popc(bits[r]);
		const unsigned incl = clo_wave_scan_inclusive<unsigned>(c, lane);
		at[r] = incl - c;
		if (lane == 63u) s_piece[r * SEL_WAVES + wave] = incl;
	}
	__syncthreads();
	const unsigned piece = lane < (unsigned) PIECES ? s_piece[lane] : 0u;
	const unsigned piece_incl = clo_wave_scan_inclusive<unsigned>(piece, lane);
	const unsigned kept = (unsigned) __builtin_amdgcn_readlane((int) piece_incl, 63);   // <= cnt
	#pragma unroll
	for (int r = 0; r < ROWS; ++r) {
		const int p = r * SEL_WAVES + (int) wave;
		at[r] += (unsigned) __builtin_amdgcn_readlane((int) piece_incl, p) - (unsigned) __builtin_amdgcn_readlane((int) piece, p);
	}

	sel_place pl;
	{
		const unsigned long long numel = n, off = offset[blockIdx.x], k_all = offset[tiles];
		const unsigned long long keep_at = off < numel ? off : numel;
		const unsigned long long before = tile_start >= off ? tile_start - off : 0ull;
		const unsigned long long rej_at = k_all + before < numel ? k_all + before : numel;
		const unsigned rejected = cnt - kept;
		pl.keep_at = (unsigned) keep_at;
		pl.keep_rows = (unsigned) (numel - keep_at < kept ? numel - keep_at : kept);
		pl.rej_at = (unsigned) rej_at;
		pl.rej_rows = partition ? (unsigned) (numel - rej_at < rejected ? numel - rej_at : rejected) : 0u;
	}

	// One array at a time through the tile's LDS: element (r, c) of this lane goes to slot rank (kept) or kept + its
	// index - rank (rejected, partition only); every slot is below cnt <= TILE. Then the two stretches are stored.
	auto compact = [&](auto* s, auto* out, auto value) {
		#pragma unroll
		for (int r = 0; r < ROWS; ++r) {
			#pragma unroll
			for (int c = 0; c < SEL_VEC; ++c) {
				const unsigned idx = (unsigned) r * SEL_ROW_ELEMS + tid * SEL_VEC + (unsigned) c;
				const unsigned rank = at[r] + (unsigned) __popc(bits[r] & ((1u << c) - 1u));
				if (bits[r] >> c & 1u) s[rank] = value(r, c, idx);
				else if (partition && idx < cnt) s[kept + (idx - rank)] = value(r, c, idx);
			}
		}
		__syncthreads();
		clo_op_store(out + pl.keep_at, pl.keep_rows, tid, [&](unsigned j) { return s[j]; });
		if (partition) clo_op_store(out + pl.rej_at, pl.rej_rows, tid, [&](unsigned j) { return s[kept + j]; });
	};
	if (want_keys) {
		compact(reinterpret_cast<TK*>(s_buf), kout, [&](int r, int c, unsigned) { return k[r][c]; });
		if constexpr (MODE != CLO_OP_KEYS) __syncthreads();   // the values take the keys' place
	}
	if constexpr (VALS) compact(reinterpret_cast<TV*>(s_buf), vout, [&](int r, int c, unsigned) { return v[r][c]; });
	if constexpr (MODE == CLO_OP_ARG) compact(reinterpret_cast<TV*>(s_buf), vout, [&](int, int, unsigned idx) { return (TV) (tile_start + idx); });
}

struct sel_args {
	const void* keys; const void* values; const void* fot; void* kout; void* vout;
	size_t n; int pred, op; unsigned* ws; unsigned long long* num_out; hipStream_t s;
};

inline int sel_scan_launch(unsigned* count, unsigned tiles, size_t n, unsigned long long* num_out, hipStream_t s) {
	clo_timing_scope timing("select_scan", s);
	hipLaunchKernelGGL(clo_select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, s, count, tiles, (unsigned long long) n, num_out);
	return (int) hipGetLastError();
}

template <typename TK, int KIND, int MODE>
int sel_launch(const sel_args& a) {
	typedef typename sel_val<MODE>::T TV;
	constexpr int ROWS = sel_rows((int) sizeof(TK), sel_val<MODE>::size);
	constexpr size_t TILE = (size_t) ROWS * SEL_ROW_ELEMS;
	const unsigned tiles = (unsigned) ((a.n + TILE - 1) / TILE);
	const int kvec = clo_op_vec_ok<TK>(a.keys), vvec = clo_op_vec_ok<TV>(a.values);
	const int fvec = a.pred == CLO_HIP_SELECT_FLAGGED ? clo_op_vec_ok<unsigned char>(a.fot) : 0;
	unsigned* count = a.ws;   // tiles + 1 words: the counts, then the offsets and the total
	{
		clo_timing_scope timing("select_count", a.s);
		hipLaunchKernelGGL((clo_select_count_kernel<TK, KIND>), dim3(tiles), dim3(SEL_THREADS), 0, a.s,
			(const TK*) a.keys, a.fot, a.n, a.pred, ROWS / SEL_CHUNK_ROWS, kvec, fvec, count);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	const int st = sel_scan_launch(count, tiles, a.n, a.num_out, a.s);
	if (st != 0) return st;
	clo_timing_scope timing("select_apply", a.s);
	hipLaunchKernelGGL((clo_select_apply_kernel<TK, KIND, MODE>), dim3(tiles), dim3(SEL_THREADS), 0, a.s,
		(const TK*) a.keys, (const TV*) a.values, a.fot, (TK*) a.kout, (TV*) a.vout, a.n, a.pred, a.op, kvec, fvec, vvec,
		(const unsigned*) count, tiles);
	return (int) hipGetLastError();
}

template <typename TK, int KIND>
int sel_dispatch_mode(const sel_args& a, int mode) {
	switch (mode) {
		case CLO_OP_KEYS: return sel_launch<TK, KIND, CLO_OP_KEYS>(a);
		case CLO_OP_V4: return sel_launch<TK, KIND, CLO_OP_V4>(a);
		case CLO_OP_V8: return sel_launch<TK, KIND, CLO_OP_V8>(a);
		default: return sel_launch<TK, KIND, CLO_OP_ARG>(a);
	}
}

template <typename TK>
int sel_dispatch(const sel_args& a, int kind, int mode) {
	if (kind == 1) return sel_dispatch_mode<TK, 1>(a, mode);
	if constexpr (sizeof(TK) > 1) {
		if (kind == 2) return sel_dispatch_mode<TK, 2>(a, mode);
	}
	return sel_dispatch_mode<TK, 0>(a, mode);
}

}  // namespace

extern "C" {

size_t clo_hip_select_tile(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return sel_tile(key_size, value_size);
}

size_t clo_hip_select_workspace_bytes(size_t numel, int key_size, int value_size) {
	const size_t tile = clo_hip_select_tile(key_size, value_size);
	if (numel == 0 || tile == 0) return 0;
	// one count per tile and the total, 4 bytes each, in whole CLO_HIP_WORKSPACE_ALIGN units
	return clo_op_ws_align(((numel - 1) / tile + 2) * sizeof(unsigned));
}

int clo_hip_select(int op, int pred, const void* keys_in, const void* values_in, const void* flags_or_threshold,
	void* keys_out, void* values_out, uint64_t* num_out, size_t numel, int key_size, int key_kind, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	if (op != CLO_HIP_SELECT_SELECT && op != CLO_HIP_SELECT_PARTITION) return CLO_HIP_EARGS;
	if (pred < CLO_HIP_SELECT_FLAGGED || pred > CLO_HIP_SELECT_NE) return CLO_HIP_EARGS;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!flags_or_threshold && (numel > 0 || pred != CLO_HIP_SELECT_FLAGGED)) return CLO_HIP_EARGS;
	if (!num_out || clo_misaligned(num_out, 8)) return CLO_HIP_EARGS;
	if (!keys_out && !values_out) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	const bool arg = value_size > 0 && !values_in;
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	// the keys are read by every comparison, and wherever they are written
	if (numel > 0 && !keys_in && (pred != CLO_HIP_SELECT_FLAGGED || keys_out)) return CLO_HIP_EARGS;
	if (clo_misaligned(keys_in, (size_t) key_size) || clo_misaligned(keys_out, (size_t) key_size)) return CLO_HIP_EARGS;
	if (pred != CLO_HIP_SELECT_FLAGGED && clo_misaligned(flags_or_threshold, (size_t) key_size)) return CLO_HIP_EARGS;
	if (value_size > 0 && (clo_misaligned(values_in, (size_t) value_size) || clo_misaligned(values_out, (size_t) value_size))) return CLO_HIP_EARGS;
	if (numel > 0) {
		if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
		if (workspace_bytes < clo_hip_select_workspace_bytes(numel, key_size, value_size)) return CLO_HIP_EWORKSPACE;
	}
	if (numel == 0) return sel_scan_launch(nullptr, 0u, 0, (unsigned long long*) num_out, (hipStream_t) stream);   // num_out = 0

	sel_args a;
	a.keys = keys_in; a.values = values_in; a.fot = flags_or_threshold; a.kout = keys_out; a.vout = values_out;
	a.n = numel; a.pred = pred; a.op = op;
	a.ws = (unsigned*) workspace; a.num_out = (unsigned long long*) num_out; a.s = (hipStream_t) stream;
	const int mode = clo_op_mode(value_size, arg);
	return clo_op_by_key_size(key_size, [&](auto tk) { return sel_dispatch<decltype(tk)>(a, key_kind, mode); });
}

}  // extern "C"
