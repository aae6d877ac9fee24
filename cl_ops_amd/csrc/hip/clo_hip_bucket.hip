// clo_hip_bucket.hip — stable multi-way partition of rows by bin, with the buckets' CSR offsets (CloBucket,
// include/clo_bucket.h; not upstream).
//
// The bin of a key is clo_hip_hist.hip's: with the sign bit flipped for signed keys, key >= lower tested on its own,
// bin = (key - lower) >> shift where that is below num_bins; every other row belongs to the REST, which is treated as
// bin num_bins. The rows leave in ascending (bin, input index) order: a stable counting sort by a number of at most 16
// bits, in one pass of 8-bit digits where num_bins + 1 <= 256 and in two stable LSD passes (low byte into the
// workspace, high byte from the workspace into the outputs) above. The digit is recomputed from the key in every
// launch: no bin array is stored.
//
// A pass is five launches, none of which waits for another work-group, none of which uses a global atomic (§10):
//   COUNT    one work-group per tile of 4096 rows counts its digits in LDS and writes them DIGIT-major:
//            counter[digit * tiles + tile], for the digits the pass has;
//   SUMS, SUMS_SCAN, ENDS   the shared three-launch scan of clo_hip_seg_device.h over the digits * tiles counters (the
//            inclusive ends in 64 bits; a group takes CLO_HIP_BUCKET_SCAN_GROUP counters, the one-group scan of the
//            groups' sums CLO_HIP_BUCKET_SCAN_TRIP sums per trip);
//   SCATTER  re-reads the tile, ranks its rows stably on chip and writes keys, values or indices to
//            base[digit][tile] + rank.
// SCATTER's ranking: the lanes load four consecutive keys (vector loads where the array's start allows them) and leave
// the digits in LDS in input order; wave w then walks rows [1024 w, 1024 w + 1024) of the tile 64 at a time, a lane's
// rank being the wave's running count of its digit plus the lanes below it with the same digit (eight ballots); the
// wave counts, scanned digit-major, give every row its slot in the tile; the rows pass through LDS in digit order, one
// array at a time, and leave in runs of consecutive addresses per digit.
// With one pass the scanned counters hold offsets_out (work-group 0 of SCATTER writes it); with two passes it is the
// library's histogram of keys_in, scanned by one work-group.
// Whatever the keys hold: COUNT and SCATTER read the same bytes and so agree; loads are bounded by numel, LDS slots
// by the tile's row count (they are counts of the tile's own rows), and every global row index is tested against numel.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_seg_device.h"

namespace {

constexpr int BKT_THREADS = 256;
constexpr int BKT_WAVES = BKT_THREADS / 64;
constexpr int BKT_VEC = 4;
constexpr int BKT_ROW_ELEMS = BKT_THREADS * BKT_VEC;    // 1024
constexpr int BKT_ROWS = 4;
constexpr unsigned BKT_TILE = BKT_ROWS * BKT_ROW_ELEMS; // 4096
constexpr unsigned BKT_WAVE_ROWS = BKT_TILE / BKT_WAVES; // the stretch of the tile a wave ranks
constexpr int BKT_STEPS = BKT_WAVE_ROWS / 64;           // 16
constexpr unsigned BKT_DIGITS = 256;
constexpr unsigned BKT_OFFS_ITEMS = 8;                  // the two-pass offsets scan takes BKT_THREADS * 8 bins per trip
static_assert(BKT_THREADS == CLO_OP_THREADS && BKT_VEC == CLO_OP_VEC, "the shared helpers' work-group and vector");
static_assert(BKT_DIGITS == (unsigned) BKT_THREADS, "one digit per thread where the digits are scanned");
static_assert(CLO_OP_ENDS_TILE == CLO_HIP_BUCKET_SCAN_GROUP && CLO_OP_SUMS_TRIP == CLO_HIP_BUCKET_SCAN_TRIP, "the header names the scan's capacities");

template <int MODE> struct bkt_val : clo_op_val<MODE> {};

// What turns a key into the digit of a pass.
template <typename TK>
struct bkt_map { TK lo, flip; unsigned shift, num_bins, dshift; };

template <typename TK>
__device__ __forceinline__ unsigned bkt_digit(TK key, const bkt_map<TK>& m) {
	const TK x = (TK) (key ^ m.flip);
	const TK b = (TK) ((TK) (x - m.lo) >> m.shift);
	// key >= lower, explicitly: where lower + (num_bins << shift) runs past the type's maximum, the wrapped difference
	// of a key below lower would land inside the range
	const bool in = x >= m.lo && (unsigned long long) b < (unsigned long long) m.num_bins;
	const unsigned bin = in ? (unsigned) b : m.num_bins;   // the rest: bin num_bins
	return (bin >> m.dshift) & 0xffu;
}

// ---- 1. count ----
template <typename TK>
__global__ __launch_bounds__(BKT_THREADS)
void clo_bucket_count_kernel(const TK* __restrict__ keys, size_t n, bkt_map<TK> m, int kvec, unsigned digits, unsigned tiles,
	unsigned* __restrict__ counter) {
	__shared__ unsigned s_cnt[BKT_DIGITS];
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	const size_t base = (size_t) blockIdx.x * BKT_TILE + (size_t) tid * BKT_VEC;
	TK k[BKT_ROWS][BKT_VEC];
	#pragma unroll
	for (int r = 0; r < BKT_ROWS; ++r) clo_op_load4<TK>(keys, base + (size_t) r * BKT_ROW_ELEMS, n, kvec != 0, k[r]);
	s_cnt[tid] = 0u;
	__syncthreads();
	#pragma unroll
	for (int r = 0; r < BKT_ROWS; ++r) {
		#pragma unroll
		for (int c = 0; c < BKT_VEC; ++c) {
			const bool valid = base + (size_t) r * BKT_ROW_ELEMS + c < n;
			const unsigned d = bkt_digit<TK>(k[r][c], m);
			// the lanes whose digit is the first valid lane's are counted by that lane alone (clo_hip_hist.hip's peel)
			bool add = valid;
			unsigned x = 1u;
			const unsigned long long act = __ballot(valid);
			if (act != 0ull) {   // (wave-uniform)
				const unsigned lead = (unsigned) __ffsll(act) - 1u;
				const unsigned d0 = (unsigned) __builtin_amdgcn_readlane((int) d, (int) lead);
				const bool same = valid && d == d0;
				const unsigned total = (unsigned) __popcll(__ballot(same));
				if (same) { add = lane == lead; x = total; }
			}
			if (add) atomicAdd(&s_cnt[d], x);
		}
	}
	__syncthreads();
	if (tid < digits) counter[(size_t) tid * tiles + blockIdx.x] = s_cnt[tid];
}

// ---- 2. the scan of the digits * tiles counters (clo_hip_seg_device.h). The kernels take neither num_in nor vec_ok and
// the three launches share ONE timing label, so the host launches them here and not through clo_op_ends_launch ----
__global__ __launch_bounds__(BKT_THREADS)
void clo_bucket_sums_kernel(const unsigned* __restrict__ counter, unsigned m_h, clo_op_u64* __restrict__ tsum) {
	clo_op_ends_sums<unsigned>(counter, nullptr, m_h, 1, tsum);
}

__global__ __launch_bounds__(BKT_THREADS)
void clo_bucket_sums_scan_kernel(clo_op_u64* __restrict__ tsum, unsigned tiles) { clo_op_ends_sums_scan(tsum, tiles); }

__global__ __launch_bounds__(BKT_THREADS)
void clo_bucket_ends_kernel(const unsigned* __restrict__ counter, unsigned m_h, const clo_op_u64* __restrict__ tsum, clo_op_u64* __restrict__ ends) {
	clo_op_ends_write<unsigned>(counter, nullptr, m_h, 1, tsum, ends);
}

__device__ __forceinline__ void bkt_store_count(void* out, int count_size, unsigned i, unsigned long long v) {
	if (count_size == 8) static_cast<unsigned long long*>(out)[i] = v;
	else static_cast<unsigned*>(out)[i] = (unsigned) v;
}

// ---- 3. scatter ----
template <typename TK, int MODE>
__global__ __launch_bounds__(BKT_THREADS)
void clo_bucket_scatter_kernel(const TK* __restrict__ keys, const typename bkt_val<MODE>::T* __restrict__ values,
	TK* __restrict__ kout, typename bkt_val<MODE>::T* __restrict__ vout, size_t n, bkt_map<TK> m, int kvec, int vvec,
	unsigned digits, unsigned tiles, const clo_op_u64* __restrict__ ends, void* __restrict__ offsets_out, int count_size) {
	typedef typename bkt_val<MODE>::T TV;
	const int dbits = 32 - __builtin_clz(digits - 1u | 1u);   // the bits in which the pass's digits differ
	constexpr bool VALS = MODE == CLO_OP_V4 || MODE == CLO_OP_V8;
	constexpr size_t ELEM = MODE != CLO_OP_KEYS && sizeof(TV) > sizeof(TK) ? sizeof(TV) : sizeof(TK);
	__shared__ __attribute__((aligned(16))) unsigned char s_buf[BKT_TILE * (ELEM < sizeof(unsigned short) ? sizeof(unsigned short) : ELEM)];
	__shared__ __attribute__((aligned(16))) unsigned char s_dig[BKT_TILE];     // the digits in input order
	// the rows' slots, in input order: in the rows' place, read into registers before the first row arrives
	unsigned short* const s_pos = reinterpret_cast<unsigned short*>(s_buf);
	unsigned char* const s_dsort = s_dig;   // the digits in slot order: in the place of those in input order, once these are dead
	__shared__ unsigned s_cnt[BKT_WAVES][BKT_DIGITS];
	__shared__ unsigned s_start[BKT_DIGITS], s_off[BKT_DIGITS];
	__shared__ unsigned s_wave[BKT_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = (unsigned) __builtin_amdgcn_readfirstlane((int) (tid >> 6));
	const size_t tile_start = (size_t) blockIdx.x * BKT_TILE, base = tile_start + (size_t) tid * BKT_VEC;
	const unsigned cnt = n - tile_start < (size_t) BKT_TILE ? (unsigned) (n - tile_start) : BKT_TILE;   // tile_start < n

	// the loads, and the digits to LDS
	TK k[BKT_ROWS][BKT_VEC];
	TV v[VALS ? BKT_ROWS : 1][BKT_VEC];
	unsigned d4[BKT_ROWS];
	#pragma unroll
	for (int r = 0; r < BKT_ROWS; ++r) {
		const size_t i0 = base + (size_t) r * BKT_ROW_ELEMS;
		clo_op_load4<TK>(keys, i0, n, kvec != 0, k[r]);
		if constexpr (VALS) clo_op_load4<TV>(values, i0, n, vvec != 0, v[r]);
	}
	#pragma unroll
	for (int w = 0; w < BKT_WAVES; ++w) s_cnt[w][tid] = 0u;
	#pragma unroll
	for (int r = 0; r < BKT_ROWS; ++r) {
		unsigned p = 0;
		#pragma unroll
		for (int c = 0; c < BKT_VEC; ++c) p |= bkt_digit<TK>(k[r][c], m) << (8 * c);
		d4[r] = p;
		*reinterpret_cast<unsigned*>(s_dig + (unsigned) r * BKT_ROW_ELEMS + tid * BKT_VEC) = p;
	}
	__syncthreads();

	// the wave's stretch, 64 rows at a time: rank = the wave's count of the digit so far + the lower lanes with it
	unsigned rk[BKT_STEPS];
	const unsigned long long below = (1ull << lane) - 1ull;
	#pragma unroll
	for (int j = 0; j < BKT_STEPS; ++j) {
		const unsigned idx = wave * BKT_WAVE_ROWS + (unsigned) j * 64u + lane;
		const bool valid = idx < cnt;
		const unsigned d = s_dig[idx];
		unsigned long long peers = __ballot(valid);
		#pragma unroll
		for (int b = 0; b < 8; ++b) {
			if (b < dbits) {   // (the same for the whole launch)
				const bool bit = (d >> b) & 1u;
				const unsigned long long mask = __ballot(bit);
				peers &= bit ? mask : ~mask;
			}
		}
		const unsigned pre = s_cnt[wave][d];
		rk[j] = pre + (unsigned) __popcll(peers & below);
		if (valid && lane == (unsigned) __ffsll(peers) - 1u) s_cnt[wave][d] = pre + (unsigned) __popcll(peers);
		__builtin_amdgcn_wave_barrier();   // the next step's counts are read after this step's are written
	}
	__syncthreads();

	// digit tid: the waves' counts become the counts of the waves before; the digits' totals are scanned over the tile
	{
		unsigned run = 0;
		#pragma unroll
		for (int w = 0; w < BKT_WAVES; ++w) {
			const unsigned c = s_cnt[w][tid];
			s_cnt[w][tid] = run;
			run += c;
		}
		const unsigned incl = clo_wave_scan_inclusive<unsigned>(run, lane);
		if (lane == 63u) s_wave[wave] = incl;
		__syncthreads();
		unsigned before = 0;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) BKT_WAVES; ++w) if (w < wave) before += s_wave[w];
		const unsigned start = before + incl - run;
		// where the digit's rows of this tile begin in the output: the end of the counter before this one
		unsigned long long g = 0;
		if (tid < digits) {
			const size_t i = (size_t) tid * tiles + blockIdx.x;
			g = i == 0 ? 0ull : ends[i - 1];
			// one pass: the digits are the bins, and the first tile's bases are the offsets
			if (offsets_out && blockIdx.x == 0) bkt_store_count(offsets_out, count_size, tid, g);
		}
		s_start[tid] = start;
		s_off[tid] = (unsigned) g - start;   // slot j of digit d goes to row s_off[d] + j (modulo 2^32; numel < 2^32)
	}
	__syncthreads();
	#pragma unroll
	for (int j = 0; j < BKT_STEPS; ++j) {
		const unsigned idx = wave * BKT_WAVE_ROWS + (unsigned) j * 64u + lane;
		if (idx < cnt) {
			const unsigned d = s_dig[idx];
			s_pos[idx] = (unsigned short) (s_start[d] + s_cnt[wave][d] + rk[j]);   // < cnt: counts of the tile's own rows
		}
	}
	__syncthreads();
	unsigned short pos[BKT_ROWS][BKT_VEC];
	#pragma unroll
	for (int r = 0; r < BKT_ROWS; ++r) {
		typedef unsigned short us4 __attribute__((ext_vector_type(4)));
		const us4 p = *reinterpret_cast<const us4*>(s_pos + (unsigned) r * BKT_ROW_ELEMS + tid * BKT_VEC);
		#pragma unroll
		for (int c = 0; c < BKT_VEC; ++c) {
			pos[r][c] = p[c];
		}
	}
	__syncthreads();   // every slot and every digit in input order has been read: their places are written from here on
	#pragma unroll
	for (int r = 0; r < BKT_ROWS; ++r) {
		#pragma unroll
		for (int c = 0; c < BKT_VEC; ++c) {
			const unsigned idx = (unsigned) r * BKT_ROW_ELEMS + tid * BKT_VEC + (unsigned) c;
			if (idx < cnt) s_dsort[pos[r][c]] = (unsigned char) (d4[r] >> (8 * c));
		}
	}

	// One array at a time through the tile's LDS, in slot order; slot j then goes to row s_off[digit] + j.
	auto pass = [&](auto* s, auto* out, auto value) {
		#pragma unroll
		for (int r = 0; r < BKT_ROWS; ++r) {
			#pragma unroll
			for (int c = 0; c < BKT_VEC; ++c) {
				const unsigned idx = (unsigned) r * BKT_ROW_ELEMS + tid * BKT_VEC + (unsigned) c;
				if (idx < cnt) s[pos[r][c]] = value(r, c, idx);
			}
		}
		__syncthreads();
		#pragma unroll 4
		for (unsigned j = tid; j < cnt; j += BKT_THREADS) {
			const unsigned row = s_off[s_dsort[j]] + j;
			if (row < n) out[row] = s[j];
		}
	};
	if (kout != nullptr) {
		pass(reinterpret_cast<TK*>(s_buf), kout, [&](int r, int c, unsigned) { return k[r][c]; });
		if constexpr (MODE != CLO_OP_KEYS) __syncthreads();   // the values take the keys' place
	}
	if constexpr (VALS) pass(reinterpret_cast<TV*>(s_buf), vout, [&](int r, int c, unsigned) { return v[r][c]; });
	if constexpr (MODE == CLO_OP_ARG) pass(reinterpret_cast<TV*>(s_buf), vout, [&](int, int, unsigned idx) { return (TV) (tile_start + idx); });
}

// ---- the offsets of two passes: hist[0, num_bins) -> its exclusive sums and the total, num_bins + 1 entries of the
// count type. One work-group. ----
__global__ __launch_bounds__(BKT_THREADS)
void clo_bucket_offsets_kernel(const unsigned* __restrict__ hist, unsigned num_bins, void* __restrict__ offsets_out, int count_size) {
	constexpr unsigned TRIP = BKT_THREADS * BKT_OFFS_ITEMS;
	__shared__ unsigned s_wave[BKT_WAVES];
	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	unsigned carry = 0;   // the sum of all counts is at most numel < 2^32
	for (unsigned base = 0; base < num_bins; base += TRIP) {
		unsigned v[BKT_OFFS_ITEMS], sum = 0;
		#pragma unroll
		for (unsigned c = 0; c < BKT_OFFS_ITEMS; ++c) {
			const unsigned i = base + tid * BKT_OFFS_ITEMS + c;
			v[c] = i < num_bins ? hist[i] : 0u;
			sum += v[c];
		}
		const unsigned incl = clo_wave_scan_inclusive<unsigned>(sum, lane);
		if (lane == 63u) s_wave[wave] = incl;
		__syncthreads();
		unsigned before = 0, total = 0;
		#pragma unroll
		for (unsigned w = 0; w < (unsigned) BKT_WAVES; ++w) {
			const unsigned s = s_wave[w];
			if (w < wave) before += s;
			total += s;
		}
		unsigned at = carry + before + incl - sum;
		#pragma unroll
		for (unsigned c = 0; c < BKT_OFFS_ITEMS; ++c) {
			const unsigned i = base + tid * BKT_OFFS_ITEMS + c;
			if (i < num_bins) bkt_store_count(offsets_out, count_size, i, at);
			at += v[c];
		}
		carry += total;
		__syncthreads();   // s_wave is written again
	}
	if (tid == 0) bkt_store_count(offsets_out, count_size, num_bins, carry);
}

// ---- host ----

// The workspace: the counters, their ends, the sums of the ends' scan; with two passes the rows between the passes and
// the histogram behind them.
struct bkt_layout { size_t counter, ends, tsum, tmp_keys, tmp_values, hist, bytes; };

inline bkt_layout bkt_layout_of(size_t numel, int key_size, int value_size, size_t num_bins) {
	bkt_layout l;
	// the counters of a pass: its digits x tiles; the first of two passes has all 256 digits
	const size_t tiles = (numel + BKT_TILE - 1) / BKT_TILE, counters = tiles * (num_bins + 1 > BKT_DIGITS ? BKT_DIGITS : num_bins + 1);
	size_t at = 0;
	l.counter = at; at += clo_op_ws_align(counters * sizeof(unsigned));
	l.ends = at; at += clo_op_ws_align(counters * sizeof(clo_op_u64));
	l.tsum = at; at += clo_op_ws_align((clo_op_ends_tiles(counters) + 1) * sizeof(clo_op_u64));
	l.tmp_keys = l.tmp_values = l.hist = at;
	if (num_bins + 1 > BKT_DIGITS) {
		l.tmp_keys = at; at += clo_op_ws_align(numel * (size_t) key_size);
		l.tmp_values = at; at += clo_op_ws_align(numel * (size_t) value_size);
		l.hist = at; at += clo_op_ws_align(num_bins * sizeof(unsigned));
	}
	l.bytes = at;
	return l;
}

struct bkt_args {
	const void* keys; const void* values; void* kout; void* vout; void* offsets_out;
	size_t n; unsigned long long lower, flip; unsigned shift, num_bins, dshift, digits; int count_size;
	unsigned* counter; clo_op_u64* ends; clo_op_u64* tsum; hipStream_t s;
};

template <typename TK, int MODE>
int bkt_pass(const bkt_args& a) {
	typedef typename bkt_val<MODE>::T TV;
	const unsigned tiles = (unsigned) ((a.n + BKT_TILE - 1) / BKT_TILE);
	const unsigned m_h = a.digits * tiles;   // <= 2^8 * 2^20
	const unsigned scan_tiles = (unsigned) clo_op_ends_tiles(m_h);
	const int kvec = clo_op_vec_ok<TK>(a.keys), vvec = clo_op_vec_ok<TV>(a.values);
	bkt_map<TK> m;
	m.lo = (TK) ((TK) a.lower ^ (TK) a.flip); m.flip = (TK) a.flip; m.shift = a.shift; m.num_bins = a.num_bins; m.dshift = a.dshift;
	{
		clo_timing_scope timing("bucket_count", a.s);
		hipLaunchKernelGGL((clo_bucket_count_kernel<TK>), dim3(tiles), dim3(BKT_THREADS), 0, a.s, (const TK*) a.keys, a.n, m, kvec, a.digits, tiles, a.counter);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	{
		clo_timing_scope timing("bucket_scan", a.s);
		hipLaunchKernelGGL(clo_bucket_sums_kernel, dim3(scan_tiles), dim3(BKT_THREADS), 0, a.s, (const unsigned*) a.counter, m_h, a.tsum);
		hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
		hipLaunchKernelGGL(clo_bucket_sums_scan_kernel, dim3(1), dim3(BKT_THREADS), 0, a.s, a.tsum, scan_tiles);
		e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
		hipLaunchKernelGGL(clo_bucket_ends_kernel, dim3(scan_tiles), dim3(BKT_THREADS), 0, a.s, (const unsigned*) a.counter, m_h, (const clo_op_u64*) a.tsum, a.ends);
		e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("bucket_scatter", a.s);
	hipLaunchKernelGGL((clo_bucket_scatter_kernel<TK, MODE>), dim3(tiles), dim3(BKT_THREADS), 0, a.s, (const TK*) a.keys, (const TV*) a.values,
		(TK*) a.kout, (TV*) a.vout, a.n, m, kvec, vvec, a.digits, tiles, (const clo_op_u64*) a.ends, a.offsets_out, a.count_size);
	return (int) hipGetLastError();
}

template <typename TK>
int bkt_pass_mode(const bkt_args& a, int mode) {
	switch (mode) {
		case CLO_OP_KEYS: return bkt_pass<TK, CLO_OP_KEYS>(a);
		case CLO_OP_V4: return bkt_pass<TK, CLO_OP_V4>(a);
		case CLO_OP_V8: return bkt_pass<TK, CLO_OP_V8>(a);
		default: return bkt_pass<TK, CLO_OP_ARG>(a);
	}
}

}  // namespace

extern "C" {

size_t clo_hip_bucket_tile(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return BKT_TILE;
}

size_t clo_hip_bucket_workspace_bytes(size_t numel, int key_size, int value_size, size_t num_bins) {
	if (numel == 0 || clo_hip_bucket_tile(key_size, value_size) == 0) return 0;
	return bkt_layout_of(numel, key_size, value_size, num_bins).bytes;
}

int clo_hip_bucket(const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* offsets_out, size_t numel,
	int key_size, int key_signed, int value_size, int count_size, uint64_t lower, unsigned shift, size_t num_bins,
	void* workspace, size_t workspace_bytes, void* stream) {
	hipStream_t s = (hipStream_t) stream;
	if (!offsets_out || num_bins == 0 || num_bins > CLO_HIP_BUCKET_MAX_BINS || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return CLO_HIP_EUNSUPPORTED;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	if (shift >= 8u * (unsigned) key_size) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	const bool arg = value_size > 0 && !values_in;
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	if (!keys_out && !arg) return CLO_HIP_EARGS;
	if (numel > 0 && !keys_in) return CLO_HIP_EARGS;
	if (clo_misaligned(keys_in, (size_t) key_size) || clo_misaligned(keys_out, (size_t) key_size)) return CLO_HIP_EARGS;
	if (value_size > 0 && (clo_misaligned(values_in, (size_t) value_size) || clo_misaligned(values_out, (size_t) value_size))) return CLO_HIP_EARGS;
	if (clo_misaligned(offsets_out, (size_t) count_size)) return CLO_HIP_EARGS;
	if (numel > 0) {
		if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
		if (workspace_bytes < clo_hip_bucket_workspace_bytes(numel, key_size, value_size, num_bins)) return CLO_HIP_EWORKSPACE;
	}
	if (numel == 0) return (int) hipMemsetAsync(offsets_out, 0, (num_bins + 1) * (size_t) count_size, s);

	const bkt_layout l = bkt_layout_of(numel, key_size, value_size, num_bins);
	char* const ws = (char*) workspace;
	bkt_args a;
	a.n = numel; a.lower = lower; a.flip = key_signed ? 1ull << (8 * key_size - 1) : 0ull;
	a.shift = shift; a.num_bins = (unsigned) num_bins; a.count_size = count_size; a.s = s;
	a.counter = (unsigned*) (ws + l.counter); a.ends = (clo_op_u64*) (ws + l.ends); a.tsum = (clo_op_u64*) (ws + l.tsum);
	const int mode = clo_op_mode(value_size, arg);
	if (num_bins + 1 <= BKT_DIGITS) {
		a.keys = keys_in; a.values = values_in; a.kout = keys_out; a.vout = values_out; a.offsets_out = offsets_out;
		a.dshift = 0u; a.digits = (unsigned) num_bins + 1u;
		return clo_op_by_key_size(key_size, [&](auto tk) { return bkt_pass_mode<decltype(tk)>(a, mode); });
	}
	// two stable passes, the low byte of the bin first; the rows between them lie in the workspace
	a.keys = keys_in; a.values = values_in; a.kout = ws + l.tmp_keys; a.vout = value_size > 0 ? ws + l.tmp_values : nullptr; a.offsets_out = nullptr;
	a.dshift = 0u; a.digits = BKT_DIGITS;
	int st = clo_op_by_key_size(key_size, [&](auto tk) { return bkt_pass_mode<decltype(tk)>(a, mode); });
	if (st != 0) return st;
	a.keys = ws + l.tmp_keys; a.values = a.vout; a.kout = keys_out; a.vout = values_out;
	a.dshift = 8u; a.digits = ((unsigned) num_bins >> 8) + 1u;
	st = clo_op_by_key_size(key_size, [&](auto tk) { return bkt_pass_mode<decltype(tk)>(a, mode == CLO_OP_ARG ? CLO_OP_V4 : mode); });
	if (st != 0) return st;
	// the offsets: this library's histogram of keys_in under the same mapping, scanned
	unsigned* const hist = (unsigned*) (ws + l.hist);
	st = clo_hip_histogram(keys_in, nullptr, hist, numel, key_size, key_signed, 5, 5, lower, shift, num_bins, 0, 0u, nullptr, 0, stream);
	if (st != 0) return st;
	clo_timing_scope timing("bucket_offsets", s);
	hipLaunchKernelGGL(clo_bucket_offsets_kernel, dim3(1), dim3(BKT_THREADS), 0, s, (const unsigned*) hist, (unsigned) num_bins, offsets_out, count_size);
	return (int) hipGetLastError();
}

}  // extern "C"
