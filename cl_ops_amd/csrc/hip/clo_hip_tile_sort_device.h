// clo_hip_tile_sort_device.h — the on-chip sort of one tile of T = 2048 rows that clo_hip_segsort.hip and
// clo_hip_segtopk.hip share: the composite item, its compare-exchange, the steps that run in a
// lane's registers, the steps that run in LDS and the LDS layout. It is here once because the two files' copies were
// the same text; what a kernel builds the composite from, and what it does with the sorted tile, stays in its file.
// Everything has internal linkage, and every __global__ function stays in its own file under its own name.
#ifndef CLO_HIP_TILE_SORT_DEVICE_H
#define CLO_HIP_TILE_SORT_DEVICE_H

#include "clo_hip_seg_device.h"

namespace {

constexpr int CLO_TS_THREADS = 256;
constexpr int CLO_TS_WAVES = CLO_TS_THREADS / 64;
static_assert(CLO_TS_THREADS == CLO_OP_THREADS, "the shared helpers stride by CLO_OP_THREADS, and clo_op_ends_launch launches groups of it");
constexpr int CLO_TS_ITEMS = 8;                                  // consecutive rows of a lane: one 8-byte load of flags
constexpr unsigned CLO_TS_TILE = CLO_TS_THREADS * CLO_TS_ITEMS;  // T = 2048 rows, for every type
static_assert((CLO_TS_TILE & (CLO_TS_TILE - 1u)) == 0u && CLO_TS_TILE < 32768u, "a power of two; rank and row take 16 bits each");

// Where element i of the tile lies in LDS: inside every aligned group of eight the place is i ^ (group & 7), so that the
// lanes' reads of their own eight consecutive elements (64 or 96 bytes apart) spread over the banks, and a step of
// distance >= 8, whose lanes read consecutive elements, stays spread.
__device__ __forceinline__ unsigned clo_ts_at(unsigned i) { return i ^ ((i >> 3) & 7u); }

// What the network sorts. Keys of up to 4 bytes: k = rank << 48 | order key << 16 | row, tag unused. 8-byte keys: k the
// order key, tag = rank << 16 | row. The padding (all ones) sorts behind every row.
struct clo_ts_item { clo_op_u64 k; unsigned tag; };

template <bool WIDE>
__device__ __forceinline__ bool clo_ts_less(const clo_ts_item& a, const clo_ts_item& b) {
	if constexpr (!WIDE) return a.k < b.k;
	else {
		const unsigned sa = a.tag >> 16, sb = b.tag >> 16;
		return sa != sb ? sa < sb : a.k != b.k ? a.k < b.k : a.tag < b.tag;
	}
}

template <bool WIDE>
__device__ __forceinline__ void clo_ts_cx(clo_ts_item& a, clo_ts_item& b, bool up) {
	if (clo_ts_less<WIDE>(b, a) == up) { const clo_ts_item t = a; a = b; b = t; }
}

// the steps of distance J < CLO_TS_ITEMS of stage `size`, on the lane's own rows [base, base + CLO_TS_ITEMS)
template <bool WIDE, int J>
__device__ __forceinline__ void clo_ts_reg_step(clo_ts_item (&v)[CLO_TS_ITEMS], unsigned base, unsigned size) {
	#pragma unroll
	for (int c = 0; c < CLO_TS_ITEMS; ++c)
		if ((c & J) == 0) clo_ts_cx<WIDE>(v[c], v[c | J], ((base + (unsigned) c) & size) == 0u);
}

template <bool WIDE>
__device__ __forceinline__ void clo_ts_reg_steps(clo_ts_item (&v)[CLO_TS_ITEMS], unsigned base, unsigned size) {
	if (size >= 8u) clo_ts_reg_step<WIDE, 4>(v, base, size);
	if (size >= 4u) clo_ts_reg_step<WIDE, 2>(v, base, size);
	clo_ts_reg_step<WIDE, 1>(v, base, size);
}

// One LDS step of distance j >= CLO_TS_ITEMS of stage `size`: every thread takes CLO_TS_TILE / 2 / CLO_TS_THREADS pairs.
// Element i of the tile lies at s_k[clo_ts_at(i)] (and s_tag[clo_ts_at(i)] for WIDE). The caller's barrier follows.
template <bool WIDE>
__device__ __forceinline__ void clo_ts_lds_step(clo_op_u64* s_k, unsigned* s_tag, unsigned tid, unsigned size, unsigned j) {
	#pragma unroll
	for (unsigned q = 0; q < CLO_TS_TILE / 2u / CLO_TS_THREADS; ++q) {
		const unsigned pr = tid + q * CLO_TS_THREADS;
		const unsigned ea = ((pr & ~(j - 1u)) << 1) | (pr & (j - 1u)), ia = clo_ts_at(ea), ib = clo_ts_at(ea | j);
		clo_ts_item a, b;
		a.k = s_k[ia]; b.k = s_k[ib];
		if constexpr (WIDE) { a.tag = s_tag[ia]; b.tag = s_tag[ib]; } else { a.tag = 0u; b.tag = 0u; }
		if (clo_ts_less<WIDE>(b, a) == ((ea & size) == 0u)) {
			s_k[ia] = b.k; s_k[ib] = a.k;
			if constexpr (WIDE) { s_tag[ia] = b.tag; s_tag[ib] = a.tag; }
		}
	}
}

// the lane's rows [base, base + CLO_TS_ITEMS) between its registers and LDS
template <bool WIDE>
__device__ __forceinline__ void clo_ts_put(const clo_ts_item (&v)[CLO_TS_ITEMS], clo_op_u64* s_k, unsigned* s_tag, unsigned base) {
	#pragma unroll
	for (int c = 0; c < CLO_TS_ITEMS; ++c) {
		s_k[clo_ts_at(base + c)] = v[c].k;
		if constexpr (WIDE) s_tag[clo_ts_at(base + c)] = v[c].tag;
	}
}

template <bool WIDE>
__device__ __forceinline__ void clo_ts_get(clo_ts_item (&v)[CLO_TS_ITEMS], const clo_op_u64* s_k, const unsigned* s_tag, unsigned base) {
	#pragma unroll
	for (int c = 0; c < CLO_TS_ITEMS; ++c) {
		v[c].k = s_k[clo_ts_at(base + c)];
		if constexpr (WIDE) v[c].tag = s_tag[clo_ts_at(base + c)]; else v[c].tag = 0u;
	}
}

// The whole network, as a kernel writes it out (v: the lane's rows, base = tid * CLO_TS_ITEMS):
//   reg_steps 2, 4, 8; put; barrier; for size = 16 .. T: { for j = size / 2 .. CLO_TS_ITEMS: { lds_step; barrier }
//   get; reg_steps(size); put; barrier }
// A macro and not a function on purpose: with the two loops inside one __forceinline__ function (the LDS arrays passed
// as pointers, or as references to arrays) the compiler gave every clo_segsort_tile_kernel for keys of up to 4 bytes 40
// VGPRs instead of 32 (cause not found); with the loops in the kernel's own text and only their bodies as functions the
// resource report of clo_hip_segsort.hip is what it was before the network moved here. Whoever turns
// this into a function compares that report again (tools/resource_usage_diff.py).
#define CLO_TS_SORT(WIDE, v, s_k, s_tag, tid, base) do { \
	clo_ts_reg_steps<WIDE>(v, base, 2u); \
	clo_ts_reg_steps<WIDE>(v, base, 4u); \
	clo_ts_reg_steps<WIDE>(v, base, 8u); \
	clo_ts_put<WIDE>(v, s_k, s_tag, base); \
	__syncthreads(); \
	for (unsigned size = 16u; size <= CLO_TS_TILE; size <<= 1) { \
		for (unsigned j = size >> 1; j >= (unsigned) CLO_TS_ITEMS; j >>= 1) { \
			clo_ts_lds_step<WIDE>(s_k, s_tag, tid, size, j); \
			__syncthreads(); \
		} \
		clo_ts_get<WIDE>(v, s_k, s_tag, base); \
		clo_ts_reg_steps<WIDE>(v, base, size); \
		clo_ts_put<WIDE>(v, s_k, s_tag, base); \
		__syncthreads(); \
	} \
} while (0)

}  // namespace

#endif
