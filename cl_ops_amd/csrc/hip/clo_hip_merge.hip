// clo_hip_merge.hip — stable merge of two sorted arrays (CloMerge, include/clo_merge.h; not upstream), with values
// carried along or the permutation written (argmerge): one read and one write of every element.
//
// A merge-path schedule in two launches, neither of which waits for another work-group:
//   PARTITION  one thread per tile boundary d = t * TILE of the OUTPUT: a binary search along the diagonal d finds how
//              many of the first d outputs come from A under the stable rule "take from A while a <= b", and writes
//              it to split[t] (tiles + 1 words of the workspace);
//   MERGE      one work-group per tile. It reads split[t] and split[t + 1] and CLAMPS both to what the sizes alone
//              allow, so that whatever the searches found on unsorted inputs every read stays inside the inputs and
//              every write inside its own TILE outputs. It stages its A range and its B range, together at most TILE
//              keys, in LDS in unsigned order (clo_keyx_fwd), each thread finds its own diagonal there and merges
//              ITEMS outputs serially in registers, remembering for each the LDS slot it came from. Keys go back
//              through LDS (original bits: clo_keyx_inv) and out in output order. Values are staged in LDS by slot and
//              gathered in output order; for argmerge the slot plus the tile's bases IS the value.
// Global loads and stores are 16-byte vectors from the first 16-byte boundary of a range on, single elements before it
// and after the last whole vector. ITEMS is odd: the threads' strided LDS accesses fall on different banks.
// Edges (a last partial tile, a tile fed by one input only, an empty input) are the same code with counts of 0.
#include <hip/hip_runtime.h>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_op_device.h"

namespace {

constexpr int MERGE_THREADS = 256;
static_assert(MERGE_THREADS == CLO_OP_THREADS, "the shared helpers stride by CLO_OP_THREADS");
constexpr int merge_items(int key_size) { return key_size <= 2 ? 17 : 9; }
constexpr size_t merge_tile(int key_size) { return (size_t) MERGE_THREADS * merge_items(key_size); }
constexpr size_t MERGE_MIN_TILE = merge_tile(8);   // sizes the workspace, whose getter does not know the key size

// the modes CLO_OP_KEYS, V4, V8 and ARG (clo_hip_op_device.h); the table keeps a name of its own here because the
// kernels' symbols spell it
template <int MODE> struct merge_val : clo_op_val<MODE> {};

template <typename TK>
__global__ __launch_bounds__(MERGE_THREADS)
void clo_merge_partition_kernel(const TK* __restrict__ ka, const TK* __restrict__ kb, unsigned na, unsigned nb, unsigned tiles,
	clo_keyx kx, unsigned* __restrict__ split) {
	clo_op_partition<TK, merge_tile((int) sizeof(TK))>(ka, kb, na, nb, tiles, kx, split);
}

template <typename TK, int MODE>
__global__ __launch_bounds__(MERGE_THREADS)
void clo_merge_kernel(const TK* __restrict__ ka, const typename merge_val<MODE>::T* __restrict__ va, unsigned na,
	const TK* __restrict__ kb, const typename merge_val<MODE>::T* __restrict__ vb, unsigned nb,
	TK* __restrict__ kout, typename merge_val<MODE>::T* __restrict__ vout, const unsigned* __restrict__ split, clo_keyx kx) {
	typedef typename merge_val<MODE>::T TV;
	constexpr int ITEMS = merge_items((int) sizeof(TK));
	constexpr unsigned TILE = (unsigned) merge_tile((int) sizeof(TK));
	constexpr bool VALS = MODE == CLO_OP_V4 || MODE == CLO_OP_V8;
	static_assert(TILE <= 65536u, "slots are 16-bit");
	__shared__ __attribute__((aligned(16))) TK s_keys[TILE];
	__shared__ unsigned short s_slot[MODE == CLO_OP_KEYS ? 1 : TILE];
	__shared__ __attribute__((aligned(16))) TV s_vals[VALS ? TILE : 1];
	const unsigned tid = threadIdx.x;

	// the tile's outputs [d0, d0 + cnt) and its ranges [a0, a0 + na_t) of A and [b0, b0 + nb_t) of B, the splits clamped
	const clo_op_range r = clo_op_tile_range<TILE>(split, na, nb);
	const unsigned d0 = r.d0, cnt = r.cnt, a0 = r.a0, b0 = r.b0, na_t = r.na_t, nb_t = r.nb_t;

	clo_op_stage<TK, true>(ka + a0, na_t, s_keys, kx, tid);
	clo_op_stage<TK, true>(kb + b0, nb_t, s_keys + na_t, kx, tid);
	if constexpr (VALS) {   // requested now, needed after the merge
		clo_op_stage<TV, false>(va + a0, na_t, s_vals, kx, tid);
		clo_op_stage<TV, false>(vb + b0, nb_t, s_vals + na_t, kx, tid);
	}
	__syncthreads();

	// this thread's ITEMS outputs start at diagonal tid * ITEMS of the tile; past cnt nothing is valid and nothing is written
	const unsigned diag = clo_op_min(tid * ITEMS, cnt);
	unsigned ai = clo_op_path<TK, false>(s_keys, s_keys + na_t, na_t, nb_t, diag, kx);
	unsigned bi = diag - ai;
	TK x = s_keys[clo_op_min(ai, TILE - 1u)], y = s_keys[clo_op_min(na_t + bi, TILE - 1u)];
	TK out[ITEMS];
	unsigned slot[ITEMS];
	#pragma unroll
	for (int i = 0; i < ITEMS; ++i) {
		// x is looked at only while ai < na_t, y only while bi < nb_t
		const bool from_a = bi >= nb_t || (ai < na_t && x <= y);
		out[i] = from_a ? x : y;
		slot[i] = from_a ? ai : na_t + bi;
		if (from_a) ++ai; else ++bi;
		const TK next = s_keys[clo_op_min(from_a ? ai : na_t + bi, TILE - 1u)];
		if (from_a) x = next; else y = next;
	}
	__syncthreads();   // every thread has read its keys: s_keys becomes the output tile
	#pragma unroll
	for (int i = 0; i < ITEMS; ++i) {
		const unsigned j = tid * ITEMS + i;
		if (j < cnt) {
			s_keys[j] = clo_keyx_inv<TK>(out[i], kx);
			if constexpr (MODE != CLO_OP_KEYS) s_slot[j] = (unsigned short) slot[i];   // < cnt
		}
	}
	__syncthreads();
	if (kout) clo_op_store<TK>(kout + d0, cnt, tid, [&](unsigned j) { return s_keys[j]; });
	if constexpr (VALS) clo_op_store<TV>(vout + d0, cnt, tid, [&](unsigned j) { return s_vals[s_slot[j]]; });
	if constexpr (MODE == CLO_OP_ARG) {
		const unsigned base_b = na + b0 - na_t;   // slot s >= na_t is B[b0 + s - na_t], index na + b0 + s - na_t of A || B (mod 2^32: exact)
		clo_op_store<TV>(vout + d0, cnt, tid, [&](unsigned j) { const unsigned s = s_slot[j]; return s < na_t ? a0 + s : base_b + s; });
	}
}

struct merge_args {
	const void* ka; const void* va; const void* kb; const void* vb; void* kout; void* vout;
	unsigned na, nb; clo_keyx kx; unsigned* split; hipStream_t s;
};

template <typename TK, int MODE>
int merge_launch(const merge_args& a) {
	typedef typename merge_val<MODE>::T TV;
	const size_t tile = merge_tile((int) sizeof(TK));
	const unsigned tiles = (unsigned) (((size_t) a.na + a.nb + tile - 1) / tile);
	{
		clo_timing_scope timing("merge_partition", a.s);
		hipLaunchKernelGGL((clo_merge_partition_kernel<TK>), dim3(tiles / MERGE_THREADS + 1u), dim3(MERGE_THREADS), 0, a.s,
			(const TK*) a.ka, (const TK*) a.kb, a.na, a.nb, tiles, a.kx, a.split);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int) e;
	}
	clo_timing_scope timing("merge", a.s);
	hipLaunchKernelGGL((clo_merge_kernel<TK, MODE>), dim3(tiles), dim3(MERGE_THREADS), 0, a.s,
		(const TK*) a.ka, (const TV*) a.va, a.na, (const TK*) a.kb, (const TV*) a.vb, a.nb, (TK*) a.kout, (TV*) a.vout,
		(const unsigned*) a.split, a.kx);
	return (int) hipGetLastError();
}

template <typename TK>
int merge_dispatch(const merge_args& a, int mode) {
	switch (mode) {
		case CLO_OP_KEYS: return merge_launch<TK, CLO_OP_KEYS>(a);
		case CLO_OP_V4: return merge_launch<TK, CLO_OP_V4>(a);
		case CLO_OP_V8: return merge_launch<TK, CLO_OP_V8>(a);
		default: return merge_launch<TK, CLO_OP_ARG>(a);
	}
}

}  // namespace

extern "C" {

size_t clo_hip_merge_tile(int key_size, int value_size) {
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size)) return 0;
	return merge_tile(key_size);
}

size_t clo_hip_merge_workspace_bytes(size_t numel_a, size_t numel_b) {
	const size_t n = numel_a + numel_b;
	if (n == 0 || n < numel_a) return 0;
	// tiles + 1 split points of 4 bytes for the smallest tile, in whole CLO_HIP_WORKSPACE_ALIGN units
	return clo_op_ws_align(((n + MERGE_MIN_TILE - 1) / MERGE_MIN_TILE + 1) * sizeof(unsigned));
}

int clo_hip_merge(const void* keys_a, const void* values_a, size_t numel_a, const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, int key_size, int key_kind, int value_size, void* workspace, size_t workspace_bytes, void* stream) {
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!clo_op_key_size_ok(key_size) || !clo_op_value_size_ok(value_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull) return CLO_HIP_EARGS;
	if ((numel_a > 0 && !keys_a) || (numel_b > 0 && !keys_b)) return CLO_HIP_EARGS;
	if (!keys_out && !values_out) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_a || values_b || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	// the values of an empty input are not looked at; those of the others are all given, or all NULL (argmerge)
	const bool given_a = numel_a > 0 && values_a, given_b = numel_b > 0 && values_b;
	const bool absent_a = numel_a > 0 && !values_a, absent_b = numel_b > 0 && !values_b;
	if ((given_a && absent_b) || (given_b && absent_a)) return CLO_HIP_EARGS;
	const bool arg = value_size > 0 && (absent_a || absent_b);
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	if (clo_misaligned(keys_a, (size_t) key_size) || clo_misaligned(keys_b, (size_t) key_size) || clo_misaligned(keys_out, (size_t) key_size))
		return CLO_HIP_EARGS;
	if (value_size > 0 && (clo_misaligned(values_a, (size_t) value_size) || clo_misaligned(values_b, (size_t) value_size)
		|| clo_misaligned(values_out, (size_t) value_size))) return CLO_HIP_EARGS;
	if (numel_a + numel_b == 0) return 0;
	if (!workspace || clo_ws_misaligned(workspace)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_merge_workspace_bytes(numel_a, numel_b)) return CLO_HIP_EWORKSPACE;

	merge_args a;
	a.ka = keys_a; a.va = arg ? nullptr : values_a; a.kb = keys_b; a.vb = arg ? nullptr : values_b;
	a.kout = keys_out; a.vout = values_out;
	a.na = (unsigned) numel_a; a.nb = (unsigned) numel_b;
	a.kx = clo_keyx_make(key_kind, 0, 8 * key_size);
	a.split = (unsigned*) workspace; a.s = (hipStream_t) stream;
	const int mode = clo_op_mode(value_size, arg);
	return clo_op_by_key_size(key_size, [&](auto tk) { return merge_dispatch<decltype(tk)>(a, mode); });
}

}  // extern "C"
