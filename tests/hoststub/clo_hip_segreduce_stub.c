/*
 * clo_hip_segreduce_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * segmented reduction (clo_hip_segreduce, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_segreduce.c) links and runs on the CPU under the sanitizers
 * (tests/segreduce_host/segreduce_host_test.c, tests/test_segreduce_cpu.py). One serial walk over the segments with the
 * same contract and the same status codes as the device code: m = min(numel_seg, *num_in), every end clipped to numel,
 * a segment's rows [max(previous clipped end, 0), clipped end) — an end below its predecessor gives an empty range —
 * rows [0, m) of aggr_out written. A short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SEGREDUCE_TILE 4352u
#define SEGREDUCE_ENDS_TILE 4096u

static size_t segreduce_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }
/* CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7 */
static int segreduce_int_type(int t) { return t >= 4 && t <= 7; }
static int segreduce_type_size(int t) { return t >= 6 ? 8 : 4; }
static int segreduce_type_signed(int t) { return t == 4 || t == 6; }

size_t clo_hip_segreduce_tile(int value_size, int sum_size) {
	return (value_size == 4 || value_size == 8) && (sum_size == 4 || sum_size == 8) && sum_size >= value_size ? SEGREDUCE_TILE : 0;
}

size_t clo_hip_segreduce_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	const size_t tiles = (numel_seg + numel + SEGREDUCE_TILE - 1) / SEGREDUCE_TILE;
	return segreduce_align(numel_seg * 8) + segreduce_align((tiles + 1) * 4) + 2 * segreduce_align(tiles * 4) + segreduce_align(tiles * 8)
		+ segreduce_align(((numel_seg + SEGREDUCE_ENDS_TILE - 1) / SEGREDUCE_ENDS_TILE + 1) * 8);
}

static uint64_t segreduce_word(const void* p, size_t i, int size) {
	if (size == 8) { uint64_t v; memcpy(&v, (const char*) p + i * 8, 8); return v; }
	uint32_t v;
	memcpy(&v, (const char*) p + i * 4, 4);
	return v;
}

/* (sum type) value, as the bits of a 64-bit word */
static uint64_t segreduce_value(const void* values, size_t i, int value_type, int sum_type) {
	uint64_t v = segreduce_word(values, i, segreduce_type_size(value_type));
	if (segreduce_type_size(value_type) == 4 && segreduce_type_signed(value_type)) v = (uint64_t) (int64_t) (int32_t) (uint32_t) v;
	return segreduce_type_size(sum_type) == 4 ? (uint32_t) v : v;
}

int clo_hip_segreduce(int op, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* aggr_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (op < 0 || op > 2) return CLO_HIP_EARGS;
	if (form != CLO_HIP_SEGREDUCE_COUNTS && form != CLO_HIP_SEGREDUCE_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	if (!segreduce_int_type(value_type) || !segreduce_int_type(sum_type) || segreduce_type_size(sum_type) < segreduce_type_size(value_type))
		return CLO_HIP_EUNSUPPORTED;
	const size_t vs = (size_t) segreduce_type_size(value_type), ss = (size_t) segreduce_type_size(sum_type);
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGREDUCE_OFFSETS)) return CLO_HIP_EARGS;
	if (!values_in && numel > 0) return CLO_HIP_EARGS;
	if (!aggr_out && numel_seg > 0) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8 || (uintptr_t) num_in % 8) return CLO_HIP_EARGS;
	if ((uintptr_t) counts_or_offsets % (size_t) count_size || (uintptr_t) values_in % vs || (uintptr_t) aggr_out % ss) return CLO_HIP_EARGS;
	if (numel_seg == 0) { *num_out = 0; return 0; }
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_segreduce_workspace_bytes(numel_seg, numel)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, clo_hip_segreduce_workspace_bytes(numel_seg, numel));   /* the kernels write it */

	const uint32_t m_h = (uint32_t) numel_seg;
	const uint32_t m = num_in && *num_in < m_h ? (uint32_t) *num_in : m_h;
	const int is_signed = segreduce_type_signed(sum_type);
	const uint64_t top = ss == 8 ? 1ull << 63 : 1ull << 31, mask = ss == 8 ? ~0ull : 0xffffffffull;
	/* min and max on unsigned numbers, a signed sum type with its sign bit flipped */
	const uint64_t flip = (op != 0 && is_signed) ? top : 0;
	const uint64_t identity = op == 1 ? mask : 0;
	const uint64_t base = form == CLO_HIP_SEGREDUCE_OFFSETS ? segreduce_word(counts_or_offsets, 0, count_size) : 0;
	uint64_t end = 0, from = 0;   /* the running end; the previous clipped end */
	for (uint32_t r = 0; r < m; ++r) {
		if (form == CLO_HIP_SEGREDUCE_OFFSETS) end = segreduce_word(counts_or_offsets, (size_t) r + 1, count_size) - base;
		else end += segreduce_word(counts_or_offsets, r, count_size);
		const uint64_t to = end < numel ? end : numel;
		uint64_t acc = identity;
		for (uint64_t i = from; i < to; ++i) {
			const uint64_t x = segreduce_value(values_in, (size_t) i, value_type, sum_type) ^ flip;
			if (op == 0) acc = (acc + x) & mask;
			else if (op == 1) acc = x < acc ? x : acc;
			else acc = x > acc ? x : acc;
		}
		acc ^= flip;
		if (ss == 8) memcpy((char*) aggr_out + (size_t) r * 8, &acc, 8);
		else { const uint32_t a32 = (uint32_t) acc; memcpy((char*) aggr_out + (size_t) r * 4, &a32, 4); }
		if (to > from) from = to;
	}
	*num_out = end;
	return 0;
}
