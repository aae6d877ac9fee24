/*
 * clo_hip_segfsum_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * floating-point segment sum (clo_hip_segfsum, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_segfsum.c) links and runs on the CPU under the sanitizers
 * (tests/segfsum_host/segfsum_host_test.c, tests/test_segfsum_cpu.py). One SERIAL walk over the segments with the same
 * contract and the same status codes as the device code, but NOT its order of addition (tests/segfsum_model.py has
 * that): m = min(numel_seg, *num_in), every end clipped to numel, a segment's rows [max(previous clipped end, 0),
 * clipped end) — an end below its predecessor gives an empty range — added left to right from +0 in the sum type,
 * rows [0, m) of sums_out written. A short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SEGFSUM_TILE 4352u
#define SEGFSUM_ENDS_TILE 4096u
/* CloType numbers (clo_common.h) */
#define SEGFSUM_HALF 8
#define SEGFSUM_FLOAT 9
#define SEGFSUM_DOUBLE 10

static size_t segfsum_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }

size_t clo_hip_segfsum_tile(int value_size, int sum_size) {
	return ((value_size == 2 && sum_size == 4) || (value_size == 4 && sum_size == 4) || (value_size == 4 && sum_size == 8)
		|| (value_size == 8 && sum_size == 8)) ? SEGFSUM_TILE : 0;
}

size_t clo_hip_segfsum_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	const size_t tiles = (numel_seg + numel + SEGFSUM_TILE - 1) / SEGFSUM_TILE;
	return segfsum_align(numel_seg * 8) + segfsum_align((tiles + 1) * 4) + 2 * segfsum_align(tiles * 4) + segfsum_align(tiles * 8)
		+ segfsum_align(((numel_seg + SEGFSUM_ENDS_TILE - 1) / SEGFSUM_ENDS_TILE + 1) * 8);
}

static uint64_t segfsum_word(const void* p, size_t i, int size) {
	if (size == 8) { uint64_t v; memcpy(&v, (const char*) p + i * 8, 8); return v; }
	uint32_t v;
	memcpy(&v, (const char*) p + i * 4, 4);
	return v;
}

/* (float) half, exact: subnormals, infinities and NaNs included */
static float segfsum_half(uint16_t h) {
	const uint32_t sign = (uint32_t) (h & 0x8000u) << 16, exp = (h >> 10) & 31u, man = h & 0x3ffu;
	uint32_t bits;
	if (exp == 31u) bits = sign | 0x7f800000u | (man << 13);
	else if (exp != 0u) bits = sign | ((exp + 112u) << 23) | (man << 13);
	else if (man == 0u) bits = sign;
	else {   /* a subnormal: man * 2^-24 */
		const float f = (float) man * (1.0f / 16777216.0f);
		memcpy(&bits, &f, 4);
		bits |= sign;
	}
	float f;
	memcpy(&f, &bits, 4);
	return f;
}

/* (double) values_in[i]: every value type is exact in a double, and a float sum is rounded back below */
static double segfsum_value(const void* values, size_t i, int value_type) {
	if (value_type == SEGFSUM_HALF) { uint16_t h; memcpy(&h, (const char*) values + i * 2, 2); return (double) segfsum_half(h); }
	if (value_type == SEGFSUM_FLOAT) { float f; memcpy(&f, (const char*) values + i * 4, 4); return (double) f; }
	double d;
	memcpy(&d, (const char*) values + i * 8, 8);
	return d;
}

int clo_hip_segfsum(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* sums_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (form != CLO_HIP_SEGFSUM_COUNTS && form != CLO_HIP_SEGFSUM_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	if (!((value_type == SEGFSUM_HALF && sum_type == SEGFSUM_FLOAT) || (value_type == SEGFSUM_FLOAT && sum_type == SEGFSUM_FLOAT)
		|| (value_type == SEGFSUM_FLOAT && sum_type == SEGFSUM_DOUBLE) || (value_type == SEGFSUM_DOUBLE && sum_type == SEGFSUM_DOUBLE)))
		return CLO_HIP_EUNSUPPORTED;
	const size_t vs = value_type == SEGFSUM_HALF ? 2 : value_type == SEGFSUM_FLOAT ? 4 : 8, ss = sum_type == SEGFSUM_FLOAT ? 4 : 8;
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGFSUM_OFFSETS)) return CLO_HIP_EARGS;
	if (!values_in && numel > 0) return CLO_HIP_EARGS;
	if (!sums_out && numel_seg > 0) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8 || (uintptr_t) num_in % 8) return CLO_HIP_EARGS;
	if ((uintptr_t) counts_or_offsets % (size_t) count_size || (uintptr_t) values_in % vs || (uintptr_t) sums_out % ss) return CLO_HIP_EARGS;
	if (numel_seg == 0) { *num_out = 0; return 0; }
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_segfsum_workspace_bytes(numel_seg, numel)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, clo_hip_segfsum_workspace_bytes(numel_seg, numel));   /* the kernels write it */

	const uint32_t m_h = (uint32_t) numel_seg;
	const uint32_t m = num_in && *num_in < m_h ? (uint32_t) *num_in : m_h;
	const uint64_t base = form == CLO_HIP_SEGFSUM_OFFSETS ? segfsum_word(counts_or_offsets, 0, count_size) : 0;
	uint64_t end = 0, from = 0;   /* the running end; the previous clipped end */
	for (uint32_t r = 0; r < m; ++r) {
		if (form == CLO_HIP_SEGFSUM_OFFSETS) end = segfsum_word(counts_or_offsets, (size_t) r + 1, count_size) - base;
		else end += segfsum_word(counts_or_offsets, r, count_size);
		const uint64_t to = end < numel ? end : numel;
		if (ss == 4) {
			float acc = 0.0f;
			for (uint64_t i = from; i < to; ++i) acc = acc + (float) segfsum_value(values_in, (size_t) i, value_type);
			memcpy((char*) sums_out + (size_t) r * 4, &acc, 4);
		} else {
			double acc = 0.0;
			for (uint64_t i = from; i < to; ++i) acc = acc + segfsum_value(values_in, (size_t) i, value_type);
			memcpy((char*) sums_out + (size_t) r * 8, &acc, 8);
		}
		if (to > from) from = to;
	}
	*num_out = end;
	return 0;
}
