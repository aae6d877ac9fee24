/*
 * clo_hip_segscan_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * segmented scan (clo_hip_segscan, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_segscan.c) links and runs on the CPU under the sanitizers
 * (tests/segscan_host/segscan_host_test.c, tests/test_segscan_cpu.py). One serial walk over the segments with the same
 * contract and the same status codes as the device code: m = min(numel_seg, *num_in), every end clipped to numel, a
 * segment's rows [max(previous clipped end, 0), clipped end) — an end below its predecessor gives an empty range — rows
 * [0, min(total, numel)) of data_out written and no other. A row's value is read before its result is written, so
 * that data_out may be values_in. A short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SEGSCAN_TILE 4352u
#define SEGSCAN_ENDS_TILE 4096u

static size_t segscan_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }
/* CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7 */
static int segscan_int_type(int t) { return t >= 4 && t <= 7; }
static int segscan_type_size(int t) { return t >= 6 ? 8 : 4; }
static int segscan_type_signed(int t) { return t == 4 || t == 6; }

size_t clo_hip_segscan_tile(int value_size, int sum_size) {
	return (value_size == 4 || value_size == 8) && (sum_size == 4 || sum_size == 8) && sum_size >= value_size ? SEGSCAN_TILE : 0;
}

size_t clo_hip_segscan_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	const size_t tiles = (numel_seg + numel + SEGSCAN_TILE - 1) / SEGSCAN_TILE;
	return segscan_align(numel_seg * 8) + segscan_align((tiles + 1) * 4) + segscan_align(tiles * 4) + segscan_align(tiles * 8)
		+ segscan_align(((numel_seg + SEGSCAN_ENDS_TILE - 1) / SEGSCAN_ENDS_TILE + 1) * 8);
}

static uint64_t segscan_word(const void* p, size_t i, int size) {
	if (size == 8) { uint64_t v; memcpy(&v, (const char*) p + i * 8, 8); return v; }
	uint32_t v;
	memcpy(&v, (const char*) p + i * 4, 4);
	return v;
}

/* (sum type) value, as the bits of a 64-bit word */
static uint64_t segscan_value(const void* values, size_t i, int value_type, int sum_type) {
	uint64_t v = segscan_word(values, i, segscan_type_size(value_type));
	if (segscan_type_size(value_type) == 4 && segscan_type_signed(value_type)) v = (uint64_t) (int64_t) (int32_t) (uint32_t) v;
	return segscan_type_size(sum_type) == 4 ? (uint32_t) v : v;
}

int clo_hip_segscan(int op, int inclusive, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* data_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (op < 0 || op > 2) return CLO_HIP_EARGS;
	if (inclusive != 0 && inclusive != 1) return CLO_HIP_EARGS;
	if (form != CLO_HIP_SEGSCAN_COUNTS && form != CLO_HIP_SEGSCAN_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	if (!segscan_int_type(value_type) || !segscan_int_type(sum_type) || segscan_type_size(sum_type) < segscan_type_size(value_type))
		return CLO_HIP_EUNSUPPORTED;
	const size_t vs = (size_t) segscan_type_size(value_type), ss = (size_t) segscan_type_size(sum_type);
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGSCAN_OFFSETS)) return CLO_HIP_EARGS;
	if ((!values_in || !data_out) && numel > 0) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8 || (uintptr_t) num_in % 8) return CLO_HIP_EARGS;
	if ((uintptr_t) counts_or_offsets % (size_t) count_size || (uintptr_t) values_in % vs || (uintptr_t) data_out % ss) return CLO_HIP_EARGS;
	if (numel_seg == 0) { *num_out = 0; return 0; }
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_segscan_workspace_bytes(numel_seg, numel)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, clo_hip_segscan_workspace_bytes(numel_seg, numel));   /* the kernels write it */

	const uint32_t m_h = (uint32_t) numel_seg;
	const uint32_t m = num_in && *num_in < m_h ? (uint32_t) *num_in : m_h;
	const int is_signed = segscan_type_signed(sum_type);
	const uint64_t top = ss == 8 ? 1ull << 63 : 1ull << 31, mask = ss == 8 ? ~0ull : 0xffffffffull;
	/* min and max on unsigned numbers, a signed sum type with its sign bit flipped */
	const uint64_t flip = (op != 0 && is_signed) ? top : 0;
	const uint64_t identity = op == 1 ? mask : 0;
	const uint64_t base = form == CLO_HIP_SEGSCAN_OFFSETS ? segscan_word(counts_or_offsets, 0, count_size) : 0;
	/* the total first: rows at and beyond min(total, numel) are not written, whatever the ends before the last say */
	uint64_t total = 0;
	if (form == CLO_HIP_SEGSCAN_OFFSETS) total = m ? segscan_word(counts_or_offsets, m, count_size) - base : 0;
	else for (uint32_t r = 0; r < m; ++r) total += segscan_word(counts_or_offsets, r, count_size);
	const uint64_t ct = total < numel ? total : numel;
	uint64_t end = 0, from = 0;   /* the running end; the previous clipped end */
	for (uint32_t r = 0; r < m; ++r) {
		if (form == CLO_HIP_SEGSCAN_OFFSETS) end = segscan_word(counts_or_offsets, (size_t) r + 1, count_size) - base;
		else end += segscan_word(counts_or_offsets, r, count_size);
		const uint64_t to = end < ct ? end : ct;
		uint64_t acc = identity;
		for (uint64_t i = from; i < to; ++i) {
			const uint64_t x = segscan_value(values_in, (size_t) i, value_type, sum_type) ^ flip;
			uint64_t after;
			if (op == 0) after = (acc + x) & mask;
			else if (op == 1) after = x < acc ? x : acc;
			else after = x > acc ? x : acc;
			const uint64_t w = (inclusive ? after : acc) ^ flip;
			if (ss == 8) memcpy((char*) data_out + (size_t) i * 8, &w, 8);
			else { const uint32_t w32 = (uint32_t) w; memcpy((char*) data_out + (size_t) i * 4, &w32, 4); }
			acc = after;
		}
		if (to > from) from = to;
	}
	*num_out = total;
	return 0;
}
