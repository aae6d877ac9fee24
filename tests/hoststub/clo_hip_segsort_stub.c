/*
 * clo_hip_segsort_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * segmented sort (clo_hip_segsort, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_segsort.c) links and runs on the CPU under the sanitizers
 * (tests/segsort_host/segsort_host_test.c, tests/test_segsort_cpu.py). One serial walk over the segments with the same
 * contract and the same status codes as the device code: m = min(numel_seg, *num_in), every end clipped to numel, a
 * segment's rows [previous clipped end, clipped end) — an end below its predecessor gives an empty range — sorted by an
 * insertion sort on the order keys, which is stable. A short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SEGSORT_TILE 2048u
#define SEGSORT_ENDS_TILE 4096u

static size_t segsort_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }
static int segsort_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }
static int segsort_value_size_ok(int vs) { return vs == 0 || vs == 4 || vs == 8; }
/* CloType numbers (clo_common.h): char 0 .. ulong 7 in pairs of signed and unsigned, half 8, float 9, double 10 */
static int segsort_key_size(int t) { return t < 0 || t > 10 ? 0 : t == 8 ? 2 : t == 9 ? 4 : t == 10 ? 8 : 1 << (t >> 1); }
static int segsort_key_kind(int t) { return t >= 8 ? 2 : (t & 1) ? 0 : 1; }

size_t clo_hip_segsort_tile(int key_size, int value_size) {
	return segsort_key_size_ok(key_size) && segsort_value_size_ok(value_size) ? SEGSORT_TILE : 0;
}

size_t clo_hip_segsort_workspace_bytes(size_t numel_seg, size_t numel, int key_size, int value_size) {
	if (numel_seg == 0 && numel == 0) return 0;
	if (!segsort_key_size_ok(key_size) || !segsort_value_size_ok(value_size)) return 0;
	const size_t tiles = (numel + SEGSORT_TILE - 1) / SEGSORT_TILE;
	return segsort_align(numel_seg * 8) + segsort_align(((numel_seg + SEGSORT_ENDS_TILE - 1) / SEGSORT_ENDS_TILE + 1) * 8)
		+ segsort_align(tiles * SEGSORT_TILE) + segsort_align(tiles * 32) + segsort_align(numel * (size_t) key_size)
		+ (value_size == 4 ? segsort_align(numel * (size_t) key_size) : 0) + segsort_align(numel * (size_t) value_size);
}

static uint64_t segsort_word(const void* p, size_t i, int size) {
	uint64_t v = 0;
	memcpy(&v, (const char*) p + i * (size_t) size, (size_t) size);   /* little endian */
	return v;
}

/* the key as an unsigned number whose order is the sort's */
static uint64_t segsort_order(uint64_t x, int ks, int kind) {
	const uint64_t sign = 1ull << (8 * ks - 1), field = ks == 8 ? ~0ull : (1ull << (8 * ks)) - 1;
	if (kind == 1) return x ^ sign;
	if (kind == 2) return x ^ ((x & sign) ? field : sign);
	return x;
}

int clo_hip_segsort(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, uint64_t* num_out, size_t numel_seg, size_t numel, int key_type, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (form != CLO_HIP_SEGSORT_COUNTS && form != CLO_HIP_SEGSORT_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int ks = segsort_key_size(key_type), kind = segsort_key_kind(key_type);
	if (ks == 0 || !segsort_value_size_ok(value_size)) return CLO_HIP_EUNSUPPORTED;
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGSORT_OFFSETS)) return CLO_HIP_EARGS;
	if (!keys_in && numel > 0) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	if (value_size == 8 && !values_in) return CLO_HIP_EARGS;
	const int arg = value_size == 4 && !values_in;
	if (!keys_out && !arg) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8 || (uintptr_t) num_in % 8) return CLO_HIP_EARGS;
	if ((uintptr_t) counts_or_offsets % (size_t) count_size || (uintptr_t) keys_in % (size_t) ks || (uintptr_t) keys_out % (size_t) ks) return CLO_HIP_EARGS;
	if (value_size > 0 && ((uintptr_t) values_in % (size_t) value_size || (uintptr_t) values_out % (size_t) value_size)) return CLO_HIP_EARGS;
	if (numel_seg == 0) { *num_out = 0; return 0; }
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	const size_t need = clo_hip_segsort_workspace_bytes(numel_seg, numel, ks, value_size);
	if (workspace_bytes < need) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, need);   /* the kernels write it */

	const uint32_t m_h = (uint32_t) numel_seg;
	const uint32_t m = num_in && *num_in < m_h ? (uint32_t) *num_in : m_h;
	const uint64_t base = form == CLO_HIP_SEGSORT_OFFSETS ? segsort_word(counts_or_offsets, 0, count_size) : 0;
	uint64_t end = 0, from = 0;   /* the running end; the previous clipped end */
	for (uint32_t r = 0; r < m; ++r) {
		if (form == CLO_HIP_SEGSORT_OFFSETS) end = segsort_word(counts_or_offsets, (size_t) r + 1, count_size) - base;
		else end += segsort_word(counts_or_offsets, r, count_size);
		const uint64_t to = end < numel ? end : numel;
		/* rows [from, to): row i goes behind every earlier row that does not lie above it */
		for (uint64_t i = from; i < to; ++i) {
			const uint64_t key = segsort_word(keys_in, (size_t) i, ks), ok = segsort_order(key, ks, kind);
			uint64_t val = arg ? i : value_size ? segsort_word(values_in, (size_t) i, value_size) : 0;
			uint64_t at = i;
			for (; at > from; --at) {
				/* the key at at - 1: in keys_out, or (the arg form without it) the key of the row values_out names */
				const uint64_t before = keys_out ? segsort_word(keys_out, (size_t) at - 1, ks)
					: segsort_word(keys_in, (size_t) segsort_word(values_out, (size_t) at - 1, 4), ks);
				if (segsort_order(before, ks, kind) <= ok) break;
				if (keys_out) memcpy((char*) keys_out + (size_t) at * (size_t) ks, (const char*) keys_out + ((size_t) at - 1) * (size_t) ks, (size_t) ks);
				if (value_size) memcpy((char*) values_out + (size_t) at * (size_t) value_size, (const char*) values_out + ((size_t) at - 1) * (size_t) value_size, (size_t) value_size);
			}
			if (keys_out) memcpy((char*) keys_out + (size_t) at * (size_t) ks, &key, (size_t) ks);
			if (value_size) memcpy((char*) values_out + (size_t) at * (size_t) value_size, &val, (size_t) value_size);
		}
		if (to > from) from = to;
	}
	*num_out = end;
	return 0;
}
