/*
 * clo_hip_segtopk_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * segmented top-k (clo_hip_segtopk, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_segtopk.c) links and runs on the CPU under the sanitizers
 * (tests/segtopk_host/segtopk_host_test.c, tests/test_segtopk_cpu.py). One serial walk over the segments with the same
 * contract and the same status codes as the device code: m = min(numel_seg, *num_in), every end clipped to numel, a
 * segment's rows [previous clipped end, clipped end) — an end below its predecessor gives an empty range — inserted one
 * by one into a list of at most k (order key, row) pairs kept ascending, a row going behind every earlier one that does
 * not lie above it, which is stable. A short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SEGTOPK_TILE 2048u
#define SEGTOPK_K_MAX 1024u
#define SEGTOPK_ENDS_TILE 4096u

static size_t segtopk_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }
static int segtopk_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }
static int segtopk_value_size_ok(int vs) { return vs == 0 || vs == 4 || vs == 8; }
/* CloType numbers (clo_common.h): char 0 .. ulong 7 in pairs of signed and unsigned, half 8, float 9, double 10 */
static int segtopk_key_size(int t) { return t < 0 || t > 10 ? 0 : t == 8 ? 2 : t == 9 ? 4 : t == 10 ? 8 : 1 << (t >> 1); }
static int segtopk_key_kind(int t) { return t >= 8 ? 2 : (t & 1) ? 0 : 1; }

size_t clo_hip_segtopk_tile(int key_size, int value_size) {
	return segtopk_key_size_ok(key_size) && segtopk_value_size_ok(value_size) ? SEGTOPK_TILE : 0;
}

size_t clo_hip_segtopk_k_max(int key_size, int value_size) {
	return segtopk_key_size_ok(key_size) && segtopk_value_size_ok(value_size) ? SEGTOPK_K_MAX : 0;
}

size_t clo_hip_segtopk_workspace_bytes(size_t numel_seg, size_t numel, size_t k, int key_size, int value_size) {
	if (numel_seg == 0 && numel == 0) return 0;
	if (!segtopk_key_size_ok(key_size) || !segtopk_value_size_ok(value_size)) return 0;
	const size_t tiles = (numel + SEGTOPK_TILE - 1) / SEGTOPK_TILE;
	return segtopk_align(numel_seg * 8) + segtopk_align(((numel_seg + SEGTOPK_ENDS_TILE - 1) / SEGTOPK_ENDS_TILE + 1) * 8)
		+ segtopk_align(tiles * SEGTOPK_TILE) + segtopk_align(tiles * SEGTOPK_TILE * 4) + segtopk_align(tiles * 32)
		+ segtopk_align(tiles * 2 * k * (size_t) key_size) + segtopk_align(tiles * 2 * k * 4);
}

static uint64_t segtopk_word(const void* p, size_t i, int size) {
	uint64_t v = 0;
	memcpy(&v, (const char*) p + i * (size_t) size, (size_t) size);   /* little endian */
	return v;
}

/* the key as an unsigned number whose order is the sort's */
static uint64_t segtopk_order(uint64_t x, int ks, int kind) {
	const uint64_t sign = 1ull << (8 * ks - 1), field = ks == 8 ? ~0ull : (1ull << (8 * ks)) - 1;
	if (kind == 1) return x ^ sign;
	if (kind == 2) return x ^ ((x & sign) ? field : sign);
	return x;
}

int clo_hip_segtopk(int which, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, uint32_t* counts_out, uint64_t* num_out, size_t numel_seg, size_t numel, size_t k, int key_type, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (which != CLO_HIP_SEGTOPK_SMALLEST && which != CLO_HIP_SEGTOPK_LARGEST) return CLO_HIP_EARGS;
	if (form != CLO_HIP_SEGTOPK_COUNTS && form != CLO_HIP_SEGTOPK_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int ks = segtopk_key_size(key_type), kind = segtopk_key_kind(key_type);
	if (ks == 0 || !segtopk_value_size_ok(value_size)) return CLO_HIP_EUNSUPPORTED;
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (k > SEGTOPK_K_MAX || (unsigned long long) numel_seg * k > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGTOPK_OFFSETS)) return CLO_HIP_EARGS;
	if (!keys_in && numel > 0) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	if (value_size == 8 && !values_in) return CLO_HIP_EARGS;
	const int arg = value_size == 4 && !values_in;
	if (!keys_out && !arg) return CLO_HIP_EARGS;
	if (!counts_out && numel_seg > 0 && k > 0) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8 || (uintptr_t) num_in % 8 || (uintptr_t) counts_out % 4) return CLO_HIP_EARGS;
	if ((uintptr_t) counts_or_offsets % (size_t) count_size || (uintptr_t) keys_in % (size_t) ks || (uintptr_t) keys_out % (size_t) ks) return CLO_HIP_EARGS;
	if (value_size > 0 && ((uintptr_t) values_in % (size_t) value_size || (uintptr_t) values_out % (size_t) value_size)) return CLO_HIP_EARGS;
	if (numel_seg == 0) { *num_out = 0; return 0; }
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	const size_t need = clo_hip_segtopk_workspace_bytes(numel_seg, numel, k, ks, value_size);
	if (workspace_bytes < need) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, need);   /* the kernels write it */

	const uint32_t m_h = (uint32_t) numel_seg;
	const uint32_t m = num_in && *num_in < m_h ? (uint32_t) *num_in : m_h;
	const uint64_t base = form == CLO_HIP_SEGTOPK_OFFSETS ? segtopk_word(counts_or_offsets, 0, count_size) : 0;
	const uint64_t flip = which == CLO_HIP_SEGTOPK_LARGEST ? ~0ull : 0ull;
	uint64_t end = 0, from = 0;   /* the running end; the previous clipped end */
	uint64_t xs[SEGTOPK_K_MAX], rows[SEGTOPK_K_MAX];   /* the list of the segment at hand */
	for (uint32_t r = 0; r < m; ++r) {
		if (form == CLO_HIP_SEGTOPK_OFFSETS) end = segtopk_word(counts_or_offsets, (size_t) r + 1, count_size) - base;
		else end += segtopk_word(counts_or_offsets, r, count_size);
		const uint64_t to = end < numel ? end : numel;
		size_t have = 0;
		for (uint64_t i = from; i < to && k > 0; ++i) {
			const uint64_t x = segtopk_order(segtopk_word(keys_in, (size_t) i, ks), ks, kind) ^ flip;
			size_t at = have;
			while (at > 0 && xs[at - 1] > x) --at;   /* behind every earlier row that does not lie above it */
			if (at >= k) continue;
			const size_t last = have < k ? have : k - 1;
			for (size_t j = last; j > at; --j) { xs[j] = xs[j - 1]; rows[j] = rows[j - 1]; }
			xs[at] = x; rows[at] = i;
			if (have < k) ++have;
		}
		if (k > 0) {
			for (size_t j = 0; j < have; ++j) {
				const size_t o = (size_t) r * k + j;
				if (keys_out) memcpy((char*) keys_out + o * (size_t) ks, (const char*) keys_in + (size_t) rows[j] * (size_t) ks, (size_t) ks);
				if (arg) { const uint32_t idx = (uint32_t) rows[j]; memcpy((char*) values_out + o * 4, &idx, 4); }
				else if (value_size) memcpy((char*) values_out + o * (size_t) value_size, (const char*) values_in + (size_t) rows[j] * (size_t) value_size, (size_t) value_size);
			}
			counts_out[r] = (uint32_t) have;
		}
		if (to > from) from = to;
	}
	*num_out = end;
	return 0;
}
