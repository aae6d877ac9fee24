/*
 * clo_hip_search_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * search (clo_hip_search, include/clo_hip.h), beside clo_hip_stub.c, so that the driver (cl_ops_amd/csrc/clo_search.c)
 * links and runs on the CPU under the sanitizers (tests/search_host/search_host_test.c, tests/test_search_cpu.py). A
 * serial binary search per needle, tile by tile, with the same contract and the same status codes. Like the kernels it
 * stays inside its arrays whatever the inputs hold: a search only reads indices of [0, numel_h), and the last tile is
 * clamped to the needles that exist.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SEARCH_STUB_TILE 1024u
#define SEARCH_STUB_LDS_KEYS 4096u
#define SEARCH_STUB_PIVOTS 1024u

static int search_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }

size_t clo_hip_search_tile(int key_size) { return search_key_size_ok(key_size) ? SEARCH_STUB_TILE : 0; }
size_t clo_hip_search_lds_keys(int key_size) { return search_key_size_ok(key_size) ? SEARCH_STUB_LDS_KEYS : 0; }
size_t clo_hip_search_pivots(int key_size) { return search_key_size_ok(key_size) ? SEARCH_STUB_PIVOTS : 0; }

size_t clo_hip_search_workspace_bytes(size_t numel_h, size_t numel_n, unsigned flags) {
	if (!(flags & CLO_HIP_SEARCH_NEEDLES_SORTED) || numel_h == 0 || numel_n == 0) return 0;
	const size_t bytes = ((numel_n + SEARCH_STUB_TILE - 1) / SEARCH_STUB_TILE) * 2 * sizeof(unsigned);
	return (bytes + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN;
}

/* element i of an array of ks-byte keys, mapped to unsigned order (little-endian host, as the device) */
static uint64_t search_key(const void* keys, size_t i, size_t ks, int kind) {
	uint64_t k = 0;
	memcpy(&k, (const char*) keys + i * ks, ks);
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	if (kind == 1) return k ^ sign;
	if (kind == 2) return (k & sign) ? k ^ all : k ^ sign;
	return k;
}

int clo_hip_search(const void* haystack, size_t numel_h, const void* needles, size_t numel_n, void* pos_out,
	int key_size, int key_kind, unsigned flags, unsigned max_groups, void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream; (void) max_groups;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!search_key_size_ok(key_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (flags & ~(CLO_HIP_SEARCH_UPPER | CLO_HIP_SEARCH_NEEDLES_SORTED)) return CLO_HIP_EARGS;
	if (numel_h > 0xffffffffull || numel_n > 0xffffffffull) return CLO_HIP_EARGS;
	if (numel_h > 0 && !haystack) return CLO_HIP_EARGS;
	if (numel_n > 0 && (!needles || !pos_out)) return CLO_HIP_EARGS;
	const size_t ks = (size_t) key_size;
	if ((numel_h > 0 && (uintptr_t) haystack % ks) || (uintptr_t) needles % ks || (uintptr_t) pos_out % sizeof(unsigned)) return CLO_HIP_EARGS;
	if (numel_n == 0) return 0;
	const size_t need = clo_hip_search_workspace_bytes(numel_h, numel_n, flags);
	if (need > 0) {
		/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
		if (!workspace) return CLO_HIP_EARGS;
		if (workspace_bytes < need) return CLO_HIP_EWORKSPACE;
		memset(workspace, 0x5A, need);   /* the kernels write it: a short buffer shows under ASan */
	}

	const int upper = (flags & CLO_HIP_SEARCH_UPPER) != 0;
	const size_t tiles = (numel_n + SEARCH_STUB_TILE - 1) / SEARCH_STUB_TILE;
	for (size_t t = 0; t < tiles; ++t) {
		const size_t n0 = t * SEARCH_STUB_TILE;
		const size_t cnt = numel_n - n0 < SEARCH_STUB_TILE ? numel_n - n0 : SEARCH_STUB_TILE;   /* the clamp of the last partial tile */
		for (size_t j = n0; j < n0 + cnt; ++j) {
			const uint64_t x = search_key(needles, j, ks, key_kind);
			size_t lo = 0, hi = numel_h;
			while (lo < hi) {
				const size_t mid = lo + (hi - lo) / 2;
				const uint64_t y = search_key(haystack, mid, ks, key_kind);
				if (upper ? y <= x : y < x) lo = mid + 1; else hi = mid;
			}
			const uint32_t p = (uint32_t) lo;
			memcpy((char*) pos_out + j * 4, &p, 4);
		}
	}
	return 0;
}
