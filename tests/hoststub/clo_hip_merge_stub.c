/*
 * clo_hip_merge_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * merge (clo_hip_merge, include/clo_hip.h), beside clo_hip_stub.c, so that the driver (cl_ops_amd/csrc/clo_merge.c)
 * links and runs on the CPU under the sanitizers (tests/merge_host/merge_host_test.c, tests/test_merge_cpu.py). A
 * serial two-pointer merge with the same contract and the same status codes. Like the kernels it stays inside its
 * arrays whatever the inputs hold: every step takes one element that exists.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define MERGE_STUB_TILE 2304u

static int merge_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }
static int merge_value_size_ok(int vs) { return vs == 0 || vs == 4 || vs == 8; }

size_t clo_hip_merge_tile(int key_size, int value_size) {
	if (!merge_key_size_ok(key_size) || !merge_value_size_ok(value_size)) return 0;
	return MERGE_STUB_TILE;
}

size_t clo_hip_merge_workspace_bytes(size_t numel_a, size_t numel_b) {
	const size_t n = numel_a + numel_b;
	if (n == 0 || n < numel_a) return 0;
	const size_t bytes = ((n + MERGE_STUB_TILE - 1) / MERGE_STUB_TILE + 1) * sizeof(unsigned);
	return (bytes + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN;
}

/* element i of an array of ks-byte keys, mapped to unsigned order (little-endian host, as the device) */
static uint64_t merge_key(const void* keys, size_t i, size_t ks, int kind) {
	uint64_t k = 0;
	memcpy(&k, (const char*) keys + i * ks, ks);
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	if (kind == 1) return k ^ sign;
	if (kind == 2) return (k & sign) ? k ^ all : k ^ sign;
	return k;
}

int clo_hip_merge(const void* keys_a, const void* values_a, size_t numel_a, const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, int key_size, int key_kind, int value_size, void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!merge_key_size_ok(key_size) || !merge_value_size_ok(value_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull) return CLO_HIP_EARGS;
	if ((numel_a > 0 && !keys_a) || (numel_b > 0 && !keys_b)) return CLO_HIP_EARGS;
	if (!keys_out && !values_out) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_a || values_b || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	const int given_a = numel_a > 0 && values_a, given_b = numel_b > 0 && values_b;
	const int absent_a = numel_a > 0 && !values_a, absent_b = numel_b > 0 && !values_b;
	if ((given_a && absent_b) || (given_b && absent_a)) return CLO_HIP_EARGS;
	const int arg = value_size > 0 && (absent_a || absent_b);
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	const size_t ks = (size_t) key_size, vs = (size_t) value_size;
	if ((uintptr_t) keys_a % ks || (uintptr_t) keys_b % ks || (uintptr_t) keys_out % ks) return CLO_HIP_EARGS;
	if (vs > 0 && ((uintptr_t) values_a % vs || (uintptr_t) values_b % vs || (uintptr_t) values_out % vs)) return CLO_HIP_EARGS;
	if (numel_a + numel_b == 0) return 0;
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_merge_workspace_bytes(numel_a, numel_b)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, clo_hip_merge_workspace_bytes(numel_a, numel_b));   /* the kernels write it: a short buffer shows under ASan */

	size_t i = 0, j = 0;
	for (size_t o = 0; o < numel_a + numel_b; ++o) {
		/* stable: from A while a <= b */
		const int from_a = j >= numel_b || (i < numel_a && merge_key(keys_a, i, ks, key_kind) <= merge_key(keys_b, j, ks, key_kind));
		if (keys_out) memcpy((char*) keys_out + o * ks, from_a ? (const char*) keys_a + i * ks : (const char*) keys_b + j * ks, ks);
		if (arg) {
			const uint32_t p = (uint32_t) (from_a ? i : numel_a + j);
			memcpy((char*) values_out + o * 4, &p, 4);
		} else if (vs > 0) {
			memcpy((char*) values_out + o * vs, from_a ? (const char*) values_a + i * vs : (const char*) values_b + j * vs, vs);
		}
		if (from_a) ++i; else ++j;
	}
	return 0;
}
