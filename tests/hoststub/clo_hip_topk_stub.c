/*
 * clo_hip_topk_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * top-k (clo_hip_topk, include/clo_hip.h), beside clo_hip_stub.c, so that the driver (cl_ops_amd/csrc/clo_topk.c)
 * links and runs on the CPU under the sanitizers (tests/topk_host/topk_host_test.c, tests/test_topk_cpu.py). A qsort of
 * (order key or its complement, index) pairs with the same contract and the same status codes. It reads keys[0, numel)
 * and values[0, numel) and writes rows [0, m) and one key at kth_out: a short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TOPK_STUB_SORTED_MAX 4096

static int topk_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }
static int topk_value_size_ok(int vs) { return vs == 0 || vs == 4 || vs == 8; }

size_t clo_hip_topk_tile(int key_size, int value_size) {
	if (!topk_key_size_ok(key_size) || !topk_value_size_ok(value_size)) return 0;
	return (key_size > value_size ? key_size : value_size) <= 4 ? 8192 : 4096;
}

size_t clo_hip_topk_sweep_groups(void) { return 1024; }   /* 256 compute units, four groups each */

size_t clo_hip_topk_sorted_max(int key_size, int value_size) {
	if (!topk_key_size_ok(key_size) || !topk_value_size_ok(value_size)) return 0;
	return TOPK_STUB_SORTED_MAX;
}

size_t clo_hip_topk_workspace_bytes(size_t numel, int key_size, int value_size) {
	const size_t tile = clo_hip_topk_tile(key_size, value_size);
	if (numel == 0 || tile == 0) return 0;
	const size_t bytes = ((numel - 1) / tile + 2) * 2 * sizeof(unsigned);
	return 8192 + 256 + TOPK_STUB_SORTED_MAX * 8 + (bytes + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN;
}

typedef struct { uint64_t x; size_t i; } topk_pair;

static int topk_by_key(const void* a, const void* b) {
	const topk_pair* p = (const topk_pair*) a;
	const topk_pair* q = (const topk_pair*) b;
	if (p->x != q->x) return p->x < q->x ? -1 : 1;
	return p->i < q->i ? -1 : p->i > q->i;
}

static int topk_by_index(const void* a, const void* b) {
	const topk_pair* p = (const topk_pair*) a;
	const topk_pair* q = (const topk_pair*) b;
	return p->i < q->i ? -1 : p->i > q->i;
}

int clo_hip_topk(int which, int order, const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* kth_out,
	size_t numel, size_t k, int key_size, int key_kind, int value_size, void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (which != CLO_HIP_TOPK_SMALLEST && which != CLO_HIP_TOPK_LARGEST) return CLO_HIP_EARGS;
	if (order != CLO_HIP_TOPK_INPUT && order != CLO_HIP_TOPK_SORTED) return CLO_HIP_EARGS;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!topk_key_size_ok(key_size) || !topk_value_size_ok(value_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!keys_out && !values_out && !kth_out) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	const int arg = value_size > 0 && !values_in;
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	if (numel > 0 && !keys_in) return CLO_HIP_EARGS;
	const size_t ks = (size_t) key_size, vs = (size_t) value_size;
	if ((uintptr_t) keys_in % ks || (uintptr_t) keys_out % ks || (uintptr_t) kth_out % ks) return CLO_HIP_EARGS;
	if (vs > 0 && ((uintptr_t) values_in % vs || (uintptr_t) values_out % vs)) return CLO_HIP_EARGS;
	const size_t m = k < numel ? k : numel;
	if (order == CLO_HIP_TOPK_SORTED && m > TOPK_STUB_SORTED_MAX) return CLO_HIP_EARGS;
	if (m == 0) return 0;
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_topk_workspace_bytes(numel, key_size, value_size)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, clo_hip_topk_workspace_bytes(numel, key_size, value_size));   /* the kernels write it */

	topk_pair* pairs = (topk_pair*) malloc(numel * sizeof(topk_pair));
	if (!pairs) return CLO_HIP_EARGS;
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	for (size_t i = 0; i < numel; ++i) {
		uint64_t x = 0;
		memcpy(&x, (const char*) keys_in + i * ks, ks);   /* little-endian host, as the device */
		if (key_kind == 1) x ^= sign;
		else if (key_kind == 2) x = (x & sign) ? x ^ all : x ^ sign;
		pairs[i].x = which == CLO_HIP_TOPK_LARGEST ? x ^ all : x;
		pairs[i].i = i;
	}
	qsort(pairs, numel, sizeof(topk_pair), topk_by_key);
	if (kth_out) memcpy(kth_out, (const char*) keys_in + pairs[m - 1].i * ks, ks);
	if (order == CLO_HIP_TOPK_INPUT) qsort(pairs, m, sizeof(topk_pair), topk_by_index);
	for (size_t row = 0; row < m; ++row) {
		const size_t i = pairs[row].i;
		if (keys_out) memcpy((char*) keys_out + row * ks, (const char*) keys_in + i * ks, ks);
		if (arg) {
			const uint32_t p = (uint32_t) i;
			memcpy((char*) values_out + row * 4, &p, 4);
		} else if (vs > 0) {
			memcpy((char*) values_out + row * vs, (const char*) values_in + i * vs, vs);
		}
	}
	free(pairs);
	return 0;
}
