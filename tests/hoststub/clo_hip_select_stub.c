/*
 * clo_hip_select_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * selection (clo_hip_select, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_select.c) links and runs on the CPU under the sanitizers (tests/select_host/select_host_test.c,
 * tests/test_select_cpu.py). Two serial walks over the elements with the same contract and the same status codes: the
 * kept ones, then for a partition the rejected ones. It reads flags[0, numel), keys[0, numel) and one threshold, and
 * writes rows [0, k) or [0, numel): a short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

static int select_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }
static int select_value_size_ok(int vs) { return vs == 0 || vs == 4 || vs == 8; }

size_t clo_hip_select_tile(int key_size, int value_size) {
	if (!select_key_size_ok(key_size) || !select_value_size_ok(value_size)) return 0;
	return (key_size > value_size ? key_size : value_size) <= 4 ? 8192 : 4096;
}

size_t clo_hip_select_workspace_bytes(size_t numel, int key_size, int value_size) {
	const size_t tile = clo_hip_select_tile(key_size, value_size);
	if (numel == 0 || tile == 0) return 0;
	const size_t bytes = ((numel - 1) / tile + 2) * sizeof(unsigned);
	return (bytes + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN;
}

/* element i of an array of ks-byte keys, mapped to unsigned order (little-endian host, as the device) */
static uint64_t select_key(const void* keys, size_t i, size_t ks, int kind) {
	uint64_t k = 0;
	memcpy(&k, (const char*) keys + i * ks, ks);
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	if (kind == 1) return k ^ sign;
	if (kind == 2) return (k & sign) ? k ^ all : k ^ sign;
	return k;
}

int clo_hip_select(int op, int pred, const void* keys_in, const void* values_in, const void* flags_or_threshold,
	void* keys_out, void* values_out, uint64_t* num_out, size_t numel, int key_size, int key_kind, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (op != CLO_HIP_SELECT_SELECT && op != CLO_HIP_SELECT_PARTITION) return CLO_HIP_EARGS;
	if (pred < CLO_HIP_SELECT_FLAGGED || pred > CLO_HIP_SELECT_NE) return CLO_HIP_EARGS;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!select_key_size_ok(key_size) || !select_value_size_ok(value_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!flags_or_threshold && (numel > 0 || pred != CLO_HIP_SELECT_FLAGGED)) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8) return CLO_HIP_EARGS;
	if (!keys_out && !values_out) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	const int arg = value_size > 0 && !values_in;
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	if (numel > 0 && !keys_in && (pred != CLO_HIP_SELECT_FLAGGED || keys_out)) return CLO_HIP_EARGS;
	const size_t ks = (size_t) key_size, vs = (size_t) value_size;
	if ((uintptr_t) keys_in % ks || (uintptr_t) keys_out % ks) return CLO_HIP_EARGS;
	if (pred != CLO_HIP_SELECT_FLAGGED && (uintptr_t) flags_or_threshold % ks) return CLO_HIP_EARGS;
	if (vs > 0 && ((uintptr_t) values_in % vs || (uintptr_t) values_out % vs)) return CLO_HIP_EARGS;
	if (numel > 0) {
		/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
		if (!workspace) return CLO_HIP_EARGS;
		if (workspace_bytes < clo_hip_select_workspace_bytes(numel, key_size, value_size)) return CLO_HIP_EWORKSPACE;
		memset(workspace, 0x5A, clo_hip_select_workspace_bytes(numel, key_size, value_size));   /* the kernels write it */
	}
	const uint64_t thr = pred == CLO_HIP_SELECT_FLAGGED ? 0 : select_key(flags_or_threshold, 0, ks, key_kind);
	size_t row = 0, k = 0;
	for (int side = 0; side < (op == CLO_HIP_SELECT_PARTITION ? 2 : 1); ++side) {   /* the kept rows, then the rejected ones */
		for (size_t i = 0; i < numel; ++i) {
			int keep;
			if (pred == CLO_HIP_SELECT_FLAGGED) keep = ((const unsigned char*) flags_or_threshold)[i] != 0;
			else {
				const uint64_t x = select_key(keys_in, i, ks, key_kind);
				keep = pred == CLO_HIP_SELECT_LT ? x < thr : pred == CLO_HIP_SELECT_LE ? x <= thr : pred == CLO_HIP_SELECT_GT ? x > thr
					: pred == CLO_HIP_SELECT_GE ? x >= thr : pred == CLO_HIP_SELECT_EQ ? x == thr : x != thr;
			}
			if (keep != (side == 0) || row >= numel) continue;
			if (keys_out) memcpy((char*) keys_out + row * ks, (const char*) keys_in + i * ks, ks);
			if (arg) {
				const uint32_t p = (uint32_t) i;
				memcpy((char*) values_out + row * 4, &p, 4);
			} else if (vs > 0) {
				memcpy((char*) values_out + row * vs, (const char*) values_in + i * vs, vs);
			}
			++row;
		}
		if (side == 0) k = row;
	}
	*num_out = k;
	return 0;
}
