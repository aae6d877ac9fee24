/*
 * clo_hip_rbk_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * reduce by key (clo_hip_reduce_by_key, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_reduce_by_key.c) links and runs on the CPU under the sanitizers (tests/rbk_host/rbk_host_test.c,
 * tests/test_reduce_by_key_cpu.py). Serial C with the same contract and the same status codes. The workspace is
 * scribbled over, as the device kernels overwrite it.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define RBK_STUB_TILE 4096u

size_t clo_hip_reduce_by_key_tile(int key_size, int value_size) {
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return 0;
	if (value_size != 0 && value_size != 4 && value_size != 8) return 0;
	return RBK_STUB_TILE;
}

size_t clo_hip_reduce_by_key_workspace_bytes(size_t numel) {
	return 256 + (numel / RBK_STUB_TILE + 1) * 16;
}

/* CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7 */
static int rbk_int_type(int t) { return t >= 4 && t <= 7; }
static int rbk_type_size(int t) { return t >= 6 ? 8 : 4; }

/* (sum type) value i, as the bits of a uint64 (the low 4 bytes for a 4-byte sum type) */
static uint64_t rbk_value(const void* values, size_t i, int value_type, int sum_type) {
	int64_t x;
	if (!values) x = 1;
	else if (value_type == 4) { int32_t v; memcpy(&v, (const char*) values + i * 4, 4); x = v; }
	else if (value_type == 5) { uint32_t v; memcpy(&v, (const char*) values + i * 4, 4); x = (int64_t) v; }
	else { memcpy(&x, (const char*) values + i * 8, 8); }
	const uint64_t bits = (uint64_t) x;
	return rbk_type_size(sum_type) == 4 ? (bits & 0xffffffffull) : bits;
}

/* a < b in the sum type */
static int rbk_less(uint64_t a, uint64_t b, int sum_type) {
	switch (sum_type) {
		case 4: return (int32_t) (uint32_t) a < (int32_t) (uint32_t) b;
		case 5: return (uint32_t) a < (uint32_t) b;
		case 6: return (int64_t) a < (int64_t) b;
		default: return a < b;
	}
}

int clo_hip_reduce_by_key(const void* keys_in, const void* values_in, void* keys_out, void* aggr_out, uint64_t* num_runs_dev,
	size_t numel, int key_size, int value_type, int sum_type, int op,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!num_runs_dev || ((uintptr_t) num_runs_dev & 7u)) return CLO_HIP_EARGS;
	if (!keys_out && !aggr_out) return CLO_HIP_EARGS;
	if (op < 0 || op > 2) return CLO_HIP_EARGS;
	if (aggr_out && !values_in && op != 0) return CLO_HIP_EARGS;
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return CLO_HIP_EUNSUPPORTED;
	if (aggr_out) {
		if (!rbk_int_type(sum_type)) return CLO_HIP_EUNSUPPORTED;
		if (values_in && (!rbk_int_type(value_type) || rbk_type_size(sum_type) < rbk_type_size(value_type))) return CLO_HIP_EUNSUPPORTED;
	}
	if (numel == 0) { *num_runs_dev = 0; return 0; }
	if (!keys_in || !workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_reduce_by_key_workspace_bytes(numel)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0xA5, clo_hip_reduce_by_key_workspace_bytes(numel));

	const unsigned char* kin = (const unsigned char*) keys_in;
	const size_t ks = (size_t) key_size, ss = (size_t) rbk_type_size(sum_type);
	uint64_t m = 0, acc = 0;
	for (size_t i = 0; i < numel; ++i) {
		const int head = i == 0 || memcmp(kin + i * ks, kin + (i - 1) * ks, ks) != 0;
		const uint64_t x = aggr_out ? rbk_value(values_in, i, value_type, sum_type) : 0;
		if (head) acc = x;
		else if (op == 0) acc += x;
		else if (op == 1) acc = rbk_less(x, acc, sum_type) ? x : acc;
		else acc = rbk_less(acc, x, sum_type) ? x : acc;
		if (i + 1 == numel || memcmp(kin + (i + 1) * ks, kin + i * ks, ks) != 0) {   /* the element ends a run: it writes the row */
			if (keys_out) memcpy((unsigned char*) keys_out + m * ks, kin + i * ks, ks);
			if (aggr_out) memcpy((unsigned char*) aggr_out + m * ss, &acc, ss);   /* (little-endian host, as the device) */
			++m;
		}
	}
	*num_runs_dev = m;
	return 0;
}
