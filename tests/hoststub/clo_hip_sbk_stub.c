/*
 * clo_hip_sbk_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * scan by key (clo_hip_scan_by_key, include/clo_hip.h), beside clo_hip_stub.c and clo_hip_rbk_stub.c, so that the
 * driver (cl_ops_amd/csrc/clo_scan_by_key.c) links and runs on the CPU under the sanitizers
 * (tests/sbk_host/sbk_host_test.c, tests/test_scan_by_key_cpu.py). Serial C with the same contract and the same
 * status codes; `out` may be `values_in` (element i is read before it is written). The workspace is scribbled over,
 * as the device kernels overwrite it.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SBK_STUB_TILE 4096u

size_t clo_hip_scan_by_key_tile(int key_size, int value_size) {
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return 0;
	if (value_size != 0 && value_size != 4 && value_size != 8) return 0;
	return SBK_STUB_TILE;
}

size_t clo_hip_scan_by_key_workspace_bytes(size_t numel) {
	return 256 + (numel / SBK_STUB_TILE + 1) * 16;
}

/* CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7 */
static int sbk_int_type(int t) { return t >= 4 && t <= 7; }
static int sbk_type_size(int t) { return t >= 6 ? 8 : 4; }

/* (sum type) value i, as the bits of a uint64 (the low 4 bytes for a 4-byte sum type) */
static uint64_t sbk_value(const void* values, size_t i, int value_type, int sum_type) {
	int64_t x;
	if (!values) x = 1;
	else if (value_type == 4) { int32_t v; memcpy(&v, (const char*) values + i * 4, 4); x = v; }
	else if (value_type == 5) { uint32_t v; memcpy(&v, (const char*) values + i * 4, 4); x = (int64_t) v; }
	else { memcpy(&x, (const char*) values + i * 8, 8); }
	const uint64_t bits = (uint64_t) x;
	return sbk_type_size(sum_type) == 4 ? (bits & 0xffffffffull) : bits;
}

/* a < b in the sum type */
static int sbk_less(uint64_t a, uint64_t b, int sum_type) {
	switch (sum_type) {
		case 4: return (int32_t) (uint32_t) a < (int32_t) (uint32_t) b;
		case 5: return (uint32_t) a < (uint32_t) b;
		case 6: return (int64_t) a < (int64_t) b;
		default: return a < b;
	}
}

/* what an exclusive scan holds at a run's first element */
static uint64_t sbk_identity(int op, int sum_type) {
	if (op == 0) return 0;
	switch (sum_type) {
		case 4: return op == 1 ? 0x7fffffffull : 0x80000000ull;
		case 5: return op == 1 ? 0xffffffffull : 0;
		case 6: return op == 1 ? 0x7fffffffffffffffull : 0x8000000000000000ull;
		default: return op == 1 ? ~0ull : 0;
	}
}

int clo_hip_scan_by_key(const void* keys_in, const void* values_in, void* out, size_t numel,
	int key_size, int value_type, int sum_type, int op, int inclusive,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (op < 0 || op > 2) return CLO_HIP_EARGS;
	if (inclusive != 0 && inclusive != 1) return CLO_HIP_EARGS;
	if (!values_in && op != 0) return CLO_HIP_EARGS;
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return CLO_HIP_EUNSUPPORTED;
	if (!sbk_int_type(sum_type)) return CLO_HIP_EUNSUPPORTED;
	if (values_in && (!sbk_int_type(value_type) || sbk_type_size(sum_type) < sbk_type_size(value_type))) return CLO_HIP_EUNSUPPORTED;
	if (numel == 0) return 0;
	if (!keys_in || !out || !workspace) return CLO_HIP_EARGS;
	if ((uintptr_t) out % (size_t) sbk_type_size(sum_type)) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_scan_by_key_workspace_bytes(numel)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0xA5, clo_hip_scan_by_key_workspace_bytes(numel));

	const unsigned char* kin = (const unsigned char*) keys_in;
	const size_t ks = (size_t) key_size, ss = (size_t) sbk_type_size(sum_type);
	const uint64_t id = sbk_identity(op, sum_type);
	uint64_t acc = id;
	for (size_t i = 0; i < numel; ++i) {
		const int head = i == 0 || memcmp(kin + i * ks, kin + (i - 1) * ks, ks) != 0;
		const uint64_t x = sbk_value(values_in, i, value_type, sum_type);   /* read before out[i] is written: in place */
		const uint64_t before = head ? id : acc;
		if (head) acc = x;
		else if (op == 0) acc += x;
		else if (op == 1) acc = sbk_less(x, acc, sum_type) ? x : acc;
		else acc = sbk_less(acc, x, sum_type) ? x : acc;
		const uint64_t r = inclusive ? acc : before;
		memcpy((unsigned char*) out + i * ss, &r, ss);   /* (little-endian host, as the device) */
	}
	return 0;
}
