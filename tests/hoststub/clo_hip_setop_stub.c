/*
 * clo_hip_setop_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * set operations (clo_hip_setop, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_setop.c) links and runs on the CPU under the sanitizers (tests/setop_host/setop_host_test.c,
 * tests/test_setop_cpu.py). A serial walk over the groups of equal keys with the same contract and the same status
 * codes. Like the kernels it stays inside its arrays whatever the inputs hold: every step consumes at least one
 * element that exists, each element is written at most once, and nothing is written at or above the capacity.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SETOP_STUB_TILE 2304u

static int setop_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }
static int setop_value_size_ok(int vs) { return vs == 0 || vs == 4 || vs == 8; }

size_t clo_hip_setop_tile(int key_size, int value_size) {
	if (!setop_key_size_ok(key_size) || !setop_value_size_ok(value_size)) return 0;
	return SETOP_STUB_TILE;
}

size_t clo_hip_setop_workspace_bytes(size_t numel_a, size_t numel_b) {
	const size_t n = numel_a + numel_b;
	if (n == 0 || n < numel_a) return 0;
	const size_t bytes = (2 * ((n + SETOP_STUB_TILE - 1) / SETOP_STUB_TILE) + 1) * sizeof(unsigned);
	return (bytes + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN;
}

/* element i of an array of ks-byte keys, mapped to unsigned order (little-endian host, as the device) */
static uint64_t setop_key(const void* keys, size_t i, size_t ks, int kind) {
	uint64_t k = 0;
	memcpy(&k, (const char*) keys + i * ks, ks);
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	if (kind == 1) return k ^ sign;
	if (kind == 2) return (k & sign) ? k ^ all : k ^ sign;
	return k;
}

typedef struct {
	const char* keys[2]; const char* values[2]; size_t numel_a;
	char* keys_out; char* values_out; size_t ks, vs, cap, k; int arg;
} setop_sink;

/* element i of side (0: A, 1: B) becomes output row k */
static void setop_emit(setop_sink* s, int side, size_t i) {
	if (s->k >= s->cap) return;
	if (s->keys_out) memcpy(s->keys_out + s->k * s->ks, s->keys[side] + i * s->ks, s->ks);
	if (s->arg) {
		const uint32_t p = (uint32_t) (side ? s->numel_a + i : i);
		memcpy(s->values_out + s->k * 4, &p, 4);
	} else if (s->vs > 0) {
		memcpy(s->values_out + s->k * s->vs, s->values[side] + i * s->vs, s->vs);
	}
	++s->k;
}

int clo_hip_setop(int op, const void* keys_a, const void* values_a, size_t numel_a, const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, uint64_t* num_out, int key_size, int key_kind, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (op < CLO_HIP_SETOP_UNION || op > CLO_HIP_SETOP_SYMMETRIC_DIFFERENCE) return CLO_HIP_EARGS;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!setop_key_size_ok(key_size) || !setop_value_size_ok(value_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull) return CLO_HIP_EARGS;
	if ((numel_a > 0 && !keys_a) || (numel_b > 0 && !keys_b)) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8) return CLO_HIP_EARGS;
	if (!keys_out && !values_out) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_a || values_b || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	const int keeps_b = op == CLO_HIP_SETOP_UNION || op == CLO_HIP_SETOP_SYMMETRIC_DIFFERENCE;
	const int given_a = numel_a > 0 && values_a, given_b = keeps_b && numel_b > 0 && values_b;
	const int absent_a = numel_a > 0 && !values_a, absent_b = keeps_b && numel_b > 0 && !values_b;
	if ((given_a && absent_b) || (given_b && absent_a)) return CLO_HIP_EARGS;
	const int arg = value_size > 0 && (absent_a || absent_b);
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	const size_t ks = (size_t) key_size, vs = (size_t) value_size, n = numel_a + numel_b;
	if ((uintptr_t) keys_a % ks || (uintptr_t) keys_b % ks || (uintptr_t) keys_out % ks) return CLO_HIP_EARGS;
	if (vs > 0 && ((uintptr_t) values_a % vs || (uintptr_t) values_b % vs || (uintptr_t) values_out % vs)) return CLO_HIP_EARGS;
	if (n > 0) {
		/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
		if (!workspace) return CLO_HIP_EARGS;
		if (workspace_bytes < clo_hip_setop_workspace_bytes(numel_a, numel_b)) return CLO_HIP_EWORKSPACE;
		memset(workspace, 0x5A, clo_hip_setop_workspace_bytes(numel_a, numel_b));   /* the kernels write it: a short buffer shows under ASan */
	}

	setop_sink s;
	s.keys[0] = (const char*) keys_a; s.keys[1] = (const char*) keys_b;
	s.values[0] = (const char*) values_a; s.values[1] = (const char*) values_b;
	s.numel_a = numel_a; s.keys_out = (char*) keys_out; s.values_out = (char*) values_out;
	s.ks = ks; s.vs = vs; s.k = 0; s.arg = arg;
	s.cap = keeps_b ? n : op == CLO_HIP_SETOP_DIFFERENCE ? numel_a : (numel_a < numel_b ? numel_a : numel_b);
	size_t i = 0, j = 0;
	while (i < numel_a || j < numel_b) {
		/* the smallest key not yet consumed, its m copies at the front of A and its n copies at the front of B */
		uint64_t x;
		if (j >= numel_b) x = setop_key(keys_a, i, ks, key_kind);
		else if (i >= numel_a) x = setop_key(keys_b, j, ks, key_kind);
		else {
			const uint64_t a = setop_key(keys_a, i, ks, key_kind), b = setop_key(keys_b, j, ks, key_kind);
			x = a <= b ? a : b;
		}
		size_t m = 0, c = 0;
		while (i + m < numel_a && setop_key(keys_a, i + m, ks, key_kind) == x) ++m;
		while (j + c < numel_b && setop_key(keys_b, j + c, ks, key_kind) == x) ++c;
		for (size_t r = 0; r < m; ++r) {
			const int matched = r < c;
			if (op == CLO_HIP_SETOP_UNION || (op == CLO_HIP_SETOP_INTERSECTION ? matched : !matched)) setop_emit(&s, 0, i + r);
		}
		for (size_t q = 0; keeps_b && q < c; ++q)
			if (q >= m) setop_emit(&s, 1, j + q);
		i += m;
		j += c;
	}
	*num_out = s.k;
	return 0;
}
