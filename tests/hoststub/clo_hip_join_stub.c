/*
 * clo_hip_join_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * equi-join (clo_hip_join, include/clo_hip.h), beside clo_hip_stub.c, so that the driver (cl_ops_amd/csrc/clo_join.c)
 * links and runs on the CPU under the sanitizers (tests/join_host/join_host_test.c, tests/test_join_cpu.py). A serial
 * walk over the groups of equal keys with the same contract and the same status codes. Like the kernels it stays inside
 * its arrays whatever the inputs hold: every step consumes at least one element that exists, every index written is
 * that of an element that exists, and nothing is written at or above the capacity.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define JOIN_STUB_TILE 2304u
#define JOIN_STUB_OUT_TILE 2048u

static int join_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }

size_t clo_hip_join_tile(int key_size) { return join_key_size_ok(key_size) ? JOIN_STUB_TILE : 0; }
size_t clo_hip_join_out_tile(void) { return JOIN_STUB_OUT_TILE; }

static size_t join_align(size_t bytes) { return (bytes + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }

size_t clo_hip_join_workspace_bytes(int kind, size_t numel_a, size_t numel_b) {
	const size_t n = numel_a + numel_b;
	if (n == 0 || n < numel_a || kind < CLO_HIP_JOIN_INNER || kind > CLO_HIP_JOIN_FULL) return 0;
	/* as the kernels' getter: split points, row offsets, emitter offsets, one entry per element, and a word per output
	 * tile that a join of these sizes can reach (the largest K, capped at the 2^32 rows a capacity can name) */
	const size_t t = (n + JOIN_STUB_TILE - 1) / JOIN_STUB_TILE;
	size_t prod = 0, alone = 0;
	if (numel_a > 0 && numel_b > 0) prod = numel_a > SIZE_MAX / numel_b ? SIZE_MAX : numel_a * numel_b;
	if (kind == CLO_HIP_JOIN_LEFT || kind == CLO_HIP_JOIN_FULL) alone += numel_a;
	if (kind == CLO_HIP_JOIN_RIGHT || kind == CLO_HIP_JOIN_FULL) alone = alone + numel_b < alone ? SIZE_MAX : alone + numel_b;
	const size_t k = prod > alone ? prod : alone, rows = k < 0xffffffffull ? k : 0xffffffffull;
	const size_t out_tiles = (rows + JOIN_STUB_OUT_TILE - 1) / JOIN_STUB_OUT_TILE;
	return join_align((t + 1) * 4) + join_align((t + 1) * 8) + join_align((t + 1) * 4) + join_align(n * 16) + join_align((out_tiles + 1) * 4);
}

/* element i of an array of ks-byte keys, mapped to unsigned order (little-endian host, as the device) */
static uint64_t join_key(const void* keys, size_t i, size_t ks, int kind) {
	uint64_t k = 0;
	memcpy(&k, (const char*) keys + i * ks, ks);
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	if (kind == 1) return k ^ sign;
	if (kind == 2) return (k & sign) ? k ^ all : k ^ sign;
	return k;
}

typedef struct {
	const char* keys[2]; uint32_t* ia; uint32_t* ib; char* keys_out; size_t ks, cap; uint64_t k;
} join_sink;

/* row (i, j), either of which may be CLO_HIP_JOIN_NONE, becomes output row k */
static void join_emit(join_sink* s, uint32_t i, uint32_t j) {
	if (s->k < s->cap) {
		if (s->ia) s->ia[s->k] = i;
		if (s->ib) s->ib[s->k] = j;
		if (s->keys_out) {
			if (i != CLO_HIP_JOIN_NONE) memcpy(s->keys_out + s->k * s->ks, s->keys[0] + (size_t) i * s->ks, s->ks);
			else memcpy(s->keys_out + s->k * s->ks, s->keys[1] + (size_t) j * s->ks, s->ks);
		}
	}
	++s->k;
}

int clo_hip_join(int kind, const void* keys_a, size_t numel_a, const void* keys_b, size_t numel_b,
	uint32_t* idx_a_out, uint32_t* idx_b_out, void* keys_out, size_t capacity, uint64_t* num_out, int key_size, int key_kind,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (kind < CLO_HIP_JOIN_INNER || kind > CLO_HIP_JOIN_FULL) return CLO_HIP_EARGS;
	if (key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (!join_key_size_ok(key_size) || (key_kind == 2 && key_size == 1)) return CLO_HIP_EUNSUPPORTED;
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull || capacity > 0xffffffffull) return CLO_HIP_EARGS;
	if ((numel_a > 0 && !keys_a) || (numel_b > 0 && !keys_b)) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8) return CLO_HIP_EARGS;
	if (capacity > 0 && !idx_a_out && !idx_b_out && !keys_out) return CLO_HIP_EARGS;
	const size_t ks = (size_t) key_size, n = numel_a + numel_b;
	if ((uintptr_t) keys_a % ks || (uintptr_t) keys_b % ks || (uintptr_t) keys_out % ks || (uintptr_t) idx_a_out % 4 || (uintptr_t) idx_b_out % 4)
		return CLO_HIP_EARGS;
	if (n > 0) {
		/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
		if (!workspace) return CLO_HIP_EARGS;
		if (workspace_bytes < clo_hip_join_workspace_bytes(kind, numel_a, numel_b)) return CLO_HIP_EWORKSPACE;
		memset(workspace, 0x5A, clo_hip_join_workspace_bytes(kind, numel_a, numel_b));   /* the kernels write it: a short buffer shows under ASan */
	}
	const int emits_a = kind == CLO_HIP_JOIN_LEFT || kind == CLO_HIP_JOIN_FULL, emits_b = kind == CLO_HIP_JOIN_RIGHT || kind == CLO_HIP_JOIN_FULL;

	join_sink s;
	s.keys[0] = (const char*) keys_a; s.keys[1] = (const char*) keys_b;
	s.ia = idx_a_out; s.ib = idx_b_out; s.keys_out = (char*) keys_out; s.ks = ks; s.cap = capacity; s.k = 0;
	size_t i = 0, j = 0;
	while (i < numel_a || j < numel_b) {
		/* the smallest key not yet consumed, its m copies at the front of A and its c copies at the front of B */
		uint64_t x;
		if (j >= numel_b) x = join_key(keys_a, i, ks, key_kind);
		else if (i >= numel_a) x = join_key(keys_b, j, ks, key_kind);
		else {
			const uint64_t a = join_key(keys_a, i, ks, key_kind), b = join_key(keys_b, j, ks, key_kind);
			x = a <= b ? a : b;
		}
		size_t m = 0, c = 0;
		while (i + m < numel_a && join_key(keys_a, i + m, ks, key_kind) == x) ++m;
		while (j + c < numel_b && join_key(keys_b, j + c, ks, key_kind) == x) ++c;
		if (m > 0 && c > 0) {
			if (s.k >= s.cap) s.k += (uint64_t) m * c;   /* only counted */
			else for (size_t r = 0; r < m; ++r)
				for (size_t q = 0; q < c; ++q) join_emit(&s, (uint32_t) (i + r), (uint32_t) (j + q));
		} else if (m > 0) {
			for (size_t r = 0; emits_a && r < m; ++r) join_emit(&s, (uint32_t) (i + r), CLO_HIP_JOIN_NONE);
		} else {
			for (size_t q = 0; emits_b && q < c; ++q) join_emit(&s, CLO_HIP_JOIN_NONE, (uint32_t) (j + q));
		}
		i += m;
		j += c;
	}
	*num_out = s.k;
	return 0;
}
