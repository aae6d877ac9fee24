/*
 * clo_hip_expand_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * expansion (clo_hip_expand, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_expand.c) links and runs on the CPU under the sanitizers (tests/expand_host/expand_host_test.c,
 * tests/test_expand_cpu.py). One serial walk over the rows with the same contract, the same status codes and the same
 * clamps as the device code: m = min(numel_in, *num_in), the segment of a row found by a halving whose trip count comes
 * from numel_in and that reads ends at indices below numel_in only, every segment id clamped to numel_in - 1, rows
 * [0, min(total, capacity)) written. A short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define EXPAND_TILE 4096u
#define EXPAND_LDS_SEGMENTS (4u * EXPAND_TILE)
#define EXPAND_ENDS_TILE 4096u

static int expand_value_size_ok(int vs) { return vs == 0 || vs == 1 || vs == 2 || vs == 4 || vs == 8; }
static size_t expand_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }

size_t clo_hip_expand_tile(int value_size) { return expand_value_size_ok(value_size) ? EXPAND_TILE : 0; }
size_t clo_hip_expand_lds_segments(void) { return EXPAND_LDS_SEGMENTS; }

size_t clo_hip_expand_workspace_bytes(size_t numel_in, size_t capacity) {
	if (numel_in == 0 && capacity == 0) return 0;
	return expand_align(numel_in * 8) + expand_align(((capacity + EXPAND_TILE - 1) / EXPAND_TILE + 1) * 4)
		+ expand_align(((numel_in + EXPAND_ENDS_TILE - 1) / EXPAND_ENDS_TILE + 1) * 8);
}

typedef struct { const void* src; const uint64_t* ends; int count_size, offsets; uint64_t base; } expand_ends;

static uint64_t expand_word(const void* p, size_t i, int size) {
	if (size == 8) { uint64_t v; memcpy(&v, (const char*) p + i * 8, 8); return v; }
	uint32_t v;
	memcpy(&v, (const char*) p + i * 4, 4);
	return v;
}

static uint64_t expand_end_at(const expand_ends* e, size_t r) {   /* r < numel_in */
	return e->offsets ? expand_word(e->src, r + 1, e->count_size) - e->base : e->ends[r];
}

/* how many of the ends [0, n) are <= x: the device's halving, its trip count from nmax = numel_in, loads at <= last */
static uint32_t expand_halve(const expand_ends* e, uint32_t n, uint64_t x, uint32_t nmax, uint32_t last) {
	uint32_t base = 0;
	for (uint32_t trips = nmax; trips > 1u; trips -= trips >> 1) {
		const uint32_t half = n > 1u ? n >> 1 : 0u;
		uint32_t at = base + (n >> 1) - (n > 1u ? 1u : 0u);
		if (at > last) at = last;
		if (expand_end_at(e, at) <= x) base += half;
		n -= half;
	}
	if (n == 1u && expand_end_at(e, base < last ? base : last) <= x) ++base;
	return base;
}

int clo_hip_expand(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* values_out, void* seg_out, void* rank_out, uint64_t* num_out, size_t numel_in, size_t capacity, int value_size,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (form != CLO_HIP_EXPAND_COUNTS && form != CLO_HIP_EXPAND_OFFSETS) return CLO_HIP_EARGS;
	if ((count_size != 4 && count_size != 8) || !expand_value_size_ok(value_size)) return CLO_HIP_EUNSUPPORTED;
	if (numel_in > 0xffffffffull || capacity > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_in > 0 || (form == CLO_HIP_EXPAND_OFFSETS && capacity > 0))) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8 || (uintptr_t) num_in % 8) return CLO_HIP_EARGS;
	if (!values_out && !seg_out && !rank_out) return CLO_HIP_EARGS;
	if ((values_in != NULL) != (values_out != NULL)) return CLO_HIP_EARGS;
	if (values_in && value_size == 0) return CLO_HIP_EARGS;
	if ((uintptr_t) counts_or_offsets % (size_t) count_size || (uintptr_t) seg_out % 4 || (uintptr_t) rank_out % 4) return CLO_HIP_EARGS;
	if (values_in && ((uintptr_t) values_in % (size_t) value_size || (uintptr_t) values_out % (size_t) value_size)) return CLO_HIP_EARGS;
	if (numel_in == 0) { *num_out = 0; return 0; }
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_expand_workspace_bytes(numel_in, capacity)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, clo_hip_expand_workspace_bytes(numel_in, capacity));   /* the kernels write it */

	const uint32_t m_h = (uint32_t) numel_in, last = m_h - 1u;
	const uint32_t m = num_in && *num_in < m_h ? (uint32_t) *num_in : m_h;
	expand_ends e = { counts_or_offsets, (const uint64_t*) workspace, count_size, form == CLO_HIP_EXPAND_OFFSETS, 0 };
	if (e.offsets) {
		e.base = expand_word(counts_or_offsets, 0, count_size);
	} else {
		uint64_t* ends = (uint64_t*) workspace;   /* its first numel_in words, as on the device; entries at r >= m add 0 */
		uint64_t run = 0;
		for (size_t r = 0; r < numel_in; ++r) {
			if (r < m) run += expand_word(counts_or_offsets, r, count_size);
			ends[r] = run;
		}
	}
	const uint64_t total = m > 0 ? expand_end_at(&e, m - 1u) : 0;
	*num_out = total;
	const size_t vs = (size_t) value_size;
	const uint64_t rows = total < capacity ? total : capacity;
	for (uint64_t j = 0; j < rows; ++j) {
		const uint32_t found = expand_halve(&e, m, j, m_h, last);
		const uint32_t r = found < last ? found : last;
		const uint64_t start = found > 0 ? expand_end_at(&e, (found - 1u) < last ? found - 1u : last) : 0;
		const uint32_t rank = (uint32_t) (j - start);
		if (values_out) memcpy((char*) values_out + j * vs, (const char*) values_in + (size_t) r * vs, vs);
		if (seg_out) memcpy((char*) seg_out + j * 4, &r, 4);
		if (rank_out) memcpy((char*) rank_out + j * 4, &rank, 4);
	}
	return 0;
}
