/*
 * clo_hip_segarg_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * segmented arg-min and arg-max (clo_hip_segarg, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_segarg.c) links and runs on the CPU under the sanitizers
 * (tests/segarg_host/segarg_host_test.c, tests/test_segarg_cpu.py). One serial walk over the segments with the same
 * contract and the same status codes as the device code: m = min(numel_seg, *num_in), every end clipped to numel, a
 * segment's rows [max(previous clipped end, 0), clipped end) — an end below its predecessor gives an empty range — rows
 * [0, m) of idx_out and val_out written. A short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define SEGARG_TILE 4352u
#define SEGARG_CARRY_TILES 4096u
#define SEGARG_ENDS_TILE 4096u

static size_t segarg_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }
/* CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7, float 9, double 10 */
static int segarg_kind(int t) { return t == 5 || t == 7 ? 0 : t == 4 || t == 6 ? 1 : t == 9 || t == 10 ? 2 : -1; }
static int segarg_type_size(int t) { return t == 6 || t == 7 || t == 10 ? 8 : 4; }

size_t clo_hip_segarg_tile(int value_size) { return value_size == 4 || value_size == 8 ? SEGARG_TILE : 0; }

size_t clo_hip_segarg_carry_tiles(void) { return SEGARG_CARRY_TILES; }

size_t clo_hip_segarg_workspace_bytes(size_t numel_seg, size_t numel) {
	if (numel_seg == 0 && numel == 0) return 0;
	const size_t tiles = (numel_seg + numel + SEGARG_TILE - 1) / SEGARG_TILE;
	return segarg_align(numel_seg * 8) + segarg_align((tiles + 1) * 4) + 4 * segarg_align(tiles * 4) + 2 * segarg_align(tiles * 8)
		+ segarg_align(((numel_seg + SEGARG_ENDS_TILE - 1) / SEGARG_ENDS_TILE + 1) * 8);
}

static uint64_t segarg_word(const void* p, size_t i, int size) {
	if (size == 8) { uint64_t v; memcpy(&v, (const char*) p + i * 8, 8); return v; }
	uint32_t v;
	memcpy(&v, (const char*) p + i * 4, 4);
	return v;
}

int clo_hip_segarg(int op, int tie, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	uint32_t* idx_out, void* val_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (op != CLO_HIP_SEGARG_ARGMIN && op != CLO_HIP_SEGARG_ARGMAX) return CLO_HIP_EARGS;
	if (tie != CLO_HIP_SEGARG_FIRST && tie != CLO_HIP_SEGARG_LAST) return CLO_HIP_EARGS;
	if (form != CLO_HIP_SEGARG_COUNTS && form != CLO_HIP_SEGARG_OFFSETS) return CLO_HIP_EARGS;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	const int kind = segarg_kind(value_type);
	if (kind < 0) return CLO_HIP_EUNSUPPORTED;
	const int vs = segarg_type_size(value_type);
	if (numel_seg > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!counts_or_offsets && (numel_seg > 0 || form == CLO_HIP_SEGARG_OFFSETS)) return CLO_HIP_EARGS;
	if (!values_in && numel > 0) return CLO_HIP_EARGS;
	if (!idx_out && numel_seg > 0) return CLO_HIP_EARGS;
	if (!num_out || (uintptr_t) num_out % 8 || (uintptr_t) num_in % 8) return CLO_HIP_EARGS;
	if ((uintptr_t) counts_or_offsets % (size_t) count_size || (uintptr_t) values_in % (size_t) vs || (uintptr_t) idx_out % 4 || (uintptr_t) val_out % (size_t) vs)
		return CLO_HIP_EARGS;
	if (numel_seg == 0) { *num_out = 0; return 0; }
	/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
	if (!workspace) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_segarg_workspace_bytes(numel_seg, numel)) return CLO_HIP_EWORKSPACE;
	memset(workspace, 0x5A, clo_hip_segarg_workspace_bytes(numel_seg, numel));   /* the kernels write it */

	const uint32_t m_h = (uint32_t) numel_seg;
	const uint32_t m = num_in && *num_in < m_h ? (uint32_t) *num_in : m_h;
	const uint64_t sign = vs == 8 ? 1ull << 63 : 1ull << 31, mask = vs == 8 ? ~0ull : 0xffffffffull;
	const uint64_t cmpl = op == CLO_HIP_SEGARG_ARGMAX ? mask : 0;
	const uint64_t base = form == CLO_HIP_SEGARG_OFFSETS ? segarg_word(counts_or_offsets, 0, count_size) : 0;
	uint64_t end = 0, from = 0;   /* the running end; the previous clipped end */
	for (uint32_t r = 0; r < m; ++r) {
		if (form == CLO_HIP_SEGARG_OFFSETS) end = segarg_word(counts_or_offsets, (size_t) r + 1, count_size) - base;
		else end += segarg_word(counts_or_offsets, r, count_size);
		const uint64_t to = end < numel ? end : numel;
		uint64_t best = mask, best_bits = 0;
		uint32_t at = 0xffffffffu;
		for (uint64_t i = from; i < to; ++i) {
			const uint64_t bits = segarg_word(values_in, (size_t) i, vs);
			uint64_t x = kind == 0 ? bits : kind == 1 ? bits ^ sign : (bits & sign) ? ~bits & mask : bits ^ sign;
			x ^= cmpl;
			if (at == 0xffffffffu || x < best || (x == best && tie == CLO_HIP_SEGARG_LAST)) { best = x; best_bits = bits; at = (uint32_t) i; }
		}
		if (at == 0xffffffffu) {   /* no row: the value whose key is all ones */
			const uint64_t x = mask ^ cmpl;
			best_bits = kind == 0 ? x : kind == 1 ? x ^ sign : (x & sign) ? x ^ sign : ~x & mask;
		}
		idx_out[r] = at;
		if (val_out) {
			if (vs == 8) memcpy((char*) val_out + (size_t) r * 8, &best_bits, 8);
			else { const uint32_t b32 = (uint32_t) best_bits; memcpy((char*) val_out + (size_t) r * 4, &b32, 4); }
		}
		if (to > from) from = to;
	}
	*num_out = end;
	return 0;
}
