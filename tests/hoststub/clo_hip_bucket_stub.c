/*
 * clo_hip_bucket_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * multi-way partition (clo_hip_bucket, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_bucket.c) links and runs on the CPU under the sanitizers (tests/bucket_host/bucket_host_test.c,
 * tests/test_bucket_cpu.py). A serial counting sort with the same contract and the same status codes: one walk counts
 * the bins, one places the rows. It reads keys[0, numel) and values[0, numel) and writes rows [0, numel) and
 * offsets_out[0, num_bins]: a short buffer shows under ASan.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int bucket_key_size_ok(int ks) { return ks == 1 || ks == 2 || ks == 4 || ks == 8; }
static int bucket_value_size_ok(int vs) { return vs == 0 || vs == 4 || vs == 8; }
static size_t bucket_align(size_t x) { return (x + CLO_HIP_WORKSPACE_ALIGN - 1) / CLO_HIP_WORKSPACE_ALIGN * CLO_HIP_WORKSPACE_ALIGN; }

size_t clo_hip_bucket_tile(int key_size, int value_size) {
	if (!bucket_key_size_ok(key_size) || !bucket_value_size_ok(value_size)) return 0;
	return 4096;
}

size_t clo_hip_bucket_workspace_bytes(size_t numel, int key_size, int value_size, size_t num_bins) {
	if (numel == 0 || clo_hip_bucket_tile(key_size, value_size) == 0) return 0;
	const size_t counters = (numel + 4095) / 4096 * (num_bins + 1 > 256 ? 256 : num_bins + 1);
	size_t bytes = bucket_align(counters * 4) + bucket_align(counters * 8) + bucket_align(((counters + 4095) / 4096 + 1) * 8);
	if (num_bins + 1 > 256)
		bytes += bucket_align(numel * (size_t) key_size) + bucket_align(numel * (size_t) value_size) + bucket_align(num_bins * 4);
	return bytes;
}

/* the bin of element i, num_bins for the rest (little-endian host, as the device) */
static size_t bucket_bin(const void* keys, size_t i, size_t ks, int key_signed, uint64_t lower, unsigned shift, size_t num_bins) {
	uint64_t k = 0;
	memcpy(&k, (const char*) keys + i * ks, ks);
	const uint64_t all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull), flip = key_signed ? 1ull << (8 * ks - 1) : 0ull;
	const uint64_t x = (k ^ flip) & all, lo = (lower ^ flip) & all;
	if (x < lo) return num_bins;
	const uint64_t b = (x - lo) >> shift;
	return b < num_bins ? (size_t) b : num_bins;
}

int clo_hip_bucket(const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* offsets_out, size_t numel,
	int key_size, int key_signed, int value_size, int count_size, uint64_t lower, unsigned shift, size_t num_bins,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (!offsets_out || num_bins == 0 || num_bins > CLO_HIP_BUCKET_MAX_BINS || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (!bucket_key_size_ok(key_size) || !bucket_value_size_ok(value_size)) return CLO_HIP_EUNSUPPORTED;
	if (count_size != 4 && count_size != 8) return CLO_HIP_EUNSUPPORTED;
	if (shift >= 8u * (unsigned) key_size) return CLO_HIP_EARGS;
	if (value_size == 0 && (values_in || values_out)) return CLO_HIP_EARGS;
	if (value_size > 0 && !values_out) return CLO_HIP_EARGS;
	const int arg = value_size > 0 && !values_in;
	if (arg && value_size != 4) return CLO_HIP_EARGS;
	if (!keys_out && !arg) return CLO_HIP_EARGS;
	if (numel > 0 && !keys_in) return CLO_HIP_EARGS;
	const size_t ks = (size_t) key_size, vs = (size_t) value_size, cs = (size_t) count_size;
	if ((uintptr_t) keys_in % ks || (uintptr_t) keys_out % ks) return CLO_HIP_EARGS;
	if (vs > 0 && ((uintptr_t) values_in % vs || (uintptr_t) values_out % vs)) return CLO_HIP_EARGS;
	if ((uintptr_t) offsets_out % cs) return CLO_HIP_EARGS;
	if (numel > 0) {
		/* (the workspace comes from the stub allocator, malloc: its CLO_HIP_WORKSPACE_ALIGN rule cannot be checked here) */
		if (!workspace) return CLO_HIP_EARGS;
		if (workspace_bytes < clo_hip_bucket_workspace_bytes(numel, key_size, value_size, num_bins)) return CLO_HIP_EWORKSPACE;
		memset(workspace, 0x5A, clo_hip_bucket_workspace_bytes(numel, key_size, value_size, num_bins));   /* the kernels write it */
	}
	uint64_t* at = (uint64_t*) calloc(num_bins + 2, sizeof(uint64_t));   /* at[b + 1]: the rows of bin b, then where bin b's next row goes */
	if (!at) return CLO_HIP_EARGS;
	for (size_t i = 0; i < numel; ++i) ++at[bucket_bin(keys_in, i, ks, key_signed, lower, shift, num_bins) + 1];
	for (size_t b = 0; b <= num_bins; ++b) {
		at[b + 1] += at[b];
		if (cs == 8) ((uint64_t*) offsets_out)[b] = at[b];
		else ((uint32_t*) offsets_out)[b] = (uint32_t) at[b];
	}
	for (size_t i = 0; i < numel; ++i) {
		const size_t row = (size_t) at[bucket_bin(keys_in, i, ks, key_signed, lower, shift, num_bins)]++;
		if (keys_out) memcpy((char*) keys_out + row * ks, (const char*) keys_in + i * ks, ks);
		if (arg) {
			const uint32_t p = (uint32_t) i;
			memcpy((char*) values_out + row * 4, &p, 4);
		} else if (vs > 0) {
			memcpy((char*) values_out + row * vs, (const char*) values_in + i * vs, vs);
		}
	}
	free(at);
	return 0;
}
