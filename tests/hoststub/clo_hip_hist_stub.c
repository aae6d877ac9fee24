/*
 * clo_hip_hist_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * histogram (clo_hip_histogram, include/clo_hip.h), beside clo_hip_stub.c, so that the driver
 * (cl_ops_amd/csrc/clo_histogram.c) links and runs on the CPU under the sanitizers (tests/hist_host/hist_host_test.c,
 * tests/test_histogram_cpu.py). Serial C with the same contract and the same status codes.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <string.h>

#define HIST_STUB_TILE 4096u
#define HIST_STUB_LDS_BYTES 65536u

size_t clo_hip_histogram_tile(int key_size, int value_size) {
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return 0;
	if (value_size != 0 && value_size != 4 && value_size != 8) return 0;
	return HIST_STUB_TILE;
}

size_t clo_hip_histogram_lds_bins(int sum_size) {
	if (sum_size != 4 && sum_size != 8) return 0;
	return HIST_STUB_LDS_BYTES / (size_t) sum_size;
}

size_t clo_hip_histogram_workspace_bytes(size_t numel, size_t num_bins) {
	(void) numel; (void) num_bins;
	return 0;
}

/* CloType numbers (clo_common.h): int 4, uint 5, long 6, ulong 7 */
static int hist_int_type(int t) { return t >= 4 && t <= 7; }
static int hist_type_size(int t) { return t >= 6 ? 8 : 4; }

int clo_hip_histogram(const void* keys_in, const void* values_in, void* hist_out, size_t numel, int key_size, int key_signed,
	int value_type, int sum_type, uint64_t lower, unsigned shift, size_t num_bins, int accumulate, unsigned max_groups,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) max_groups; (void) workspace; (void) workspace_bytes; (void) stream;
	if (!hist_out || num_bins == 0 || num_bins > 0xffffffffull || numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (key_size != 1 && key_size != 2 && key_size != 4 && key_size != 8) return CLO_HIP_EUNSUPPORTED;
	if (shift >= 8u * (unsigned) key_size) return CLO_HIP_EARGS;
	if (!hist_int_type(sum_type)) return CLO_HIP_EUNSUPPORTED;
	if (values_in && (!hist_int_type(value_type) || hist_type_size(sum_type) < hist_type_size(value_type))) return CLO_HIP_EUNSUPPORTED;
	const size_t ks = (size_t) key_size, ss = (size_t) hist_type_size(sum_type);
	if ((uintptr_t) hist_out % ss) return CLO_HIP_EARGS;
	if (numel > 0 && !keys_in) return CLO_HIP_EARGS;
	if ((uintptr_t) keys_in % ks || (values_in && (uintptr_t) values_in % (size_t) hist_type_size(value_type))) return CLO_HIP_EARGS;
	if (!accumulate) memset(hist_out, 0, num_bins * ss);

	const uint64_t mask = key_size == 8 ? ~0ull : ((1ull << (8 * key_size)) - 1ull);
	const uint64_t flip = key_signed ? 1ull << (8 * key_size - 1) : 0ull;   /* signed keys compare as unsigned ones with the sign bit flipped */
	const uint64_t lo = (lower & mask) ^ flip;
	for (size_t i = 0; i < numel; ++i) {
		uint64_t k = 0;
		memcpy(&k, (const char*) keys_in + i * ks, ks);   /* (little-endian host, as the device) */
		k ^= flip;
		if (k < lo) continue;
		const uint64_t b = (k - lo) >> shift;
		if (b >= (uint64_t) num_bins) continue;
		int64_t x;
		if (!values_in) x = 1;
		else if (value_type == 4) { int32_t v; memcpy(&v, (const char*) values_in + i * 4, 4); x = v; }
		else if (value_type == 5) { uint32_t v; memcpy(&v, (const char*) values_in + i * 4, 4); x = (int64_t) v; }
		else memcpy(&x, (const char*) values_in + i * 8, 8);
		if (ss == 4) {
			uint32_t h;
			memcpy(&h, (char*) hist_out + b * 4, 4);
			h += (uint32_t) (uint64_t) x;
			memcpy((char*) hist_out + b * 4, &h, 4);
		} else {
			uint64_t h;
			memcpy(&h, (char*) hist_out + b * 8, 8);
			h += (uint64_t) x;
			memcpy((char*) hist_out + b * 8, &h, 8);
		}
	}
	return 0;
}
