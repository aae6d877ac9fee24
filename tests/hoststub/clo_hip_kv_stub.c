/*
 * clo_hip_kv_stub.c — TEST INFRASTRUCTURE, never part of the product: a host-memory version of the thin C-ABI's
 * key-value sort (clo_hip_radix_sort_kv, include/clo_hip.h), beside clo_hip_stub.c, so that the satradix driver's
 * by-key path (cl_ops_amd/csrc/clo_sort_satradix.c) links and runs on the CPU under the sanitizers
 * (tests/kv_host/kv_host_test.c, tests/test_sort_by_key_cpu.py). Serial C with the same contract: a stable sort of
 * the indices by the ordered key field, then the keys and values gathered in that order. The pair buffers are
 * scribbled over, as the device sort overwrites them.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

size_t clo_hip_radix_kv_workspace_bytes(size_t numel, int key_size, int key_bits, int digit_bits) {
	(void) numel;
	if (key_size != 1 && key_size != 2 && key_size != 4) return 0;
	return (digit_bits < 1 || digit_bits > 8 || key_bits < 1) ? 0 : 1024;
}

/* the ordered unsigned image of the key field [shift, shift + bits) of a key_size-byte element */
static uint32_t kv_ordered_key(const unsigned char* keys, size_t i, int key_size, int shift, int bits, int kind) {
	uint32_t e = 0;
	memcpy(&e, keys + i * (size_t) key_size, (size_t) key_size);   /* (little-endian host, as the device) */
	const uint32_t mask = bits >= 32 ? 0xffffffffu : ((1u << bits) - 1u);
	uint32_t k = (e >> shift) & mask;
	const uint32_t sign = 1u << (bits - 1);
	if (kind == 1) k ^= sign;
	else if (kind == 2) k = (k & sign) ? (~k & mask) : (k | sign);
	return k;
}

int clo_hip_radix_sort_kv(const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* pairs_a, void* pairs_b,
	size_t numel, int key_size, int key_shift, int key_bits, int key_kind, int digit_bits,
	void* workspace, size_t workspace_bytes, void* stream) {
	(void) stream;
	if (numel == 0) return 0;
	if (!keys_in || !values_out || !pairs_a || !pairs_b || pairs_a == pairs_b || !workspace) return CLO_HIP_EARGS;
	if (key_size != 1 && key_size != 2 && key_size != 4) return CLO_HIP_EUNSUPPORTED;
	if (key_bits < 1 || key_shift < 0 || key_shift + key_bits > 8 * key_size || key_kind < 0 || key_kind > 2) return CLO_HIP_EARGS;
	if (key_kind == 2 && key_bits != 16 && key_bits != 32) return CLO_HIP_EARGS;
	if (digit_bits < 1 || digit_bits > 8) return CLO_HIP_EUNSUPPORTED;
	if (numel > 0xffffffffull) return CLO_HIP_EARGS;
	if (workspace_bytes < clo_hip_radix_kv_workspace_bytes(numel, key_size, key_bits, digit_bits)) return CLO_HIP_EWORKSPACE;
	memset(pairs_a, 0xA5, numel * 8);
	memset(pairs_b, 0x5A, numel * 8);
	memset(workspace, 0, 512);

	const unsigned char* kin = (const unsigned char*) keys_in;
	uint32_t* key = (uint32_t*) malloc(numel * sizeof(uint32_t));
	uint32_t* idx = (uint32_t*) malloc(numel * sizeof(uint32_t));
	uint32_t* idx2 = (uint32_t*) malloc(numel * sizeof(uint32_t));
	unsigned char* ko = (unsigned char*) malloc(numel * (size_t) key_size);
	uint32_t* vo = (uint32_t*) malloc(numel * sizeof(uint32_t));
	int st = 0;
	if (!key || !idx || !idx2 || !ko || !vo) { st = 2; goto done; }
	for (size_t i = 0; i < numel; ++i) {
		key[i] = kv_ordered_key(kin, i, key_size, key_shift, key_bits, key_kind);
		idx[i] = (uint32_t) i;
	}
	for (int d = 0; d * 8 < key_bits; ++d) {   /* stable LSD byte-wise counting sort of the indices */
		size_t cnt[257];
		memset(cnt, 0, sizeof(cnt));
		for (size_t i = 0; i < numel; ++i) cnt[((key[idx[i]] >> (8 * d)) & 255u) + 1]++;
		for (int k = 0; k < 256; ++k) cnt[k + 1] += cnt[k];
		for (size_t i = 0; i < numel; ++i) idx2[cnt[(key[idx[i]] >> (8 * d)) & 255u]++] = idx[i];
		uint32_t* t = idx; idx = idx2; idx2 = t;
	}
	/* gathered into copies first: the output arrays may be the input arrays */
	for (size_t j = 0; j < numel; ++j) {
		memcpy(ko + j * (size_t) key_size, kin + (size_t) idx[j] * (size_t) key_size, (size_t) key_size);
		if (values_in) memcpy(&vo[j], (const unsigned char*) values_in + (size_t) idx[j] * 4, 4);
		else vo[j] = idx[j];
	}
	if (keys_out) memcpy(keys_out, ko, numel * (size_t) key_size);
	memcpy(values_out, vo, numel * 4);
done:
	free(key); free(idx); free(idx2); free(ko); free(vo);
	return st;
}
