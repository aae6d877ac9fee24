/*
 * clo_hip_rng_stub.c — TEST INFRASTRUCTURE, never part of the product: host-memory versions of the thin C-ABI's
 * clo_hip_rng_* entry points (include/clo_hip.h), beside clo_hip_stub.c, so that the CloRng driver
 * (cl_ops_amd/csrc/clo_rng.c) runs on the CPU under the sanitizers (tests/rng_host/rng_host_test.c,
 * tests/test_rng_cpu.py). Serial C with the same contract and the same arithmetic as the device header
 * (include/clo_rng/clo_rng_device.hpp). There is no run-time compiler here: a hash other than the built-in ones
 * fails the way a hash that does not compile fails, with a log the caller frees.
 */
#include "clo_hip.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

const char* clo_hip_rng_device_source(void) { return "/* host stub: no device source */\n"; }

static const size_t stub_seed_size[6] = { 8, 8, 16, 8, 4, 16 };

static void stub_from_ulong(int gen, uint64_t seed, void* st) {
	uint32_t* w = (uint32_t*) st;
	switch (gen) {
		case 0: case 1: memcpy(st, &seed, 8); break;
		case 2: w[0] = (uint32_t) seed; w[1] = (uint32_t) (seed >> 16); w[2] = (uint32_t) (seed >> 32); w[3] = (uint32_t) (seed >> 46); break;
		case 3: w[0] = (uint32_t) seed; w[1] = (uint32_t) (seed >> 32); break;
		case 4: w[0] = (uint32_t) seed; break;
		default: w[0] = (uint32_t) seed; w[1] = (uint32_t) (seed >> 32); w[2] = w[0]; w[3] = w[1]; break;
	}
}

static uint32_t taus(uint32_t z, int s1, int s2, int s3, uint32_t m) { return ((z & m) << s3) ^ (((z << s1) ^ z) >> s2); }

static uint32_t stub_next(int gen, void* st) {
	uint32_t* w = (uint32_t*) st;
	uint64_t s;
	switch (gen) {
		case 0:
			memcpy(&s, st, 8);
			s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
			memcpy(st, &s, 8);
			return (uint32_t) (s >> 16);
		case 1:
			memcpy(&s, st, 8);
			s ^= s << 21; s ^= s >> 35; s ^= s << 4;
			memcpy(st, &s, 8);
			return (uint32_t) s;
		case 2: {
			const uint32_t t = w[0] ^ (w[0] << 11);
			w[0] = w[1]; w[1] = w[2]; w[2] = w[3];
			w[3] = w[3] ^ (w[3] >> 19) ^ (t ^ (t >> 8));
			return w[3];
		}
		case 3: {
			const uint32_t x = w[0], c = w[1], res = x ^ c;
			const uint32_t hi = (uint32_t) (((uint64_t) x * 4294883355u) >> 32);
			w[0] = x * 4294883355u + c;
			w[1] = hi + (w[0] < c);
			return res;
		}
		case 4: {
			int32_t v;
			memcpy(&v, st, 4);
			v = (int32_t) (((int64_t) v * 16807) % 2147483647);
			memcpy(st, &v, 4);
			return (uint32_t) v << 1;
		}
		default: {
			const uint32_t x = w[0];
			w[0] = taus(w[1], 13, 19, 12, 4294967294u);
			w[1] = taus(w[2], 2, 25, 4, 4294967288u);
			w[2] = taus(w[3], 3, 11, 17, 4294967294u);
			w[3] = 1664525u * x + 1013904223u;
			return w[0];
		}
	}
}

int clo_hip_rng_init(int gen, void* states, size_t count, uint64_t main_seed, int hash, void* stream) {
	(void) stream;
	if (count == 0) return 0;
	if (gen < 0 || gen > 5 || !states || hash < 0 || hash > 2) return CLO_HIP_EARGS;
	for (size_t g = 0; g < count; ++g) {
		uint64_t x = (uint64_t) g + main_seed;
		if (hash == 1) x = (x * 2654435761ULL) % 0x100000000ULL;
		if (hash == 2) {
			x = ((x >> 16) ^ x) * 0x45d9f3b;
			x = ((x >> 16) ^ x) * 0x45d9f3b;
			x = (x >> 16) ^ x;
		}
		stub_from_ulong(gen, x, (char*) states + g * stub_seed_size[gen]);
	}
	return 0;
}

int clo_hip_rng_init_jit(int gen, const char* hash, void* states, size_t count, uint64_t main_seed, void* stream, char** log) {
	(void) gen; (void) hash; (void) states; (void) count; (void) main_seed; (void) stream;
	static const char text[] = "host stub: no run-time compiler";
	if (log) {
		*log = (char*) malloc(sizeof(text));
		if (*log) memcpy(*log, text, sizeof(text));
	}
	return CLO_HIP_EARGS;
}

int clo_hip_rng_fill(int gen, void* states, size_t count, unsigned* out, size_t numel, unsigned bits, unsigned maxint,
	int layout, void* stream) {
	(void) stream;
	if (numel == 0) return 0;
	if (gen < 0 || gen > 5 || !states || !out || count == 0 || bits < 1 || bits > 32) return CLO_HIP_EARGS;
	if (layout != 0 && layout != 1 && layout != 4) return CLO_HIP_EARGS;
	for (size_t i = 0; i < numel; ++i) {   /* draw order: i = d * count + s, draws of one state in order */
		const uint32_t x = stub_next(gen, (char*) states + (i % count) * stub_seed_size[gen]);
		out[i] = maxint ? x % maxint : x >> (32 - bits);
	}
	return 0;
}
