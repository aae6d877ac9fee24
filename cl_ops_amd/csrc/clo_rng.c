/*
 * clo_rng.c — CloRng: device random number generators (reference: src/cl_ops/rng/clo_rng.c:57-412, restated)
 * and the bulk fill clo_rng_fill (new). The device code is include/clo_rng/clo_rng_device.hpp; the kernels that
 * seed and fill are reached through the thin C-ABI (clo_hip_rng_*, include/clo_hip.h).
 *
 * Every argument is checked before anything touches the device, so that the errors come back the same on a
 * context without one. Unlike upstream, err may be NULL everywhere.
 */
#include "clo_rng.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "clo_internal.h"

struct clo_rng {
	char* src;                 /* the selecting line + the device header's text */
	CCLBuffer* seeds_device;
	size_t size_in_device;     /* seeds_count * seed size */
	size_t seeds_count;
	int gen;                   /* index in clo_rng_infos */
	int owns_seeds;            /* 0 for CLO_RNG_SEED_EXT_DEV: the client's buffer */
};

/* clo_rng.c:60-68: name, source, seed size. `src` is the line that selects the generator in front of the device
 * header's text (upstream: the generator's own OpenCL source between the work-item and API sources). */
static const struct clo_rng_info infos[] = {
	{ "lcg", "#define CLO_RNG_LCG 1\n", 8 },
	{ "xorshift64", "#define CLO_RNG_XORSHIFT64 1\n", 8 },
	{ "xorshift128", "#define CLO_RNG_XORSHIFT128 1\n", 16 },
	{ "mwc64x", "#define CLO_RNG_MWC64X 1\n", 8 },
	{ "parkmiller", "#define CLO_RNG_PARKMILLER 1\n", 4 },
	{ "tauslcg", "#define CLO_RNG_TAUSLCG 1\n", 16 },
	{ NULL, NULL, 0 }
};

const struct clo_rng_info* clo_rng_get_infos(void) { return infos; }

/* ---- Mersenne Twister MT19937 (Matsumoto & Nishimura, 1998): init_genrand + genrand_int32, the stream of GLib's
 * g_rand_new_with_seed / g_rand_int that upstream's HOST_MT seeds come from (clo_rng.c:158-186) ---- */
#define MT_N 624
#define MT_M 397
typedef struct {
	uint32_t mt[MT_N];
	int mti;
} clo_mt;

static void clo_mt_seed(clo_mt* m, uint32_t seed) {
	m->mt[0] = seed;
	for (int i = 1; i < MT_N; ++i) m->mt[i] = 1812433253u * (m->mt[i - 1] ^ (m->mt[i - 1] >> 30)) + (uint32_t) i;
	m->mti = MT_N;
}

static uint32_t clo_mt_next(clo_mt* m) {
	if (m->mti >= MT_N) {
		for (int k = 0; k < MT_N; ++k) {
			const uint32_t y = (m->mt[k] & 0x80000000u) | (m->mt[(k + 1) % MT_N] & 0x7fffffffu);
			m->mt[k] = m->mt[(k + MT_M) % MT_N] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
		}
		m->mti = 0;
	}
	uint32_t y = m->mt[m->mti++];
	y ^= y >> 11;
	y ^= (y << 7) & 0x9d2c5680u;
	y ^= (y << 15) & 0xefc60000u;
	y ^= y >> 18;
	return y;
}

static char* concat2(const char* a, const char* b) {
	const size_t la = strlen(a), lb = strlen(b);
	char* s = (char*) malloc(la + lb + 1);
	if (!s) return NULL;
	memcpy(s, a, la);
	memcpy(s + la, b, lb + 1);
	return s;
}

/* DEV_GID: one init kernel over the states (clo_rng.c:100-155). */
static int device_seed_init(int gen, const char* hash, CCLBuffer* seeds, size_t seeds_count, cl_ulong main_seed,
	CCLQueue* cq, GError** err) {
	const int kind = (!hash || !*hash) ? 0 : !strcmp(hash, "KNUTH(x)") ? 1 : !strcmp(hash, "XS1(x)") ? 2 : -1;
	CCLEvent* evt = ccl_queue_begin_command(cq, "clo_rng_init", err);
	if (!evt) return 0;
	char* log = NULL;
	const int st = kind >= 0
		? clo_hip_rng_init(gen, ccl_buffer_get_device_ptr(seeds), seeds_count, main_seed, kind, ccl_queue_get_stream(cq))
		: clo_hip_rng_init_jit(gen, hash, ccl_buffer_get_device_ptr(seeds), seeds_count, main_seed, ccl_queue_get_stream(cq), &log);
	if (st != 0) {
		ccl_queue_abort_command(cq, evt);
		if (kind < 0 && st == CLO_HIP_EARGS)
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Could not build the seed hash '%s': %s%s%.400s", hash,
				clo_hip_error_string(st), log ? "\n" : "", log ? log : "");
		else
			clo_hip_failed(st, err, "clo_rng_init");
		free(log);
		return 0;
	}
	free(log);
	return ccl_queue_end_command(cq, evt, err) ? 1 : 0;
}

/* HOST_MT: seeds_count * seed_size / 4 draws, in memory order (clo_rng.c:158-213). */
static int host_seed_init(CCLBuffer* seeds, size_t bytes, cl_ulong main_seed, CCLQueue* cq, GError** err) {
	uint32_t* host = (uint32_t*) malloc(bytes);
	clo_mt* m = (clo_mt*) malloc(sizeof(clo_mt));
	if (!host || !m) {
		free(host);
		free(m);
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory for %zu bytes of seeds.", bytes);
		return 0;
	}
	clo_mt_seed(m, (uint32_t) main_seed);
	for (size_t i = 0; i < bytes / sizeof(uint32_t); ++i) host[i] = clo_mt_next(m);
	CCLEvent* evt = ccl_buffer_enqueue_write(seeds, cq, 1, 0, bytes, host, NULL, err);
	if (evt) ccl_event_set_name(evt, "CLO: write seeds");
	free(host);
	free(m);
	return evt != NULL;
}

CloRng* clo_rng_new(const char* type, CloRngSeedType seed_type, void* seeds, size_t seeds_count, cl_ulong main_seed,
	const char* hash, CCLContext* ctx, CCLQueue* cq, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);

	int gen = -1;
	for (int i = 0; type && infos[i].name; ++i)
		if (!strcmp(type, infos[i].name)) gen = i;
	if (gen < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_IMPL_NOT_FOUND, "The requested RNG implementation, '%s', was not found.",
			type ? type : "(null)");
		return NULL;
	}
	const size_t seed_size = infos[gen].seed_size;
	if (seeds_count == 0 || seeds_count > SIZE_MAX / seed_size) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The number of seeds must be between 1 and %zu.", SIZE_MAX / seed_size);
		return NULL;
	}
	const size_t bytes = seeds_count * seed_size;
	switch (seed_type) {
		case CLO_RNG_SEED_DEV_GID:
		case CLO_RNG_SEED_HOST_MT:
			if (seeds) {
				clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The %s seed type expects a NULL seeds parameter.",
					seed_type == CLO_RNG_SEED_DEV_GID ? "DEV_GID" : "HOST_MT");
				return NULL;
			}
			break;
		case CLO_RNG_SEED_EXT_HOST:
			if (!seeds) {
				clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The EXT_HOST seed type expects a non-NULL seeds parameter.");
				return NULL;
			}
			break;
		case CLO_RNG_SEED_EXT_DEV:
			if (!seeds) {
				clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The EXT_DEV seed type expects a device buffer as seeds parameter.");
				return NULL;
			}
			if (ccl_buffer_get_size((CCLBuffer*) seeds) < bytes) {
				clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The '%s' RNG type requires a buffer of at least %zu bytes. "
					"The size of the provided external device seeds buffer is only %zu bytes.",
					type, bytes, ccl_buffer_get_size((CCLBuffer*) seeds));
				return NULL;
			}
			break;
		default:
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown seed type.");
			return NULL;
	}
	if (seed_type != CLO_RNG_SEED_EXT_DEV && (!ctx || !cq)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A context and a queue are required for this seed type.");
		return NULL;
	}

	CloRng* rng = (CloRng*) calloc(1, sizeof(CloRng));
	if (rng) rng->src = concat2(infos[gen].src, clo_hip_rng_device_source());
	if (!rng || !rng->src) {
		if (rng) free(rng);
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	rng->gen = gen;
	rng->seeds_count = seeds_count;
	rng->size_in_device = bytes;

	if (seed_type == CLO_RNG_SEED_EXT_DEV) {
		rng->seeds_device = (CCLBuffer*) seeds;
		rng->owns_seeds = 0;
		return rng;
	}
	rng->seeds_device = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes, NULL, err);
	rng->owns_seeds = 1;
	int ok = rng->seeds_device != NULL;
	if (ok) {
		if (seed_type == CLO_RNG_SEED_DEV_GID)
			ok = device_seed_init(gen, hash, rng->seeds_device, seeds_count, main_seed, cq, err);
		else if (seed_type == CLO_RNG_SEED_HOST_MT)
			ok = host_seed_init(rng->seeds_device, bytes, main_seed, cq, err);
		else
			ok = ccl_buffer_enqueue_write(rng->seeds_device, cq, 1, 0, bytes, seeds, NULL, err) != NULL;
	}
	if (!ok) {
		clo_rng_destroy(rng);
		return NULL;
	}
	return rng;
}

void clo_rng_destroy(CloRng* rng) {
	clo_return_if_fail(rng != NULL);
	if (rng->owns_seeds) ccl_buffer_destroy(rng->seeds_device);
	free(rng->src);
	free(rng);
}

const char* clo_rng_get_source(CloRng* rng) {
	clo_return_val_if_fail(rng != NULL, NULL);
	return rng->src;
}

CCLBuffer* clo_rng_get_device_seeds(CloRng* rng) {
	clo_return_val_if_fail(rng != NULL, NULL);
	return rng->seeds_device;
}

size_t clo_rng_get_size(CloRng* rng) {
	clo_return_val_if_fail(rng != NULL, 0);
	return rng->size_in_device;
}

CCLEvent* clo_rng_fill(CloRng* rng, CCLQueue* cq, CCLBuffer* out, size_t numel, cl_uint bits, cl_uint maxint, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	if (!rng || !cq) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_rng_fill needs an RNG and a queue.");
		return NULL;
	}
	if (bits < 1 || bits > 32) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Number of bits must be between 1 and 32.");
		return NULL;
	}
	if (numel > 0 && (!out || numel > SIZE_MAX / sizeof(cl_uint) || ccl_buffer_get_size(out) < numel * sizeof(cl_uint))) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The output buffer must hold %zu numbers (%zu bytes), it has %zu bytes.",
			numel, numel * sizeof(cl_uint), out ? ccl_buffer_get_size(out) : (size_t) 0);
		return NULL;
	}
	CCLEvent* evt = ccl_queue_begin_command(cq, "clo_rng_fill", err);
	if (!evt) return NULL;
	const int st = clo_hip_rng_fill(rng->gen, ccl_buffer_get_device_ptr(rng->seeds_device), rng->seeds_count,
		numel ? (unsigned*) ccl_buffer_get_device_ptr(out) : NULL, numel, bits, maxint, 0, ccl_queue_get_stream(cq));
	if (clo_hip_failed(st, err, "clo_rng_fill")) {
		ccl_queue_abort_command(cq, evt);
		return NULL;
	}
	if (!ccl_queue_end_command(cq, evt, err)) return NULL;
	return evt;
}
