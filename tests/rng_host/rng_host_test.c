/*
 * rng_host_test.c — the CloRng driver (cl_ops_amd/csrc/clo_rng.c) on the CPU, over the host stub of the thin
 * C-ABI (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_rng_cpu.py): every seed type, every
 * error path, EXT_DEV ownership, destroy, and fills whose values are checked against known answers and against a
 * draw-by-draw restatement of the fill's index rule.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cl_ops.h"

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); ++failures; } } while (0)

/* expects an error of `code` in err (or none with code 0), and frees it */
static void expect(GError** err, int code, const char* what) {
	if (code == 0) {
		CHECK(*err == NULL, "%s: unexpected error %s", what, *err ? (*err)->message : "");
	} else {
		CHECK(*err != NULL && (*err)->code == code, "%s: expected code %d, got %d (%s)", what, code, *err ? (*err)->code : 0,
			*err ? (*err)->message : "no error");
	}
	if (*err) { clo_gerror_free(*err); *err = NULL; }
}

static void read_all(CCLBuffer* b, CCLQueue* cq, void* host, size_t bytes) {
	GError* err = NULL;
	CHECK(ccl_buffer_enqueue_read(b, cq, 1, 0, bytes, host, NULL, &err) != NULL, "read");
	expect(&err, 0, "read");
}

static void test_errors(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	CHECK(clo_rng_new("nosuchrng", CLO_RNG_SEED_DEV_GID, NULL, 16, 0, NULL, ctx, cq, &err) == NULL, "unknown type");
	expect(&err, CLO_ERROR_IMPL_NOT_FOUND, "unknown type");
	CHECK(clo_rng_new(NULL, CLO_RNG_SEED_DEV_GID, NULL, 16, 0, NULL, ctx, cq, &err) == NULL, "NULL type");
	expect(&err, CLO_ERROR_IMPL_NOT_FOUND, "NULL type");
	uint64_t host[4] = { 1, 2, 3, 4 };
	CHECK(clo_rng_new("lcg", CLO_RNG_SEED_DEV_GID, host, 4, 0, NULL, ctx, cq, &err) == NULL, "DEV_GID with seeds");
	expect(&err, CLO_ERROR_ARGS, "DEV_GID with seeds");
	CHECK(clo_rng_new("lcg", CLO_RNG_SEED_HOST_MT, host, 4, 0, NULL, ctx, cq, &err) == NULL, "HOST_MT with seeds");
	expect(&err, CLO_ERROR_ARGS, "HOST_MT with seeds");
	CHECK(clo_rng_new("lcg", CLO_RNG_SEED_EXT_HOST, NULL, 4, 0, NULL, ctx, cq, &err) == NULL, "EXT_HOST without seeds");
	expect(&err, CLO_ERROR_ARGS, "EXT_HOST without seeds");
	CHECK(clo_rng_new("lcg", CLO_RNG_SEED_EXT_DEV, NULL, 4, 0, NULL, ctx, cq, &err) == NULL, "EXT_DEV without seeds");
	expect(&err, CLO_ERROR_ARGS, "EXT_DEV without seeds");
	CHECK(clo_rng_new("lcg", CLO_RNG_SEED_DEV_GID, NULL, 0, 0, NULL, ctx, cq, &err) == NULL, "zero seeds");
	expect(&err, CLO_ERROR_ARGS, "zero seeds");
	CHECK(clo_rng_new("lcg", (CloRngSeedType) 7, NULL, 4, 0, NULL, ctx, cq, &err) == NULL, "unknown seed type");
	expect(&err, CLO_ERROR_ARGS, "unknown seed type");
	CHECK(clo_rng_new("lcg", CLO_RNG_SEED_DEV_GID, NULL, 4, 0, NULL, ctx, NULL, &err) == NULL, "no queue");
	expect(&err, CLO_ERROR_ARGS, "no queue");
	/* a short external buffer: 3 tauslcg states need 48 bytes */
	CCLBuffer* small = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 47, NULL, &err);
	expect(&err, 0, "buffer");
	CHECK(clo_rng_new("tauslcg", CLO_RNG_SEED_EXT_DEV, small, 3, 0, NULL, ctx, cq, &err) == NULL, "short EXT_DEV");
	expect(&err, CLO_ERROR_ARGS, "short EXT_DEV");
	ccl_buffer_destroy(small);
	/* a hash the (stub's) compiler refuses: the JIT sorters' error, the log in the message, nothing leaked */
	CHECK(clo_rng_new("lcg", CLO_RNG_SEED_DEV_GID, NULL, 4, 0, "x = y +", ctx, cq, &err) == NULL, "bad hash");
	CHECK(err && strstr(err->message, "x = y +") && strstr(err->message, "no run-time compiler"), "bad hash message");
	expect(&err, CLO_ERROR_ARGS, "bad hash");
	/* err == NULL is accepted everywhere */
	CHECK(clo_rng_new("nosuchrng", CLO_RNG_SEED_DEV_GID, NULL, 4, 0, NULL, ctx, cq, NULL) == NULL, "NULL err");
	CHECK(clo_rng_new("lcg", CLO_RNG_SEED_EXT_HOST, NULL, 4, 0, NULL, ctx, cq, NULL) == NULL, "NULL err");

	/* fill arguments */
	CloRng* rng = clo_rng_new("xorshift64", CLO_RNG_SEED_DEV_GID, NULL, 8, 1, NULL, ctx, cq, &err);
	expect(&err, 0, "new");
	CCLBuffer* out = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 40, NULL, &err);
	expect(&err, 0, "buffer");
	CHECK(clo_rng_fill(rng, cq, out, 10, 0, 0, &err) == NULL, "bits 0");
	expect(&err, CLO_ERROR_ARGS, "bits 0");
	CHECK(clo_rng_fill(rng, cq, out, 10, 33, 0, &err) == NULL, "bits 33");
	expect(&err, CLO_ERROR_ARGS, "bits 33");
	CHECK(clo_rng_fill(rng, cq, out, 11, 32, 0, &err) == NULL, "short out");
	expect(&err, CLO_ERROR_ARGS, "short out");
	CHECK(clo_rng_fill(rng, cq, NULL, 1, 32, 0, &err) == NULL, "NULL out");
	expect(&err, CLO_ERROR_ARGS, "NULL out");
	CHECK(clo_rng_fill(NULL, cq, out, 1, 32, 0, &err) == NULL, "NULL rng");
	expect(&err, CLO_ERROR_ARGS, "NULL rng");
	CHECK(clo_rng_fill(rng, cq, out, 11, 32, 0, NULL) == NULL, "NULL err");
	CHECK(clo_rng_fill(rng, cq, NULL, 0, 32, 0, &err) != NULL, "numel 0 with no buffer");
	expect(&err, 0, "numel 0");
	ccl_buffer_destroy(out);
	clo_rng_destroy(rng);
}

/* One step of each generator, restated (what the fill must reproduce draw by draw). */
static uint32_t ref_next(int gen, uint32_t* w) {
	uint64_t s;
	switch (gen) {
		case 0: memcpy(&s, w, 8); s = (s * 0x5DEECE66DULL + 0xB) & ((1ULL << 48) - 1); memcpy(w, &s, 8); return (uint32_t) (s >> 16);
		case 1: memcpy(&s, w, 8); s ^= s << 21; s ^= s >> 35; s ^= s << 4; memcpy(w, &s, 8); return (uint32_t) s;
		default: return 0;
	}
}

static void test_seed_types_and_fill(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	const struct clo_rng_info* infos = clo_rng_infos;
	static const char* names[] = { "lcg", "xorshift64", "xorshift128", "mwc64x", "parkmiller", "tauslcg" };
	static const size_t sizes[] = { 8, 8, 16, 8, 4, 16 };
	for (int i = 0; i < 6; ++i)
		CHECK(infos[i].name && !strcmp(infos[i].name, names[i]) && infos[i].seed_size == sizes[i], "infos[%d]", i);
	CHECK(infos[6].name == NULL, "infos end");

	for (int g = 0; g < 6; ++g) {
		for (int t = 0; t < 4; ++t) {
			const size_t S = 37;
			const size_t bytes = S * sizes[g];
			unsigned char* host = (unsigned char*) malloc(bytes);
			for (size_t k = 0; k < bytes; ++k) host[k] = (unsigned char) (k * 7 + 3);
			CCLBuffer* ext = NULL;
			void* seeds = NULL;
			if (t == CLO_RNG_SEED_EXT_HOST) seeds = host;
			if (t == CLO_RNG_SEED_EXT_DEV) {
				ext = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes + 5, NULL, &err);
				expect(&err, 0, "ext buffer");
				ccl_buffer_enqueue_write(ext, cq, 1, 0, bytes, host, NULL, &err);
				expect(&err, 0, "ext write");
				seeds = ext;
			}
			const char* hash = t == CLO_RNG_SEED_DEV_GID ? (g % 3 == 0 ? NULL : g % 3 == 1 ? "KNUTH(x)" : "XS1(x)") : NULL;
			CloRng* rng = clo_rng_new(names[g], (CloRngSeedType) t, seeds, S, 5489, hash, ctx, cq, &err);
			expect(&err, 0, "clo_rng_new");
			if (!rng) { free(host); ccl_buffer_destroy(ext); continue; }
			CHECK(clo_rng_get_size(rng) == bytes, "size");
			CHECK(clo_rng_get_source(rng) && !strncmp(clo_rng_get_source(rng), infos[g].src, strlen(infos[g].src)), "source");
			CCLBuffer* dev = clo_rng_get_device_seeds(rng);
			CHECK(dev != NULL && (t != CLO_RNG_SEED_EXT_DEV || dev == ext), "device seeds");
			unsigned char* st = (unsigned char*) malloc(bytes);
			read_all(dev, cq, st, bytes);
			if (t == CLO_RNG_SEED_EXT_HOST || t == CLO_RNG_SEED_EXT_DEV) CHECK(!memcmp(st, host, bytes), "external seeds %d/%d", g, t);
			if (t == CLO_RNG_SEED_HOST_MT && g == 4) {   /* MT19937 init_genrand(5489): first output 3499211612 */
				uint32_t first;
				memcpy(&first, st, 4);
				CHECK(first == 3499211612u, "HOST_MT first draw %u", first);
			}
			if (t == CLO_RNG_SEED_DEV_GID && g == 0) {   /* lcg, no hash: state g = g + main_seed */
				uint64_t s5;
				memcpy(&s5, st + 5 * 8, 8);
				CHECK(s5 == 5489 + 5, "DEV_GID state");
			}
			/* a fill of 100 numbers with 37 states: 3 draws of states 0..25, 2 of the rest */
			const size_t numel = 100;
			CCLBuffer* out = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, numel * 4, NULL, &err);
			expect(&err, 0, "out");
			CHECK(clo_rng_fill(rng, cq, out, numel, 32, 0, &err) != NULL, "fill");
			expect(&err, 0, "fill");
			uint32_t got[100];
			read_all(out, cq, got, sizeof(got));
			if (g <= 1) {
				uint32_t w[2 * 37];
				memcpy(w, st, bytes);
				for (size_t i = 0; i < numel; ++i)
					CHECK(got[i] == ref_next(g, w + 2 * (i % S)), "fill value %d/%d at %zu", g, t, i);
				unsigned char* after = (unsigned char*) malloc(bytes);
				read_all(dev, cq, after, bytes);
				CHECK(!memcmp(after, w, bytes), "final states %d/%d", g, t);
				free(after);
			}
			CHECK(clo_rng_fill(rng, cq, out, numel, 7, 6, &err) != NULL, "fill maxint");
			expect(&err, 0, "fill maxint");
			read_all(out, cq, got, sizeof(got));
			for (size_t i = 0; i < numel; ++i) CHECK(got[i] < 6, "maxint");
			ccl_buffer_destroy(out);
			clo_rng_destroy(rng);
			if (ext) {   /* the client's buffer outlives the RNG */
				unsigned char* again = (unsigned char*) malloc(bytes);
				read_all(ext, cq, again, bytes);
				CHECK(ccl_buffer_get_size(ext) == bytes + 5, "EXT_DEV buffer survives destroy");
				free(again);
				ccl_buffer_destroy(ext);
			}
			free(st);
			free(host);
		}
	}
}

static void test_known_answers(CCLContext* ctx, CCLQueue* cq) {
	/* java.util.Random(42).nextInt() == -1170105035: the lcg from the scrambled seed 42 ^ 0x5DEECE66D */
	GError* err = NULL;
	uint64_t seed = 42ULL ^ 0x5DEECE66DULL;
	CloRng* rng = clo_rng_new("lcg", CLO_RNG_SEED_EXT_HOST, &seed, 1, 0, NULL, ctx, cq, &err);
	expect(&err, 0, "lcg");
	CCLBuffer* out = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4, NULL, &err);
	clo_rng_fill(rng, cq, out, 1, 32, 0, &err);
	expect(&err, 0, "fill");
	int32_t v;
	read_all(out, cq, &v, 4);
	CHECK(v == -1170105035, "java.util.Random(42) %d", v);
	clo_rng_destroy(rng);
	ccl_buffer_destroy(out);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	test_errors(ctx, cq);
	test_seed_types_and_fill(ctx, cq);
	test_known_answers(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("rng host ok\n");
	return failures ? 1 : 0;
}
