/*
 * kv_host_test.c — clo_sort_by_key_with_device_data / _with_host_data (include/clo_sort.h) on the CPU, over the host
 * stubs of the thin C-ABI (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_sort_by_key_cpu.py).
 * Every key type satradix sorts by key, a key field inside the element, values given and NULL, keys_out given and
 * NULL, in place, the host-data form, and every refusal the driver makes (err == NULL included). The expected result
 * comes from a comparison sort of (key, index) written here, not from the stub's radix sort.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cl_ops.h"

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); ++failures; } } while (0)

static void expect(GError** err, int code, const char* what) {
	if (code == 0) {
		CHECK(*err == NULL, "%s: unexpected error %s", what, *err ? (*err)->message : "");
	} else {
		CHECK(*err != NULL && (*err)->code == code, "%s: expected code %d, got %d (%s)", what, code, *err ? (*err)->code : 0,
			*err ? (*err)->message : "no error");
	}
	if (*err) { clo_gerror_free(*err); *err = NULL; }
}

static uint32_t rng_state = 12345u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

typedef struct { const char* type; const char* get_key; int es; int kind; int shift; int bits; } kcase;

/* the key of element i as a signed 64-bit number in the sort's order */
static int64_t ref_key(const kcase* c, const unsigned char* keys, size_t i) {
	uint32_t e = 0;
	memcpy(&e, keys + i * (size_t) c->es, (size_t) c->es);
	const uint32_t mask = c->bits >= 32 ? 0xffffffffu : ((1u << c->bits) - 1u);
	const uint32_t f = (e >> c->shift) & mask;
	if (c->kind == 0) return (int64_t) f;
	if (c->kind == 1) return (int64_t) f - ((f >> (c->bits - 1)) ? ((int64_t) 1 << c->bits) : 0);   /* two's complement */
	/* IEEE total order: the magnitude, negated for a set sign bit (-0 before +0, -NaN first, +NaN last) */
	const int64_t mag = (int64_t) (f & (mask >> 1));
	return (f >> (c->bits - 1)) ? -mag - 1 : mag;
}

static const kcase* g_case;
static const unsigned char* g_keys;
static int cmp_idx(const void* a, const void* b) {
	const uint32_t i = *(const uint32_t*) a, j = *(const uint32_t*) b;
	const int64_t ki = ref_key(g_case, g_keys, i), kj = ref_key(g_case, g_keys, j);
	if (ki != kj) return ki < kj ? -1 : 1;
	return i < j ? -1 : (i > j ? 1 : 0);   /* stable */
}

static void fill_keys(const kcase* c, unsigned char* keys, size_t n, int dup) {
	for (size_t i = 0; i < n; ++i) {
		uint32_t x = rnd();
		if (dup) x %= 5u;   /* heavy duplicates */
		if (c->kind == 2 && (i % 7) == 0) {   /* specials: +-0, +-inf, NaNs of both signs */
			static const uint32_t f32[6] = { 0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00001u, 0xffc00002u };
			static const uint32_t f16[6] = { 0x0000u, 0x8000u, 0x7c00u, 0xfc00u, 0x7e01u, 0xfe02u };
			x = c->es == 4 ? f32[(i / 7) % 6] : f16[(i / 7) % 6];
		}
		memcpy(keys + i * (size_t) c->es, &x, (size_t) c->es);
	}
}

/* mode bit 0: values given, bit 1: keys_out given, bit 2: in place (both given, outputs = inputs) */
static void run_case(CCLContext* ctx, CCLQueue* cq, const kcase* c, const char* options, size_t n, int mode, int dup) {
	GError* err = NULL;
	CloType et;
	et = (CloType) 0;
	const char* tn = c->type;
	et = clo_type_by_name(tn, &err);
	expect(&err, 0, "type");
	CloSort* s = clo_sort_new("satradix", options, ctx, &et, NULL, NULL, c->get_key, NULL, &err);
	expect(&err, 0, "clo_sort_new");
	if (!s) return;
	const int vals = mode & 1, kout = (mode & 2) != 0, inplace = (mode & 4) != 0;
	const size_t kb = n * (size_t) c->es, vb = n * 4;
	unsigned char* keys = (unsigned char*) malloc(kb + 1);
	uint32_t* values = (uint32_t*) malloc(vb + 4);
	unsigned char* got_k = (unsigned char*) malloc(kb + 1);
	uint32_t* got_v = (uint32_t*) malloc(vb + 4);
	uint32_t* order = (uint32_t*) malloc(n * 4 + 4);
	fill_keys(c, keys, n, dup);
	for (size_t i = 0; i < n; ++i) { values[i] = rnd(); order[i] = (uint32_t) i; }
	g_case = c; g_keys = keys;
	if (n) qsort(order, n, 4, cmp_idx);

	CCLBuffer* kin = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, kb + 1, NULL, &err);
	CCLBuffer* vin = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, vb + 4, NULL, &err);
	CCLBuffer* ko = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, kb + 1, NULL, &err);
	CCLBuffer* vo = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, vb + 4, NULL, &err);
	expect(&err, 0, "buffers");
	if (n) {
		ccl_buffer_enqueue_write(kin, cq, CL_TRUE, 0, kb, keys, NULL, &err);
		ccl_buffer_enqueue_write(vin, cq, CL_TRUE, 0, vb, values, NULL, &err);
		expect(&err, 0, "write");
	}
	CCLEvent* evt = clo_sort_by_key_with_device_data(s, cq, NULL, kin, (vals || inplace) ? vin : NULL,
		inplace ? kin : (kout ? ko : NULL), inplace ? vin : vo, n, 0, &err);
	expect(&err, 0, "sort by key");
	CHECK(evt != NULL, "no event");
	if (n) {
		ccl_buffer_enqueue_read(inplace ? vin : vo, cq, CL_TRUE, 0, vb, got_v, NULL, &err);
		if (kout || inplace) ccl_buffer_enqueue_read(inplace ? kin : ko, cq, CL_TRUE, 0, kb, got_k, NULL, &err);
		expect(&err, 0, "read");
	}
	int bad = 0;
	for (size_t j = 0; j < n && !bad; ++j) {
		const uint32_t want_v = (vals || inplace) ? values[order[j]] : order[j];
		if (got_v[j] != want_v) bad = 1;
		if ((kout || inplace) && memcmp(got_k + j * (size_t) c->es, keys + (size_t) order[j] * (size_t) c->es, (size_t) c->es) != 0) bad = 1;
	}
	CHECK(!bad, "%s get_key %s options %s n %zu mode %d dup %d: wrong result", c->type, c->get_key ? c->get_key : "-",
		options ? options : "-", n, mode, dup);

	/* the host-data form gives the same */
	if (n && !inplace) {
		unsigned char* hk = (unsigned char*) malloc(kb);
		uint32_t* hv = (uint32_t*) malloc(vb);
		CHECK(clo_sort_by_key_with_host_data(s, cq, NULL, keys, vals ? values : NULL, kout ? hk : NULL, hv, n, 0, &err), "host data");
		expect(&err, 0, "host data");
		CHECK(memcmp(hv, got_v, vb) == 0, "host data values differ (%s n %zu mode %d)", c->type, n, mode);
		if (kout) CHECK(memcmp(hk, got_k, kb) == 0, "host data keys differ (%s n %zu mode %d)", c->type, n, mode);
		free(hk);
		free(hv);
	}
	ccl_buffer_destroy(kin); ccl_buffer_destroy(vin); ccl_buffer_destroy(ko); ccl_buffer_destroy(vo);
	free(keys); free(values); free(got_k); free(got_v); free(order);
	clo_sort_destroy(s);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	CCLBuffer* k = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 64, NULL, &err);
	CCLBuffer* v = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 64, NULL, &err);
	expect(&err, 0, "buffers");
	uint32_t hk[4] = { 3, 1, 2, 0 }, hv[4], ho[4];
	CloType ui = CLO_UINT, ul = CLO_ULONG;
	static const char* const others[3] = { "sbitonic", "abitonic", "gselect" };
	for (int i = 0; i < 3; ++i) {
		CloSort* s = clo_sort_new(others[i], NULL, ctx, &ui, NULL, NULL, NULL, NULL, &err);
		expect(&err, 0, others[i]);
		CHECK(clo_sort_by_key_with_device_data(s, cq, NULL, k, NULL, NULL, v, 4, 0, &err) == NULL, "%s", others[i]);
		expect(&err, CLO_ERROR_ARGS, others[i]);
		CHECK(!clo_sort_by_key_with_host_data(s, cq, NULL, hk, NULL, NULL, ho, 4, 0, &err), "%s host", others[i]);
		expect(&err, CLO_ERROR_ARGS, others[i]);
		CHECK(clo_sort_by_key_with_device_data(s, cq, NULL, k, NULL, NULL, v, 4, 0, NULL) == NULL, "%s, err NULL", others[i]);
		clo_sort_destroy(s);
	}
	CloSort* s8 = clo_sort_new("satradix", NULL, ctx, &ul, NULL, NULL, NULL, NULL, &err);
	expect(&err, 0, "ulong sorter");
	CHECK(clo_sort_by_key_with_device_data(s8, cq, NULL, k, NULL, NULL, v, 4, 0, &err) == NULL, "8-byte elements");
	expect(&err, CLO_ERROR_ARGS, "8-byte elements");
	CHECK(!clo_sort_by_key_with_host_data(s8, NULL, NULL, hk, NULL, NULL, ho, 2, 0, NULL), "8-byte elements, host, err NULL");
	clo_sort_destroy(s8);
	CloSort* s = clo_sort_new("satradix", NULL, ctx, &ui, NULL, NULL, NULL, NULL, &err);
	expect(&err, 0, "uint sorter");
	CHECK(clo_sort_by_key_with_device_data(s, cq, NULL, k, NULL, k, NULL, 4, 0, &err) == NULL, "values_out NULL");
	expect(&err, CLO_ERROR_ARGS, "values_out NULL");
	CHECK(!clo_sort_by_key_with_host_data(s, cq, NULL, hk, hv, hk, NULL, 4, 0, &err), "values_out NULL, host");
	expect(&err, CLO_ERROR_ARGS, "values_out NULL, host");
	CHECK(clo_sort_by_key_with_device_data(s, cq, NULL, k, NULL, NULL, v, (size_t) 1 << 32, 0, &err) == NULL, "numel 2^32");
	expect(&err, CLO_ERROR_ARGS, "numel 2^32");
	CHECK(!clo_sort_by_key_with_host_data(s, cq, NULL, hk, NULL, NULL, ho, (size_t) 1 << 32, 0, &err), "numel 2^32, host");
	expect(&err, CLO_ERROR_ARGS, "numel 2^32, host");
	CHECK(clo_sort_by_key_with_device_data(s, cq, NULL, k, NULL, NULL, NULL, 4, 0, NULL) == NULL, "values_out NULL, err NULL");
	CHECK(clo_sort_by_key_with_device_data(s, cq, NULL, k, NULL, NULL, v, 17, 0, &err) == NULL, "numel beyond the buffers");
	expect(&err, CLO_ERROR_ARGS, "numel beyond the buffers");
	/* numel 0 behaves as the plain sort's 0: an event, nothing written */
	CCLEvent* e0 = clo_sort_by_key_with_device_data(s, cq, NULL, k, NULL, NULL, v, 0, 0, &err);
	expect(&err, 0, "numel 0");
	CHECK(e0 != NULL, "numel 0: no event");
	CHECK(clo_sort_by_key_with_host_data(s, cq, NULL, hk, NULL, NULL, ho, 0, 0, &err), "numel 0, host");
	expect(&err, 0, "numel 0, host");
	clo_sort_destroy(s);
	ccl_buffer_destroy(k);
	ccl_buffer_destroy(v);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const kcase cases[] = {
		{ "uchar", NULL, 1, 0, 0, 8 }, { "char", NULL, 1, 1, 0, 8 }, { "ushort", NULL, 2, 0, 0, 16 }, { "short", NULL, 2, 1, 0, 16 },
		{ "uint", NULL, 4, 0, 0, 32 }, { "int", NULL, 4, 1, 0, 32 }, { "half", NULL, 2, 2, 0, 16 }, { "float", NULL, 4, 2, 0, 32 },
		{ "uint", "((x) & 0xffff)", 4, 0, 0, 16 }, { "uint", "((x) >> 8)", 4, 0, 8, 24 },
	};
	static const size_t sizes[] = { 0, 1, 37, 1000 };
	static const char* const options[] = { NULL, "radix=4", "radix=256" };
	for (size_t c = 0; c < sizeof(cases) / sizeof(cases[0]); ++c)
		for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z)
			for (int mode = 0; mode < 5; ++mode)
				for (int o = 0; o < 3; ++o)
					run_case(ctx, cq, &cases[c], options[o], sizes[z], mode, (int) (z + mode) % 2);
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("kv host ok\n");
	return failures ? 1 : 0;
}
