/*
 * merge_host_test.c — CloMerge (include/clo_merge.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_merge_cpu.py). Every key type; keys only, 4-
 * and 8-byte values, argmerge with and without keys_out; an empty side, both sides empty; the host-data form; one
 * object used large -> small -> large (its workspace grows once and is reused); every refusal the driver makes (err
 * == NULL included), with the outputs left alone; a clean destroy. The expected results are computed here by an
 * insertion of B's elements into A by their order keys, not taken from the stub.
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

static uint32_t rng_state = 2463534242u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int kind_of(CloType t) {
	if (t == CLO_CHAR || t == CLO_SHORT || t == CLO_INT || t == CLO_LONG) return 1;
	if (t == CLO_HALF || t == CLO_FLOAT || t == CLO_DOUBLE) return 2;
	return 0;
}

/* the bits of a key as an unsigned number in the merge's order */
static uint64_t order_key(uint64_t bits, size_t ks, int kind) {
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	bits &= all;
	if (kind == 1) return bits ^ sign;
	if (kind == 2) return (bits & sign) ? bits ^ all : bits ^ sign;
	return bits;
}

typedef struct { uint64_t ord, bits; uint32_t index; uint64_t value; } elem;

static int by_order(const void* x, const void* y) {
	const elem* a = (const elem*) x; const elem* b = (const elem*) y;
	if (a->ord != b->ord) return a->ord < b->ord ? -1 : 1;
	return a->index < b->index ? -1 : a->index > b->index;
}

/* n sorted keys drawn from few values (so that ties occur) around the type's sign change, with values */
static void make_side(elem* e, size_t n, size_t ks, int kind, uint32_t first_index) {
	for (size_t i = 0; i < n; ++i) {
		uint64_t bits = (uint64_t) (rnd() % 23) - 11u;   /* -11 .. 11 as two's complement */
		if (kind == 2) bits = (rnd() & 1 ? 1ull << (8 * ks - 1) : 0ull) | (rnd() % 7);   /* +-0 and small denormals */
		e[i].bits = ks == 8 ? bits : bits & ((1ull << (8 * ks)) - 1ull);
		e[i].ord = order_key(bits, ks, kind);
		e[i].index = 0;
		e[i].value = ((uint64_t) rnd() << 32) | rnd();
	}
	qsort(e, n, sizeof(elem), by_order);   /* (all indices 0: any order among equal keys; their bits are equal) */
	for (size_t i = 0; i < n; ++i) e[i].index = first_index + (uint32_t) i;
}

enum { KEYS_ONLY, VAL4, VAL8, ARG, ARG_ONLY };

static void run_merge(CCLContext* ctx, CCLQueue* cq, CloMerge* m, CloType kt, int mode, size_t na, size_t nb, int host_form) {
	GError* err = NULL;
	const size_t ks = clo_type_sizeof(kt), vs = mode == KEYS_ONLY ? 0 : mode == VAL8 ? 8 : 4, n = na + nb;
	const int kind = kind_of(kt), vals = mode == VAL4 || mode == VAL8, keys_out = mode != ARG_ONLY;
	elem* e = (elem*) malloc((n + 1) * sizeof(elem));
	make_side(e, na, ks, kind, 0);
	make_side(e + na, nb, ks, kind, (uint32_t) na);
	unsigned char* hk = (unsigned char*) malloc(n * ks + 8);
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	for (size_t i = 0; i < n; ++i) { memcpy(hk + i * ks, &e[i].bits, ks); memcpy(hv + i * vs, &e[i].value, vs); }
	qsort(e, n, sizeof(elem), by_order);   /* by key, ties by index in A || B: the stable order */
	unsigned char* want_k = (unsigned char*) malloc(n * ks + 8);
	unsigned char* want_v = (unsigned char*) malloc(n * 8 + 8);
	for (size_t i = 0; i < n; ++i) {
		memcpy(want_k + i * ks, &e[i].bits, ks);
		if (vals) memcpy(want_v + i * vs, &e[i].value, vs); else memcpy(want_v + i * 4, &e[i].index, 4);
	}
	unsigned char* got_k = (unsigned char*) malloc(n * ks + 8);
	unsigned char* got_v = (unsigned char*) malloc(n * 8 + 8);
	memset(got_k, 0xEE, n * ks + 8);
	memset(got_v, 0xEE, n * 8 + 8);
	if (host_form) {
		CHECK(clo_merge_with_host_data(m, (na & 1) ? cq : NULL, NULL, hk, vals ? hv : NULL, na, hk + na * ks, vals ? hv + na * vs : NULL, nb,
			keys_out ? got_k : NULL, vs ? got_v : NULL, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[6];   /* keys a, values a, keys b, values b, keys out, values out */
		const size_t bytes[6] = { na * ks, na * vs, nb * ks, nb * vs, n * ks, n * vs };
		for (int i = 0; i < 6; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], hk, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, bytes[1], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], hk + na * ks, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3], hv + na * vs, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, bytes[4] + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_write(b[5], cq, CL_TRUE, 0, bytes[5] + 8, got_v, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_merge_with_device_data(m, cq, NULL, b[0], vals ? b[1] : NULL, na, b[2], vals ? b[3] : NULL, nb,
			keys_out ? b[4] : NULL, vs ? b[5] : NULL, &err);
		expect(&err, 0, "merge");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, bytes[4] + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_read(b[5], cq, CL_TRUE, 0, bytes[5] + 8, got_v, NULL, &err);
		expect(&err, 0, "read");
		for (int i = 0; i < 6; ++i) ccl_buffer_destroy(b[i]);
	}
	if (keys_out) CHECK(memcmp(got_k, want_k, n * ks) == 0, "key type %d mode %d %zu + %zu host %d: wrong keys", (int) kt, mode, na, nb, host_form);
	if (vs) CHECK(memcmp(got_v, want_v, n * vs) == 0, "key type %d mode %d %zu + %zu host %d: wrong values", (int) kt, mode, na, nb, host_form);
	for (size_t i = keys_out ? n * ks : 0; i < n * ks + 8; ++i) CHECK(got_k[i] == 0xEE, "keys_out written at byte %zu (mode %d, %zu + %zu)", i, mode, na, nb);
	for (size_t i = n * vs; i < n * 8 + 8; ++i) CHECK(got_v[i] == 0xEE, "values_out written at byte %zu (mode %d, %zu + %zu)", i, mode, na, nb);
	free(e); free(hk); free(hv); free(want_k); free(want_v); free(got_k); free(got_v);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_merge_new(NULL, ctx, CLO_UINT, 2, &err), "value_size 2");
	REFUSED_NEW(clo_merge_new(NULL, ctx, CLO_UINT, 16, &err), "value_size 16");
	REFUSED_NEW(clo_merge_new("descending", ctx, CLO_UINT, 0, &err), "options");
	REFUSED_NEW(clo_merge_new(NULL, ctx, (CloType) 11, 0, &err), "an unknown key type");
	CHECK(clo_merge_new(NULL, ctx, CLO_UINT, 3, NULL) == NULL, "value_size 3, err NULL");
	CHECK(clo_merge_new("x", ctx, CLO_UINT, 4, NULL) == NULL, "options, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* ka = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);
	CCLBuffer* kb = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);         /* adjacent to ka */
	CCLBuffer* va = ccl_buffer_new_from_device_ptr(ctx, base + 256, 64, &err);
	CCLBuffer* vb = ccl_buffer_new_from_device_ptr(ctx, base + 320, 64, &err);
	CCLBuffer* ko = ccl_buffer_new_from_device_ptr(ctx, base + 512, 128, &err);
	CCLBuffer* vo = ccl_buffer_new_from_device_ptr(ctx, base + 640, 128, &err);       /* adjacent to ko */
	CCLBuffer* ko_on_kb = ccl_buffer_new_from_device_ptr(ctx, base + 124, 128, &err); /* one shared element with kb */
	CCLBuffer* vo_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 600, 128, &err); /* starts inside ko */
	CCLBuffer* ko_in_va = ccl_buffer_new_from_device_ptr(ctx, base + 200, 128, &err); /* across the start of va */
	expect(&err, 0, "buffers");
	uint32_t h[16] = { 0 }, g[16] = { 0 }, hv[16] = { 0 }, gv[16] = { 0 }, ho[32], hvo[32];
	for (int i = 0; i < 32; ++i) { ho[i] = 0xABCD0000u + (uint32_t) i; hvo[i] = 0x12340000u + (uint32_t) i; }
	CloMerge* m0 = clo_merge_new(NULL, ctx, CLO_UINT, 0, &err);
	CloMerge* m4 = clo_merge_new("", ctx, CLO_UINT, 4, &err);
	CloMerge* m8 = clo_merge_new(NULL, ctx, CLO_UINT, 8, &err);
	expect(&err, 0, "objects");
	if (!m0 || !m4 || !m8) return;
	CHECK(clo_merge_get_context(m4) == ctx && clo_merge_get_key_type(m4) == CLO_UINT && clo_merge_get_key_size(m4) == 4
		&& clo_merge_get_value_size(m4) == 4 && clo_merge_get_value_size(m0) == 0 && clo_merge_get_value_size(m8) == 8, "getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_merge_with_device_data(m4, cq, NULL, ka, va, ((size_t) 1 << 32) - 16, kb, vb, 16, ko, vo, &err), "n 2^32");
	REFUSED_HOST(clo_merge_with_host_data(m4, cq, NULL, h, hv, (size_t) 1 << 31, g, gv, (size_t) 1 << 31, ho, hvo, &err), "n 2^32, host");
	REFUSED_DEV(clo_merge_with_device_data(m0, cq, NULL, NULL, NULL, 16, kb, NULL, 16, ko, NULL, &err), "keys_a NULL");
	REFUSED_HOST(clo_merge_with_host_data(m0, cq, NULL, h, NULL, 16, NULL, NULL, 16, ho, NULL, &err), "keys_b NULL, host");
	REFUSED_DEV(clo_merge_with_device_data(m4, cq, NULL, ka, va, 16, kb, NULL, 16, ko, vo, &err), "values_b alone NULL");
	REFUSED_HOST(clo_merge_with_host_data(m4, cq, NULL, h, NULL, 16, g, gv, 16, ho, hvo, &err), "values_a alone NULL, host");
	REFUSED_DEV(clo_merge_with_device_data(m0, cq, NULL, ka, va, 16, kb, vb, 16, ko, NULL, &err), "values with value_size 0");
	REFUSED_HOST(clo_merge_with_host_data(m0, cq, NULL, h, NULL, 16, g, NULL, 16, ho, hvo, &err), "values_out with value_size 0, host");
	REFUSED_DEV(clo_merge_with_device_data(m4, cq, NULL, ka, va, 16, kb, vb, 16, ko, NULL, &err), "values_out NULL");
	REFUSED_HOST(clo_merge_with_host_data(m8, cq, NULL, h, NULL, 8, g, NULL, 8, ho, hvo, &err), "NULL values with value_size 8, host");
	REFUSED_DEV(clo_merge_with_device_data(m8, cq, NULL, ka, NULL, 8, kb, NULL, 8, ko, vo, &err), "NULL values with value_size 8");
	REFUSED_DEV(clo_merge_with_device_data(m0, cq, NULL, ka, NULL, 16, kb, NULL, 16, NULL, NULL, &err), "both outputs NULL");
	REFUSED_HOST(clo_merge_with_host_data(m4, cq, NULL, h, hv, 16, g, gv, 16, NULL, NULL, &err), "both outputs NULL, host");
	REFUSED_DEV(clo_merge_with_device_data(m0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ka, NULL, &err), "keys_out on keys_a");
	REFUSED_DEV(clo_merge_with_device_data(m0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko_on_kb, NULL, &err), "keys_out sharing kb's last element");
	REFUSED_DEV(clo_merge_with_device_data(m4, cq, NULL, ka, va, 16, kb, vb, 16, ko_in_va, vo, &err), "keys_out across the start of values_a");
	REFUSED_DEV(clo_merge_with_device_data(m4, cq, NULL, ka, va, 16, kb, vb, 16, ko, vo_in_ko, &err), "values_out inside keys_out");
	REFUSED_DEV(clo_merge_with_device_data(m4, cq, NULL, ka, va, 16, kb, vb, 16, ko, vb, &err), "values_out on values_b");
	REFUSED_HOST(clo_merge_with_host_data(m4, cq, NULL, h, hv, 16, g, gv, 16, ho, ho + 31, &err), "values_out on keys_out's last element, host");
	REFUSED_HOST(clo_merge_with_host_data(m0, cq, NULL, ho + 8, NULL, 16, g, NULL, 16, ho, NULL, &err), "keys_a inside keys_out, host");
	REFUSED_DEV(clo_merge_with_device_data(m0, cq, NULL, ka, NULL, 17, kb, NULL, 16, ko, NULL, &err), "numel_a beyond the buffer");
	REFUSED_DEV(clo_merge_with_device_data(m4, cq, NULL, ka, va, 16, kb, vb, 16, ko, va, &err), "values_out too small (and on values_a)");
	/* err == NULL */
	CHECK(clo_merge_with_device_data(m0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ka, NULL, NULL) == NULL, "in place, err NULL");
	CHECK(clo_merge_with_device_data(m4, cq, NULL, ka, va, 16, kb, NULL, 16, ko, vo, NULL) == NULL, "one values NULL, err NULL");
	CHECK(!clo_merge_with_host_data(m4, NULL, NULL, h, hv, (size_t) 1 << 32, g, gv, 1, ho, hvo, NULL), "n 2^32, host, err NULL");
	CHECK(!clo_merge_with_host_data(m0, NULL, NULL, h, NULL, 16, g, NULL, 16, NULL, NULL, NULL), "both outputs NULL, host, err NULL");
	for (int i = 0; i < 32; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	/* adjacent, disjoint views of one allocation are accepted */
	CHECK(clo_merge_with_device_data(m4, cq, NULL, ka, va, 16, kb, vb, 16, ko, vo, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	/* both inputs empty: success, nothing written, no queue needed in the host form */
	CHECK(clo_merge_with_host_data(m4, NULL, NULL, NULL, NULL, 0, NULL, NULL, 0, ho, hvo, &err), "both empty, host");
	expect(&err, 0, "both empty, host");
	CHECK(clo_merge_with_device_data(m4, cq, NULL, NULL, NULL, 0, NULL, NULL, 0, ko, vo, &err) != NULL, "both empty, device");
	expect(&err, 0, "both empty, device");
	for (int i = 0; i < 32; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "an empty merge wrote an output at %d", i);

	clo_merge_destroy(m0); clo_merge_destroy(m4); clo_merge_destroy(m8);
	ccl_buffer_destroy(ka); ccl_buffer_destroy(kb); ccl_buffer_destroy(va); ccl_buffer_destroy(vb); ccl_buffer_destroy(ko);
	ccl_buffer_destroy(vo); ccl_buffer_destroy(ko_on_kb); ccl_buffer_destroy(vo_in_ko); ccl_buffer_destroy(ko_in_va);
	ccl_buffer_destroy(big);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType types[] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };
	/* large -> small -> large on one object per mode, with an empty side on either hand and both */
	static const size_t sizes[][2] = { { 9000, 7001 }, { 37, 5 }, { 0, 300 }, { 300, 0 }, { 1, 1 }, { 0, 0 }, { 12000, 9000 } };
	for (size_t t = 0; t < sizeof(types) / sizeof(types[0]); ++t) {
		for (int mode = KEYS_ONLY; mode <= ARG_ONLY; ++mode) {
			CloMerge* m = clo_merge_new(NULL, ctx, types[t], mode == KEYS_ONLY ? 0 : mode == VAL8 ? 8 : 4, &err);
			expect(&err, 0, "clo_merge_new");
			if (!m) continue;
			for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z)
				for (int host_form = 0; host_form < 2; ++host_form)
					run_merge(ctx, cq, m, types[t], mode, sizes[z][0], sizes[z][1], host_form);
			clo_merge_destroy(m);
		}
	}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("merge host ok\n");
	return failures ? 1 : 0;
}
