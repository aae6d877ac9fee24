/*
 * setop_host_test.c — CloSetOp (include/clo_setop.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_setop_cpu.py). Every op and key type; keys only,
 * 4- and 8-byte values, the arg form with and without keys_out; an empty side, both sides empty; the host-data form; one
 * object used large -> small -> large (its workspace grows once and is reused); every refusal the driver makes (err
 * == NULL included), with the outputs left alone; a clean destroy. The expected results are computed here from the
 * sorted concatenation and the counts of every group of equal keys, not taken from the stub.
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

/* n sorted keys drawn from few values (so that runs occur in both inputs) around the type's sign change, with values */
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
static const char* const op_names[4] = { "union", "intersection", "difference", "symmetric_difference" };

/* e[0, n): A || B sorted by (key, index). The kept elements, in place at the front; returns how many. */
static size_t keep_rows(elem* e, size_t n, size_t na, int op) {
	size_t k = 0;
	for (size_t g = 0; g < n;) {
		size_t end = g, m = 0;
		while (end < n && e[end].ord == e[g].ord) { if (e[end].index < na) ++m; ++end; }
		const size_t c = end - g - m;
		for (size_t i = g; i < end; ++i) {
			const int from_a = e[i].index < na;
			const size_t rank = from_a ? i - g : i - g - m;
			const int matched = from_a ? rank < c : rank < m;
			const int keep = op == 0 ? (from_a || !matched) : op == 1 ? (from_a && matched) : op == 2 ? (from_a && !matched) : !matched;
			if (keep) e[k++] = e[i];
		}
		g = end;
	}
	return k;
}

static void run_setop(CCLContext* ctx, CCLQueue* cq, CloSetOp* so, int op, CloType kt, int mode, size_t na, size_t nb, int host_form) {
	GError* err = NULL;
	const size_t ks = clo_type_sizeof(kt), vs = mode == KEYS_ONLY ? 0 : mode == VAL8 ? 8 : 4, n = na + nb;
	const int kind = kind_of(kt), vals = mode == VAL4 || mode == VAL8, keys_out = mode != ARG_ONLY, keeps_b = op == 0 || op == 3;
	const size_t cap = clo_setop_get_max_numel_out(so, na, nb);
	CHECK(cap == (keeps_b ? n : op == 2 ? na : (na < nb ? na : nb)), "capacity of %s for %zu + %zu: %zu", op_names[op], na, nb, cap);
	elem* e = (elem*) malloc((n + 1) * sizeof(elem));
	make_side(e, na, ks, kind, 0);
	make_side(e + na, nb, ks, kind, (uint32_t) na);
	unsigned char* hk = (unsigned char*) malloc(n * ks + 8);
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	for (size_t i = 0; i < n; ++i) { memcpy(hk + i * ks, &e[i].bits, ks); memcpy(hv + i * vs, &e[i].value, vs); }
	qsort(e, n, sizeof(elem), by_order);   /* by key, ties by index in A || B: the merge order */
	const size_t k = keep_rows(e, n, na, op);
	CHECK(k <= cap, "%zu rows expected in a capacity of %zu", k, cap);
	unsigned char* want_k = (unsigned char*) malloc(cap * ks + 8);
	unsigned char* want_v = (unsigned char*) malloc(cap * 8 + 8);
	for (size_t i = 0; i < k; ++i) {
		memcpy(want_k + i * ks, &e[i].bits, ks);
		if (vals) memcpy(want_v + i * vs, &e[i].value, vs); else memcpy(want_v + i * 4, &e[i].index, 4);
	}
	unsigned char* got_k = (unsigned char*) malloc(cap * ks + 8);
	unsigned char* got_v = (unsigned char*) malloc(cap * 8 + 8);
	memset(got_k, 0xEE, cap * ks + 8);
	memset(got_v, 0xEE, cap * 8 + 8);
	size_t got = 12345;
	/* intersection and difference never look at values_b: every other call passes NULL for it */
	const unsigned char* hvb = vals && (keeps_b || ((na + nb) & 1)) ? hv + na * vs : NULL;
	if (host_form) {
		CHECK(clo_setop_with_host_data(so, (na & 1) ? cq : NULL, NULL, hk, vals ? hv : NULL, na, hk + na * ks, hvb, nb,
			keys_out ? got_k : NULL, vs ? got_v : NULL, &got, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[7];   /* keys a, values a, keys b, values b, keys out, values out, the count */
		const size_t bytes[7] = { na * ks, na * vs, nb * ks, nb * vs, cap * ks, cap * vs, 8 };
		cl_ulong count = 12345;
		for (int i = 0; i < 7; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], hk, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, bytes[1], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], hk + na * ks, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3], hv + na * vs, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, bytes[4] + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_write(b[5], cq, CL_TRUE, 0, bytes[5] + 8, got_v, NULL, &err);
		ccl_buffer_enqueue_write(b[6], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_setop_with_device_data(so, cq, NULL, b[0], vals ? b[1] : NULL, na, b[2], hvb ? b[3] : NULL, nb,
			keys_out ? b[4] : NULL, vs ? b[5] : NULL, b[6], &err);
		expect(&err, 0, "setop");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, bytes[4] + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_read(b[5], cq, CL_TRUE, 0, bytes[5] + 8, got_v, NULL, &err);
		ccl_buffer_enqueue_read(b[6], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "read");
		got = (size_t) count;
		for (int i = 0; i < 7; ++i) ccl_buffer_destroy(b[i]);
	}
	CHECK(got == k, "%s key type %d mode %d %zu + %zu host %d: %zu rows, expected %zu", op_names[op], (int) kt, mode, na, nb, host_form, got, k);
	if (keys_out) CHECK(memcmp(got_k, want_k, k * ks) == 0, "%s key type %d mode %d %zu + %zu host %d: wrong keys", op_names[op], (int) kt, mode, na, nb, host_form);
	if (vs) CHECK(memcmp(got_v, want_v, k * vs) == 0, "%s key type %d mode %d %zu + %zu host %d: wrong values", op_names[op], (int) kt, mode, na, nb, host_form);
	for (size_t i = keys_out ? k * ks : 0; i < cap * ks + 8; ++i) CHECK(got_k[i] == 0xEE, "keys_out written at byte %zu (%s mode %d, %zu + %zu)", i, op_names[op], mode, na, nb);
	for (size_t i = k * vs; i < cap * 8 + 8; ++i) CHECK(got_v[i] == 0xEE, "values_out written at byte %zu (%s mode %d, %zu + %zu)", i, op_names[op], mode, na, nb);
	free(e); free(hk); free(hv); free(want_k); free(want_v); free(got_k); free(got_v);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_setop_new("union", NULL, ctx, CLO_UINT, 2, &err), "value_size 2");
	REFUSED_NEW(clo_setop_new("union", NULL, ctx, CLO_UINT, 16, &err), "value_size 16");
	REFUSED_NEW(clo_setop_new("union", "descending", ctx, CLO_UINT, 0, &err), "options");
	REFUSED_NEW(clo_setop_new("union", NULL, ctx, (CloType) 11, 0, &err), "an unknown key type");
	REFUSED_NEW(clo_setop_new("xor", NULL, ctx, CLO_UINT, 0, &err), "an unknown op");
	REFUSED_NEW(clo_setop_new(NULL, NULL, ctx, CLO_UINT, 0, &err), "a NULL op");
	REFUSED_NEW(clo_setop_new("Union", NULL, ctx, CLO_UINT, 0, &err), "an op in another case");
	CHECK(clo_setop_new("union", NULL, ctx, CLO_UINT, 3, NULL) == NULL, "value_size 3, err NULL");
	CHECK(clo_setop_new("unio", NULL, ctx, CLO_UINT, 4, NULL) == NULL, "an unknown op, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* ka = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);
	CCLBuffer* kb = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);         /* adjacent to ka */
	CCLBuffer* va = ccl_buffer_new_from_device_ptr(ctx, base + 256, 64, &err);
	CCLBuffer* vb = ccl_buffer_new_from_device_ptr(ctx, base + 320, 64, &err);
	CCLBuffer* ko = ccl_buffer_new_from_device_ptr(ctx, base + 512, 128, &err);
	CCLBuffer* vo = ccl_buffer_new_from_device_ptr(ctx, base + 640, 128, &err);       /* adjacent to ko */
	CCLBuffer* cnt = ccl_buffer_new_from_device_ptr(ctx, base + 768, 8, &err);        /* adjacent to vo */
	CCLBuffer* ko_on_kb = ccl_buffer_new_from_device_ptr(ctx, base + 124, 128, &err); /* one shared element with kb */
	CCLBuffer* vo_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 600, 128, &err); /* starts inside ko */
	CCLBuffer* cnt_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 632, 8, &err);  /* the last 8 bytes of ko */
	CCLBuffer* cnt_in_ka = ccl_buffer_new_from_device_ptr(ctx, base + 8, 8, &err);
	CCLBuffer* cnt_odd = ccl_buffer_new_from_device_ptr(ctx, base + 772, 8, &err);    /* not 8-byte aligned */
	CCLBuffer* cnt_small = ccl_buffer_new_from_device_ptr(ctx, base + 776, 4, &err);
	CCLBuffer* ko_64 = ccl_buffer_new_from_device_ptr(ctx, base + 1024, 64, &err);    /* 16 keys: enough for an intersection */
	expect(&err, 0, "buffers");
	uint32_t h[16] = { 0 }, g[16] = { 0 }, hv[16] = { 0 }, gv[16] = { 0 }, ho[40], hvo[40];
	for (int i = 0; i < 40; ++i) { ho[i] = 0xABCD0000u + (uint32_t) i; hvo[i] = 0x12340000u + (uint32_t) i; }
	size_t hn = 777;
	CloSetOp* u0 = clo_setop_new("union", NULL, ctx, CLO_UINT, 0, &err);
	CloSetOp* u4 = clo_setop_new("union", "", ctx, CLO_UINT, 4, &err);
	CloSetOp* u8 = clo_setop_new("symmetric_difference", NULL, ctx, CLO_UINT, 8, &err);
	CloSetOp* i4 = clo_setop_new("intersection", NULL, ctx, CLO_UINT, 4, &err);
	CloSetOp* d0 = clo_setop_new("difference", NULL, ctx, CLO_UINT, 0, &err);
	expect(&err, 0, "objects");
	if (!u0 || !u4 || !u8 || !i4 || !d0) return;
	CHECK(clo_setop_get_context(u4) == ctx && clo_setop_get_key_type(u4) == CLO_UINT && clo_setop_get_key_size(u4) == 4
		&& clo_setop_get_value_size(u4) == 4 && clo_setop_get_value_size(u0) == 0 && clo_setop_get_value_size(u8) == 8
		&& !strcmp(clo_setop_get_op(u8), "symmetric_difference") && !strcmp(clo_setop_get_op(d0), "difference"), "getters");
	CHECK(clo_setop_get_max_numel_out(u0, 5, 9) == 14 && clo_setop_get_max_numel_out(u8, 5, 9) == 14
		&& clo_setop_get_max_numel_out(i4, 5, 9) == 5 && clo_setop_get_max_numel_out(i4, 9, 5) == 5
		&& clo_setop_get_max_numel_out(d0, 5, 9) == 5 && clo_setop_get_max_numel_out(d0, 9, 5) == 9, "capacities");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_setop_with_device_data(u4, cq, NULL, ka, va, ((size_t) 1 << 32) - 16, kb, vb, 16, ko, vo, cnt, &err), "n 2^32");
	REFUSED_HOST(clo_setop_with_host_data(u4, cq, NULL, h, hv, (size_t) 1 << 31, g, gv, (size_t) 1 << 31, ho, hvo, &hn, &err), "n 2^32, host");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, NULL, NULL, 16, kb, NULL, 16, ko, NULL, cnt, &err), "keys_a NULL");
	REFUSED_HOST(clo_setop_with_host_data(u0, cq, NULL, h, NULL, 16, NULL, NULL, 16, ho, NULL, &hn, &err), "keys_b NULL, host");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko, NULL, NULL, &err), "num_out NULL");
	REFUSED_HOST(clo_setop_with_host_data(u0, cq, NULL, h, NULL, 16, g, NULL, 16, ho, NULL, NULL, &err), "num_out NULL, host");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko, NULL, cnt_odd, &err), "num_out misaligned");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko, NULL, cnt_small, &err), "num_out of 4 bytes");
	REFUSED_DEV(clo_setop_with_device_data(u4, cq, NULL, ka, va, 16, kb, NULL, 16, ko, vo, cnt, &err), "values_b alone NULL");
	REFUSED_HOST(clo_setop_with_host_data(u4, cq, NULL, h, NULL, 16, g, gv, 16, ho, hvo, &hn, &err), "values_a alone NULL, host");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, va, 16, kb, vb, 16, ko, NULL, cnt, &err), "values with value_size 0");
	REFUSED_HOST(clo_setop_with_host_data(d0, cq, NULL, h, NULL, 16, g, NULL, 16, ho, hvo, &hn, &err), "values_out with value_size 0, host");
	REFUSED_DEV(clo_setop_with_device_data(i4, cq, NULL, ka, va, 16, kb, vb, 16, ko, NULL, cnt, &err), "values_out NULL");
	REFUSED_HOST(clo_setop_with_host_data(u8, cq, NULL, h, NULL, 8, g, NULL, 8, ho, hvo, &hn, &err), "NULL values with value_size 8, host");
	REFUSED_DEV(clo_setop_with_device_data(u8, cq, NULL, ka, NULL, 8, kb, NULL, 8, ko, vo, cnt, &err), "NULL values with value_size 8");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, NULL, NULL, cnt, &err), "both outputs NULL");
	REFUSED_HOST(clo_setop_with_host_data(u4, cq, NULL, h, hv, 16, g, gv, 16, NULL, NULL, &hn, &err), "both outputs NULL, host");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ka, NULL, cnt, &err), "keys_out on keys_a");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko_on_kb, NULL, cnt, &err), "keys_out sharing kb's last element");
	REFUSED_DEV(clo_setop_with_device_data(u4, cq, NULL, ka, va, 16, kb, vb, 16, ko, vo_in_ko, cnt, &err), "values_out inside keys_out");
	REFUSED_DEV(clo_setop_with_device_data(u4, cq, NULL, ka, va, 16, kb, vb, 16, ko, vb, cnt, &err), "values_out on values_b");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko, NULL, cnt_in_ko, &err), "num_out inside keys_out");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko, NULL, cnt_in_ka, &err), "num_out inside keys_a");
	REFUSED_HOST(clo_setop_with_host_data(u4, cq, NULL, h, hv, 16, g, gv, 16, ho, ho + 31, &hn, &err), "values_out on keys_out's last element, host");
	REFUSED_HOST(clo_setop_with_host_data(u0, cq, NULL, ho + 8, NULL, 16, g, NULL, 16, ho, NULL, &hn, &err), "keys_a inside keys_out, host");
	REFUSED_HOST(clo_setop_with_host_data(u0, cq, NULL, h, NULL, 16, g, NULL, 16, ho, NULL, (size_t*) (ho + 30), &err), "num_out inside keys_out, host");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 17, kb, NULL, 16, ko, NULL, cnt, &err), "numel_a beyond the buffer");
	REFUSED_DEV(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko_64, NULL, cnt, &err), "keys_out below a union's capacity");
	/* err == NULL */
	CHECK(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ka, NULL, cnt, NULL) == NULL, "in place, err NULL");
	CHECK(clo_setop_with_device_data(u0, cq, NULL, ka, NULL, 16, kb, NULL, 16, ko, NULL, NULL, NULL) == NULL, "num_out NULL, err NULL");
	CHECK(!clo_setop_with_host_data(u4, NULL, NULL, h, hv, (size_t) 1 << 32, g, gv, 1, ho, hvo, &hn, NULL), "n 2^32, host, err NULL");
	CHECK(!clo_setop_with_host_data(u0, NULL, NULL, h, NULL, 16, g, NULL, 16, NULL, NULL, &hn, NULL), "both outputs NULL, host, err NULL");
	for (int i = 0; i < 40; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	CHECK(hn == 777, "a refused call wrote num_out");
	/* adjacent, disjoint views of one allocation are accepted; an intersection's outputs need min(numel_a, numel_b) only,
	 * and it does not look at values_b: on values_out, or NULL */
	CHECK(clo_setop_with_device_data(u4, cq, NULL, ka, va, 16, kb, vb, 16, ko, vo, cnt, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_setop_with_device_data(i4, cq, NULL, ka, va, 16, kb, NULL, 16, ko_64, vo, cnt, &err) != NULL, "intersection, values_b NULL");
	expect(&err, 0, "intersection, values_b NULL");
	CHECK(clo_setop_with_device_data(i4, cq, NULL, ka, va, 16, kb, vo, 16, ko_64, vo, cnt, &err) != NULL, "intersection, values_b on values_out");
	expect(&err, 0, "intersection, values_b on values_out");
	/* both inputs empty: success, num_out 0, nothing else written, no queue needed in the host form */
	CHECK(clo_setop_with_host_data(u4, NULL, NULL, NULL, NULL, 0, NULL, NULL, 0, ho, hvo, &hn, &err), "both empty, host");
	expect(&err, 0, "both empty, host");
	CHECK(hn == 0, "both empty, host: num_out %zu", hn);
	hn = 777;
	CHECK(clo_setop_with_host_data(i4, NULL, NULL, h, hv, 16, NULL, NULL, 0, ho, hvo, &hn, &err), "intersection with nothing, host");
	expect(&err, 0, "intersection with nothing, host");
	CHECK(hn == 0, "intersection with nothing, host: num_out %zu", hn);
	cl_ulong dn = 777;
	ccl_buffer_enqueue_write(cnt, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	CHECK(clo_setop_with_device_data(u4, cq, NULL, NULL, NULL, 0, NULL, NULL, 0, ko, vo, cnt, &err) != NULL, "both empty, device");
	expect(&err, 0, "both empty, device");
	ccl_buffer_enqueue_read(cnt, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	expect(&err, 0, "read");
	CHECK(dn == 0, "both empty, device: num_out %llu", (unsigned long long) dn);
	for (int i = 0; i < 40; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "an empty call wrote an output at %d", i);

	clo_setop_destroy(u0); clo_setop_destroy(u4); clo_setop_destroy(u8); clo_setop_destroy(i4); clo_setop_destroy(d0);
	CCLBuffer* all[] = { ka, kb, va, vb, ko, vo, cnt, ko_on_kb, vo_in_ko, cnt_in_ko, cnt_in_ka, cnt_odd, cnt_small, ko_64, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType types[] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };
	/* large -> small -> large on one object per op and mode, with an empty side on either hand and both */
	static const size_t sizes[][2] = { { 5000, 3001 }, { 37, 5 }, { 0, 300 }, { 300, 0 }, { 1, 1 }, { 0, 0 }, { 7000, 6000 } };
	for (int op = 0; op < 4; ++op) {
		for (size_t t = 0; t < sizeof(types) / sizeof(types[0]); ++t) {
			for (int mode = KEYS_ONLY; mode <= ARG_ONLY; ++mode) {
				CloSetOp* so = clo_setop_new(op_names[op], NULL, ctx, types[t], mode == KEYS_ONLY ? 0 : mode == VAL8 ? 8 : 4, &err);
				expect(&err, 0, "clo_setop_new");
				if (!so) continue;
				for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z)
					for (int host_form = 0; host_form < 2; ++host_form)
						run_setop(ctx, cq, so, op, types[t], mode, sizes[z][0], sizes[z][1], host_form);
				clo_setop_destroy(so);
			}
		}
	}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("setop host ok\n");
	return failures ? 1 : 0;
}
