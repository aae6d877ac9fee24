/*
 * join_host_test.c — CloJoin (include/clo_join.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_join_cpu.py). Every kind and key type; the count
 * form; K above, at and below the capacity; an empty side, both sides empty; the device and the host-data form; one
 * object used large -> small -> large (its workspace grows once and is reused); every refusal the driver makes (err
 * == NULL included), with the outputs left alone; a clean destroy. The expected rows are computed here from the sorted
 * concatenation and the counts of every group of equal keys, not taken from the stub.
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

/* the bits of a key as an unsigned number in the join's order */
static uint64_t order_key(uint64_t bits, size_t ks, int kind) {
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	bits &= all;
	if (kind == 1) return bits ^ sign;
	if (kind == 2) return (bits & sign) ? bits ^ all : bits ^ sign;
	return bits;
}

typedef struct { uint64_t ord, bits; uint32_t index; } elem;

static int by_order(const void* x, const void* y) {
	const elem* a = (const elem*) x; const elem* b = (const elem*) y;
	if (a->ord != b->ord) return a->ord < b->ord ? -1 : 1;
	return a->index < b->index ? -1 : a->index > b->index;
}

/* n sorted keys drawn from `distinct` values around the type's sign change (so that runs occur in both inputs, and keys
 * of one input alone) */
static void make_side(elem* e, size_t n, size_t ks, int kind, uint32_t first_index, uint32_t distinct) {
	for (size_t i = 0; i < n; ++i) {
		uint64_t bits = (uint64_t) (rnd() % distinct) - distinct / 2;   /* as two's complement */
		if (kind == 2) bits = (rnd() & 1 ? 1ull << (8 * ks - 1) : 0ull) | (rnd() % distinct);   /* +-0 and small denormals */
		e[i].bits = ks == 8 ? bits : bits & ((1ull << (8 * ks)) - 1ull);
		e[i].ord = order_key(bits, ks, kind);
		e[i].index = 0;
	}
	qsort(e, n, sizeof(elem), by_order);   /* (all indices 0: any order among equal keys; their bits are equal) */
	for (size_t i = 0; i < n; ++i) e[i].index = first_index + (uint32_t) i;
}

static const char* const kind_names[4] = { "inner", "left", "right", "full" };
#define NONE CLO_JOIN_NONE

/* e[0, n): A || B sorted by (key, index). The first min(K, cap) rows into ia, ib, bits; returns K. */
static uint64_t want_rows(const elem* e, size_t n, size_t na, int kind, size_t cap, uint32_t* ia, uint32_t* ib, uint64_t* bits) {
	uint64_t k = 0;
	const int emits_a = kind == 1 || kind == 3, emits_b = kind == 2 || kind == 3;
#define ROW(x, y) do { if (k < cap) { ia[k] = (x); ib[k] = (y); bits[k] = e[g].bits; } ++k; } while (0)
	for (size_t g = 0; g < n;) {
		size_t end = g, m = 0;
		while (end < n && e[end].ord == e[g].ord) { if (e[end].index < na) ++m; ++end; }
		const size_t c = end - g - m;   /* the A rows are e[g, g + m), the B rows e[g + m, end) */
		if (m > 0 && c > 0) {
			for (size_t i = 0; i < m; ++i) for (size_t j = 0; j < c; ++j) ROW(e[g + i].index, e[g + m + j].index - (uint32_t) na);
		} else if (m > 0) {
			for (size_t i = 0; emits_a && i < m; ++i) ROW(e[g + i].index, NONE);
		} else {
			for (size_t j = 0; emits_b && j < c; ++j) ROW(NONE, e[g + j].index - (uint32_t) na);
		}
		g = end;
	}
#undef ROW
	return k;
}

/* cap_mode: 0 the count form, 1 K - 1 rows (or 0), 2 exactly K, 3 K + 7 */
static void run_join(CCLContext* ctx, CCLQueue* cq, CloJoin* jn, int kind, CloType kt, size_t na, size_t nb, uint32_t distinct, int cap_mode, int host_form) {
	GError* err = NULL;
	const size_t ks = clo_type_sizeof(kt), n = na + nb;
	const int kk = kind_of(kt);
	elem* e = (elem*) malloc((n + 1) * sizeof(elem));
	make_side(e, na, ks, kk, 0, distinct);
	make_side(e + na, nb, ks, kk, (uint32_t) na, distinct);
	unsigned char* hk = (unsigned char*) malloc(n * ks + 8);
	for (size_t i = 0; i < n; ++i) memcpy(hk + i * ks, &e[i].bits, ks);
	qsort(e, n, sizeof(elem), by_order);   /* by key, ties by index in A || B: the merge order */
	uint32_t dummy_i[1]; uint64_t dummy_b[1];
	const uint64_t K = want_rows(e, n, na, kind, 0, dummy_i, dummy_i, dummy_b);
	CHECK(K <= clo_join_get_max_numel_out(jn, na, nb), "%s of %zu and %zu: %llu rows above the bound", kind_names[kind], na, nb, (unsigned long long) K);
	const size_t cap = cap_mode == 0 ? 0 : cap_mode == 1 ? (K > 0 ? (size_t) K - 1 : 0) : cap_mode == 2 ? (size_t) K : (size_t) K + 7;
	const size_t rows = K < cap ? (size_t) K : cap;
	uint32_t* want_a = (uint32_t*) malloc((cap + 2) * 4);
	uint32_t* want_b = (uint32_t*) malloc((cap + 2) * 4);
	uint64_t* want_bits = (uint64_t*) malloc((cap + 2) * 8);
	want_rows(e, n, na, kind, cap, want_a, want_b, want_bits);
	uint32_t* got_a = (uint32_t*) malloc((cap + 2) * 4);
	uint32_t* got_b = (uint32_t*) malloc((cap + 2) * 4);
	unsigned char* got_k = (unsigned char*) malloc((cap + 2) * ks);
	memset(got_a, 0xEE, (cap + 2) * 4);
	memset(got_b, 0xEE, (cap + 2) * 4);
	memset(got_k, 0xEE, (cap + 2) * ks);
	/* which outputs are given: all of them, or (other sizes) one dropped; none in the count form */
	const int give_a = cap_mode != 0 && (n % 3 != 1), give_b = cap_mode != 0 && (n % 3 != 2 || !give_a), give_k = cap_mode != 0 && (n % 5 != 0);
	uint64_t got = 12345;
	if (host_form) {
		size_t hn = 12345;
		CHECK(clo_join_with_host_data(jn, (na & 1) ? cq : NULL, NULL, hk, na, hk + na * ks, nb,
			give_a ? got_a : NULL, give_b ? got_b : NULL, give_k ? got_k : NULL, cap, &hn, &err), "host data");
		expect(&err, 0, "host data");
		got = hn;
	} else {
		CCLBuffer* b[6];   /* keys a, keys b, idx a, idx b, keys out, the count */
		const size_t bytes[6] = { na * ks, nb * ks, cap * 4, cap * 4, cap * ks, 8 };
		cl_ulong count = 12345;
		for (int i = 0; i < 6; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], hk, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, bytes[1], hk + na * ks, NULL, &err);
		ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2] + 8, got_a, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3] + 8, got_b, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, bytes[4] + ks, got_k, NULL, &err);
		ccl_buffer_enqueue_write(b[5], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_join_with_device_data(jn, cq, NULL, na ? b[0] : NULL, na, nb ? b[1] : NULL, nb,
			give_a ? b[2] : NULL, give_b ? b[3] : NULL, give_k ? b[4] : NULL, cap, b[5], &err);
		expect(&err, 0, "join");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[2], cq, CL_TRUE, 0, bytes[2] + 8, got_a, NULL, &err);
		ccl_buffer_enqueue_read(b[3], cq, CL_TRUE, 0, bytes[3] + 8, got_b, NULL, &err);
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, bytes[4] + ks, got_k, NULL, &err);
		ccl_buffer_enqueue_read(b[5], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "read");
		got = count;
		for (int i = 0; i < 6; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "%s key type %d %zu and %zu, capacity %zu of %llu, host %d"
#define WHERE_ARGS kind_names[kind], (int) kt, na, nb, cap, (unsigned long long) K, host_form
	CHECK(got == K, WHERE ": num_out %llu", WHERE_ARGS, (unsigned long long) got);
	if (give_a) CHECK(memcmp(got_a, want_a, rows * 4) == 0, WHERE ": wrong idx_a", WHERE_ARGS);
	if (give_b) CHECK(memcmp(got_b, want_b, rows * 4) == 0, WHERE ": wrong idx_b", WHERE_ARGS);
	if (give_k) for (size_t i = 0; i < rows; ++i) CHECK(memcmp(got_k + i * ks, &want_bits[i], ks) == 0, WHERE ": wrong key at row %zu", WHERE_ARGS, i);
	const unsigned char* ga = (const unsigned char*) got_a; const unsigned char* gb = (const unsigned char*) got_b;
	for (size_t i = give_a ? rows * 4 : 0; i < (cap + 2) * 4; ++i) CHECK(ga[i] == 0xEE, WHERE ": idx_a_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = give_b ? rows * 4 : 0; i < (cap + 2) * 4; ++i) CHECK(gb[i] == 0xEE, WHERE ": idx_b_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = give_k ? rows * ks : 0; i < (cap + 2) * ks; ++i) CHECK(got_k[i] == 0xEE, WHERE ": keys_out written at byte %zu", WHERE_ARGS, i);
	free(e); free(hk); free(want_a); free(want_b); free(want_bits); free(got_a); free(got_b); free(got_k);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_join_new("inner", "descending", ctx, CLO_UINT, &err), "options");
	REFUSED_NEW(clo_join_new("inner", NULL, ctx, (CloType) 11, &err), "an unknown key type");
	REFUSED_NEW(clo_join_new("outer", NULL, ctx, CLO_UINT, &err), "an unknown kind");
	REFUSED_NEW(clo_join_new(NULL, NULL, ctx, CLO_UINT, &err), "a NULL kind");
	REFUSED_NEW(clo_join_new("Inner", NULL, ctx, CLO_UINT, &err), "a kind in another case");
	REFUSED_NEW(clo_join_new("inner", NULL, NULL, CLO_UINT, &err), "no context");
	CHECK(clo_join_new("semi", NULL, ctx, CLO_UINT, NULL) == NULL, "an unknown kind, err NULL");
	CHECK(clo_join_new("left", "x", ctx, CLO_UINT, NULL) == NULL, "options, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* ka = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);
	CCLBuffer* kb = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);         /* adjacent to ka */
	CCLBuffer* ia = ccl_buffer_new_from_device_ptr(ctx, base + 256, 128, &err);       /* 32 rows each */
	CCLBuffer* ib = ccl_buffer_new_from_device_ptr(ctx, base + 384, 128, &err);       /* adjacent to ia */
	CCLBuffer* ko = ccl_buffer_new_from_device_ptr(ctx, base + 512, 128, &err);       /* adjacent to ib */
	CCLBuffer* cnt = ccl_buffer_new_from_device_ptr(ctx, base + 640, 8, &err);        /* adjacent to ko */
	CCLBuffer* ia_on_kb = ccl_buffer_new_from_device_ptr(ctx, base + 124, 128, &err); /* one shared element with kb */
	CCLBuffer* ib_in_ia = ccl_buffer_new_from_device_ptr(ctx, base + 380, 128, &err); /* starts on ia's last element */
	CCLBuffer* cnt_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 632, 8, &err);  /* the last 8 bytes of ko */
	CCLBuffer* cnt_in_ka = ccl_buffer_new_from_device_ptr(ctx, base + 8, 8, &err);
	CCLBuffer* cnt_odd = ccl_buffer_new_from_device_ptr(ctx, base + 652, 8, &err);    /* not 8-byte aligned */
	CCLBuffer* cnt_small = ccl_buffer_new_from_device_ptr(ctx, base + 656, 4, &err);
	expect(&err, 0, "buffers");
	uint32_t h[16] = { 0 }, g[16] = { 0 }, hia[40], hib[40], hko[40];
	for (int i = 0; i < 40; ++i) { hia[i] = 0xABCD0000u + (uint32_t) i; hib[i] = 0x12340000u + (uint32_t) i; hko[i] = 0x77770000u + (uint32_t) i; }
	size_t hn = 777;
	CloJoin* in = clo_join_new("inner", NULL, ctx, CLO_UINT, &err);
	CloJoin* fu = clo_join_new("full", "", ctx, CLO_UINT, &err);
	CloJoin* le = clo_join_new("left", NULL, ctx, CLO_DOUBLE, &err);
	CloJoin* ri = clo_join_new("right", NULL, ctx, CLO_UCHAR, &err);
	expect(&err, 0, "objects");
	if (!in || !fu || !le || !ri) return;
	CHECK(clo_join_get_context(fu) == ctx && clo_join_get_key_type(fu) == CLO_UINT && clo_join_get_key_size(fu) == 4
		&& clo_join_get_key_type(le) == CLO_DOUBLE && clo_join_get_key_size(le) == 8 && clo_join_get_key_size(ri) == 1
		&& !strcmp(clo_join_get_kind(in), "inner") && !strcmp(clo_join_get_kind(le), "left") && !strcmp(clo_join_get_kind(ri), "right")
		&& !strcmp(clo_join_get_kind(fu), "full"), "getters");
	CHECK(clo_join_get_max_numel_out(in, 5, 9) == 45 && clo_join_get_max_numel_out(in, 0, 9) == 0 && clo_join_get_max_numel_out(le, 5, 0) == 5
		&& clo_join_get_max_numel_out(le, 0, 5) == 0 && clo_join_get_max_numel_out(ri, 0, 5) == 5 && clo_join_get_max_numel_out(fu, 1, 1) == 2
		&& clo_join_get_max_numel_out(fu, 2, 1) == 3 && clo_join_get_max_numel_out(fu, 3, 3) == 9 && clo_join_get_max_numel_out(le, 3, 1) == 3
		&& clo_join_get_max_numel_out(in, (size_t) 1 << 40, (size_t) 1 << 40) == SIZE_MAX
		&& clo_join_get_max_numel_out(fu, SIZE_MAX, SIZE_MAX) == SIZE_MAX && clo_join_get_max_numel_out(fu, SIZE_MAX, 0) == SIZE_MAX, "upper bounds");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, ((size_t) 1 << 32) - 16, kb, 16, ia, ib, ko, 32, cnt, &err), "n 2^32");
	REFUSED_HOST(clo_join_with_host_data(in, cq, NULL, h, (size_t) 1 << 31, g, (size_t) 1 << 31, hia, hib, hko, 32, &hn, &err), "n 2^32, host");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, ko, (size_t) 1 << 32, cnt, &err), "capacity 2^32");
	REFUSED_HOST(clo_join_with_host_data(fu, cq, NULL, h, 16, g, 16, hia, hib, hko, (size_t) 1 << 32, &hn, &err), "capacity 2^32, host");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, NULL, 16, kb, 16, ia, ib, ko, 32, cnt, &err), "keys_a NULL");
	REFUSED_HOST(clo_join_with_host_data(in, cq, NULL, h, 16, NULL, 16, hia, hib, hko, 32, &hn, &err), "keys_b NULL, host");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, ko, 32, NULL, &err), "num_out NULL");
	REFUSED_HOST(clo_join_with_host_data(in, cq, NULL, h, 16, g, 16, hia, hib, hko, 32, NULL, &err), "num_out NULL, host");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, ko, 32, cnt_odd, &err), "num_out misaligned");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, ko, 32, cnt_small, &err), "num_out of 4 bytes");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, NULL, NULL, NULL, 32, cnt, &err), "a capacity and no output");
	REFUSED_HOST(clo_join_with_host_data(fu, cq, NULL, h, 16, g, 16, NULL, NULL, NULL, 1, &hn, &err), "a capacity and no output, host");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ka, ib, ko, 16, cnt, &err), "idx_a_out on keys_a");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia_on_kb, ib, ko, 32, cnt, &err), "idx_a_out sharing kb's last element");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib_in_ia, ko, 32, cnt, &err), "idx_b_out on idx_a_out's last element");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ia, NULL, 32, cnt, &err), "idx_b_out on idx_a_out");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, kb, 16, cnt, &err), "keys_out on keys_b");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, ko, 32, cnt_in_ko, &err), "num_out inside keys_out");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, ko, 32, cnt_in_ka, &err), "num_out inside keys_a");
	REFUSED_HOST(clo_join_with_host_data(in, cq, NULL, h, 16, g, 16, hia, hia + 31, hko, 32, &hn, &err), "idx_b_out on idx_a_out's last element, host");
	REFUSED_HOST(clo_join_with_host_data(in, cq, NULL, hia + 8, 16, g, 16, hia, hib, hko, 32, &hn, &err), "keys_a inside idx_a_out, host");
	REFUSED_HOST(clo_join_with_host_data(in, cq, NULL, h, 16, g, 16, hia, hib, hko, 32, (size_t*) (hko + 30), &err), "num_out inside keys_out, host");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 17, kb, 16, ia, ib, ko, 32, cnt, &err), "numel_a beyond the buffer");
	REFUSED_DEV(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, ko, 33, cnt, &err), "a capacity beyond the outputs");
	/* err == NULL */
	CHECK(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ka, ib, ko, 16, cnt, NULL) == NULL, "on an input, err NULL");
	CHECK(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ia, ib, ko, 32, NULL, NULL) == NULL, "num_out NULL, err NULL");
	CHECK(!clo_join_with_host_data(in, NULL, NULL, h, (size_t) 1 << 32, g, 1, hia, hib, hko, 32, &hn, NULL), "n 2^32, host, err NULL");
	CHECK(!clo_join_with_host_data(in, NULL, NULL, h, 16, g, 16, NULL, NULL, NULL, 5, &hn, NULL), "a capacity and no output, host, err NULL");
	for (int i = 0; i < 40; ++i) CHECK(hia[i] == 0xABCD0000u + (uint32_t) i && hib[i] == 0x12340000u + (uint32_t) i && hko[i] == 0x77770000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	CHECK(hn == 777, "a refused call wrote num_out");
	/* adjacent, disjoint views of one allocation are accepted; an output at capacity 0 has no bytes and overlaps nothing */
	CHECK(clo_join_with_device_data(fu, cq, NULL, ka, 16, kb, 16, ia, ib, ko, 32, cnt, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_join_with_device_data(in, cq, NULL, ka, 16, kb, 16, ka, NULL, NULL, 0, cnt, &err) != NULL, "capacity 0");
	expect(&err, 0, "capacity 0");
	/* both inputs empty: success, num_out 0, nothing else written, no queue needed in the host form */
	CHECK(clo_join_with_host_data(fu, NULL, NULL, NULL, 0, NULL, 0, hia, hib, hko, 32, &hn, &err), "both empty, host");
	expect(&err, 0, "both empty, host");
	CHECK(hn == 0, "both empty, host: num_out %zu", hn);
	cl_ulong dn = 777;
	ccl_buffer_enqueue_write(cnt, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	CHECK(clo_join_with_device_data(fu, cq, NULL, NULL, 0, NULL, 0, ia, ib, ko, 32, cnt, &err) != NULL, "both empty, device");
	expect(&err, 0, "both empty, device");
	ccl_buffer_enqueue_read(cnt, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	expect(&err, 0, "read");
	CHECK(dn == 0, "both empty, device: num_out %llu", (unsigned long long) dn);
	for (int i = 0; i < 40; ++i) CHECK(hia[i] == 0xABCD0000u + (uint32_t) i && hib[i] == 0x12340000u + (uint32_t) i && hko[i] == 0x77770000u + (uint32_t) i, "an empty call wrote an output at %d", i);

	clo_join_destroy(in); clo_join_destroy(fu); clo_join_destroy(le); clo_join_destroy(ri);
	CCLBuffer* all[] = { ka, kb, ia, ib, ko, cnt, ia_on_kb, ib_in_ia, cnt_in_ko, cnt_in_ka, cnt_odd, cnt_small, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType types[] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };
	/* large -> small -> large on one object per kind and type, with an empty side on either hand and both; keys from
	 * `distinct` values: many short runs, or a few long ones */
	static const size_t sizes[][3] = { { 5000, 3001, 4001 }, { 37, 5, 9 }, { 0, 300, 50 }, { 300, 0, 50 }, { 1, 1, 1 }, { 0, 0, 1 }, { 900, 700, 23 }, { 7000, 6000, 9001 } };
	for (int kind = 0; kind < 4; ++kind) {
		for (size_t t = 0; t < sizeof(types) / sizeof(types[0]); ++t) {
			CloJoin* jn = clo_join_new(kind_names[kind], NULL, ctx, types[t], &err);
			expect(&err, 0, "clo_join_new");
			if (!jn) continue;
			for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z)
				for (int cap_mode = 0; cap_mode < 4; ++cap_mode)
					run_join(ctx, cq, jn, kind, types[t], sizes[z][0], sizes[z][1], (uint32_t) sizes[z][2], cap_mode, (int) ((z + cap_mode) & 1));
			clo_join_destroy(jn);
		}
	}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("join host ok\n");
	return failures ? 1 : 0;
}
