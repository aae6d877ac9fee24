/*
 * select_host_test.c — CloSelect (include/clo_select.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_select_cpu.py). Every op, pred and key type;
 * keys only, 4- and 8-byte values, the arg form with and without keys_out, and for "flagged" without keys_in; numel 0;
 * the host-data form; one object used large -> small -> large (its workspace grows once and is reused); every refusal
 * the driver makes (err == NULL included), with the outputs left alone; a clean destroy. The expected rows are computed
 * here from signed / unsigned / sign-magnitude comparisons of the keys, not taken from the stub.
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

/* -1, 0 or 1: how the key with bits x compares with the one with bits y, from the definition: unsigned by bits, signed
 * by value, IEEE by sign and magnitude (negative numbers descend with their magnitude; -0 below +0) */
static int compare_keys(uint64_t x, uint64_t y, size_t ks, int kind) {
	const unsigned bits = 8 * (unsigned) ks;
	const uint64_t all = ks == 8 ? ~0ull : ((1ull << bits) - 1ull), sign = 1ull << (bits - 1);
	x &= all; y &= all;
	if (kind == 0) return x < y ? -1 : x > y;
	const int nx = (x & sign) != 0, ny = (y & sign) != 0;
	if (nx != ny) return nx ? -1 : 1;
	if (kind == 1) return x < y ? -1 : x > y;            /* the same sign: two's complement orders like the bits */
	const uint64_t mx = x & (sign - 1), my = y & (sign - 1);
	if (nx) return mx > my ? -1 : mx < my;
	return mx < my ? -1 : mx > my;
}

static int keeps(int pred, int cmp, unsigned char flag) {
	switch (pred) {
		case 0: return flag != 0;
		case 1: return cmp < 0;
		case 2: return cmp <= 0;
		case 3: return cmp > 0;
		case 4: return cmp >= 0;
		case 5: return cmp == 0;
		default: return cmp != 0;
	}
}

enum { KEYS_ONLY, VAL4, VAL8, ARG, ARG_ONLY, ARG_NO_KEYS };   /* the last: "flagged" alone, keys_in NULL */
static const char* const op_names[2] = { "select", "partition" };
static const char* const pred_names[7] = { "flagged", "lt", "le", "gt", "ge", "eq", "ne" };

static void run_select(CCLContext* ctx, CCLQueue* cq, CloSelect* sel, int op, int pred, CloType kt, int mode, size_t n, int host_form) {
	GError* err = NULL;
	const size_t ks = clo_type_sizeof(kt), vs = mode == KEYS_ONLY ? 0 : mode == VAL8 ? 8 : 4;
	const int kind = kind_of(kt), vals = mode == VAL4 || mode == VAL8, keys_out = mode != ARG_ONLY && mode != ARG_NO_KEYS;
	unsigned char* hk = (unsigned char*) malloc(n * ks + 8);
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	unsigned char* hf = (unsigned char*) malloc(n + 8);
	uint64_t* bits = (uint64_t*) malloc((n + 1) * sizeof(uint64_t));
	/* few distinct keys around the type's sign change; the threshold is one of them; flags with values other than 0 / 1 */
	for (size_t i = 0; i <= n; ++i) {
		uint64_t b = (uint64_t) (rnd() % 23) - 11u;   /* -11 .. 11 as two's complement */
		if (kind == 2) b = (rnd() & 1 ? 1ull << (8 * ks - 1) : 0ull) | (rnd() % 7);   /* +-0 and small denormals */
		bits[i] = ks == 8 ? b : b & ((1ull << (8 * ks)) - 1ull);
	}
	uint64_t thr = bits[n];
	for (size_t i = 0; i < n; ++i) {
		const uint64_t v = ((uint64_t) rnd() << 32) | rnd();
		memcpy(hk + i * ks, &bits[i], ks);
		memcpy(hv + i * vs, &v, vs);
		hf[i] = (unsigned char) (rnd() % 3 ? 0 : 1 + rnd() % 255);
	}
	/* the expected rows */
	uint32_t* want_p = (uint32_t*) malloc((n + 1) * sizeof(uint32_t));
	size_t k = 0, rows = 0;
	for (int side = 0; side <= op; ++side) {
		for (size_t i = 0; i < n; ++i)
			if (keeps(pred, pred ? compare_keys(bits[i], thr, ks, kind) : 0, hf[i]) == (side == 0)) want_p[rows++] = (uint32_t) i;
		if (side == 0) k = rows;
	}
	unsigned char* got_k = (unsigned char*) malloc(n * ks + 8);
	unsigned char* got_v = (unsigned char*) malloc(n * 8 + 8);
	memset(got_k, 0xEE, n * ks + 8);
	memset(got_v, 0xEE, n * 8 + 8);
	size_t got = 12345;
	const void* fot = pred == 0 ? (const void*) hf : (const void*) &thr;   /* little-endian: the key's bytes come first */
	if (host_form) {
		CHECK(clo_select_with_host_data(sel, (n & 1) ? cq : NULL, NULL, mode == ARG_NO_KEYS ? NULL : hk, vals ? hv : NULL, fot,
			keys_out ? got_k : NULL, vs ? got_v : NULL, n, &got, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[6];   /* keys, values, flags or threshold, keys out, values out, the count */
		const size_t fot_bytes = pred == 0 ? n : ks;
		const size_t bytes[6] = { n * ks, n * vs, fot_bytes, n * ks, n * vs, 8 };
		cl_ulong count = 12345;
		for (int i = 0; i < 6; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], hk, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, bytes[1], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], (void*) fot, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3] + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, bytes[4] + 8, got_v, NULL, &err);
		ccl_buffer_enqueue_write(b[5], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_select_with_device_data(sel, cq, NULL, mode == ARG_NO_KEYS ? NULL : b[0], vals ? b[1] : NULL, b[2],
			keys_out ? b[3] : NULL, vs ? b[4] : NULL, b[5], n, &err);
		expect(&err, 0, "select");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[3], cq, CL_TRUE, 0, bytes[3] + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, bytes[4] + 8, got_v, NULL, &err);
		ccl_buffer_enqueue_read(b[5], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "read");
		got = (size_t) count;
		for (int i = 0; i < 6; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "%s %s key type %d mode %d n %zu host %d"
#define WHERE_ARGS op_names[op], pred_names[pred], (int) kt, mode, n, host_form
	CHECK(got == k, WHERE ": k = %zu, expected %zu", WHERE_ARGS, got, k);
	for (size_t j = 0; j < rows; ++j) {
		const size_t i = want_p[j];
		if (keys_out) CHECK(memcmp(got_k + j * ks, hk + i * ks, ks) == 0, WHERE ": wrong key in row %zu", WHERE_ARGS, j);
		if (vals) CHECK(memcmp(got_v + j * vs, hv + i * vs, vs) == 0, WHERE ": wrong value in row %zu", WHERE_ARGS, j);
		else if (vs) CHECK(memcmp(got_v + j * 4, &want_p[j], 4) == 0, WHERE ": wrong index in row %zu", WHERE_ARGS, j);
	}
	for (size_t i = keys_out ? rows * ks : 0; i < n * ks + 8; ++i) CHECK(got_k[i] == 0xEE, WHERE ": keys_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = rows * vs; i < n * 8 + 8; ++i) CHECK(got_v[i] == 0xEE, WHERE ": values_out written at byte %zu", WHERE_ARGS, i);
	free(hk); free(hv); free(hf); free(bits); free(want_p); free(got_k); free(got_v);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_select_new("select", "lt", NULL, ctx, CLO_UINT, 2, &err), "value_size 2");
	REFUSED_NEW(clo_select_new("select", "lt", NULL, ctx, CLO_UINT, 16, &err), "value_size 16");
	REFUSED_NEW(clo_select_new("select", "lt", "descending", ctx, CLO_UINT, 0, &err), "options");
	REFUSED_NEW(clo_select_new("select", "lt", NULL, ctx, (CloType) 11, 0, &err), "an unknown key type");
	REFUSED_NEW(clo_select_new("filter", "lt", NULL, ctx, CLO_UINT, 0, &err), "an unknown op");
	REFUSED_NEW(clo_select_new(NULL, "lt", NULL, ctx, CLO_UINT, 0, &err), "a NULL op");
	REFUSED_NEW(clo_select_new("Select", "lt", NULL, ctx, CLO_UINT, 0, &err), "an op in another case");
	REFUSED_NEW(clo_select_new("select", "less", NULL, ctx, CLO_UINT, 0, &err), "an unknown pred");
	REFUSED_NEW(clo_select_new("select", NULL, NULL, ctx, CLO_UINT, 0, &err), "a NULL pred");
	REFUSED_NEW(clo_select_new("partition", "LT", NULL, ctx, CLO_UINT, 0, &err), "a pred in another case");
	CHECK(clo_select_new("select", "lt", NULL, ctx, CLO_UINT, 3, NULL) == NULL, "value_size 3, err NULL");
	CHECK(clo_select_new("selec", "lt", NULL, ctx, CLO_UINT, 4, NULL) == NULL, "an unknown op, err NULL");
	CHECK(clo_select_new("select", "l", NULL, ctx, CLO_UINT, 4, NULL) == NULL, "an unknown pred, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* ki = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);
	CCLBuffer* vi = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);          /* adjacent to ki */
	CCLBuffer* fl = ccl_buffer_new_from_device_ptr(ctx, base + 128, 16, &err);         /* 16 flags */
	CCLBuffer* th = ccl_buffer_new_from_device_ptr(ctx, base + 144, 4, &err);          /* one uint, adjacent to fl */
	CCLBuffer* ko = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* vo = ccl_buffer_new_from_device_ptr(ctx, base + 576, 64, &err);         /* adjacent to ko */
	CCLBuffer* cnt = ccl_buffer_new_from_device_ptr(ctx, base + 640, 8, &err);         /* adjacent to vo */
	CCLBuffer* ko_on_ki = ccl_buffer_new_from_device_ptr(ctx, base + 60, 64, &err);    /* one shared element with ki */
	CCLBuffer* ko_on_fl = ccl_buffer_new_from_device_ptr(ctx, base + 140, 64, &err);   /* the flags' last four bytes */
	CCLBuffer* ko_on_th = ccl_buffer_new_from_device_ptr(ctx, base + 84, 64, &err);    /* ends on the threshold */
	CCLBuffer* vo_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 572, 64, &err);   /* starts on ko's last ROW (row 15 of numel, whatever k is) */
	CCLBuffer* cnt_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 568, 8, &err);   /* the last 8 bytes of ko */
	CCLBuffer* cnt_in_ki = ccl_buffer_new_from_device_ptr(ctx, base + 8, 8, &err);
	CCLBuffer* cnt_on_th = ccl_buffer_new_from_device_ptr(ctx, base + 144, 8, &err);
	CCLBuffer* cnt_odd = ccl_buffer_new_from_device_ptr(ctx, base + 644, 8, &err);     /* not 8-byte aligned */
	CCLBuffer* cnt_small = ccl_buffer_new_from_device_ptr(ctx, base + 648, 4, &err);
	CCLBuffer* fl_short = ccl_buffer_new_from_device_ptr(ctx, base + 128, 15, &err);
	CCLBuffer* th_short = ccl_buffer_new_from_device_ptr(ctx, base + 144, 2, &err);
	CCLBuffer* ko_short = ccl_buffer_new_from_device_ptr(ctx, base + 1024, 60, &err);  /* 15 rows: below numel even where k is small */
	expect(&err, 0, "buffers");
	uint32_t h[16] = { 0 }, hv[16] = { 0 }, ho[24], hvo[24], t = 5;
	unsigned char f[16] = { 0 };
	for (int i = 0; i < 24; ++i) { ho[i] = 0xABCD0000u + (uint32_t) i; hvo[i] = 0x12340000u + (uint32_t) i; }
	size_t hn = 777;
	CloSelect* s0 = clo_select_new("select", "lt", NULL, ctx, CLO_UINT, 0, &err);
	CloSelect* s4 = clo_select_new("select", "ge", "", ctx, CLO_UINT, 4, &err);
	CloSelect* p8 = clo_select_new("partition", "eq", NULL, ctx, CLO_UINT, 8, &err);
	CloSelect* f0 = clo_select_new("select", "flagged", NULL, ctx, CLO_UINT, 0, &err);
	CloSelect* f4 = clo_select_new("partition", "flagged", NULL, ctx, CLO_UINT, 4, &err);
	expect(&err, 0, "objects");
	if (!s0 || !s4 || !p8 || !f0 || !f4) return;
	CHECK(clo_select_get_context(s4) == ctx && clo_select_get_key_type(s4) == CLO_UINT && clo_select_get_key_size(s4) == 4
		&& clo_select_get_value_size(s4) == 4 && clo_select_get_value_size(s0) == 0 && clo_select_get_value_size(p8) == 8
		&& !strcmp(clo_select_get_op(p8), "partition") && !strcmp(clo_select_get_op(f0), "select")
		&& !strcmp(clo_select_get_pred(p8), "eq") && !strcmp(clo_select_get_pred(f4), "flagged"), "getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, cnt, (size_t) 1 << 32, &err), "numel 2^32");
	REFUSED_HOST(clo_select_with_host_data(s4, cq, NULL, h, hv, &t, ho, hvo, (size_t) 1 << 32, &hn, &err), "numel 2^32, host");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, NULL, NULL, th, ko, NULL, cnt, 16, &err), "keys_in NULL for a comparison");
	REFUSED_HOST(clo_select_with_host_data(f0, cq, NULL, NULL, NULL, f, ho, NULL, 16, &hn, &err), "keys_in NULL with keys_out, host");
	REFUSED_DEV(clo_select_with_device_data(s4, cq, NULL, NULL, NULL, th, NULL, vo, cnt, 16, &err), "keys_in NULL, comparison in arg form");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, NULL, ko, NULL, cnt, 16, &err), "threshold NULL");
	REFUSED_HOST(clo_select_with_host_data(f0, cq, NULL, h, NULL, NULL, ho, NULL, 16, &hn, &err), "flags NULL, host");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, NULL, 16, &err), "num_out NULL");
	REFUSED_HOST(clo_select_with_host_data(s0, cq, NULL, h, NULL, &t, ho, NULL, 16, NULL, &err), "num_out NULL, host");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, cnt_odd, 16, &err), "num_out misaligned");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, cnt_small, 16, &err), "num_out of 4 bytes");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, vi, th, ko, NULL, cnt, 16, &err), "values with value_size 0");
	REFUSED_HOST(clo_select_with_host_data(f0, cq, NULL, h, NULL, f, ho, hvo, 16, &hn, &err), "values_out with value_size 0, host");
	REFUSED_DEV(clo_select_with_device_data(s4, cq, NULL, ki, vi, th, ko, NULL, cnt, 16, &err), "values_out NULL");
	REFUSED_HOST(clo_select_with_host_data(p8, cq, NULL, h, NULL, &t, ho, hvo, 8, &hn, &err), "NULL values with value_size 8, host");
	REFUSED_DEV(clo_select_with_device_data(p8, cq, NULL, ki, NULL, th, ko, vo, cnt, 8, &err), "NULL values with value_size 8");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, NULL, NULL, cnt, 16, &err), "both outputs NULL");
	REFUSED_HOST(clo_select_with_host_data(s4, cq, NULL, h, hv, &t, NULL, NULL, 16, &hn, &err), "both outputs NULL, host");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ki, NULL, cnt, 16, &err), "in place");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko_on_ki, NULL, cnt, 16, &err), "keys_out sharing keys_in's last element");
	REFUSED_DEV(clo_select_with_device_data(f0, cq, NULL, ki, NULL, fl, ko_on_fl, NULL, cnt, 16, &err), "keys_out on the flags' end");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko_on_th, NULL, cnt, 16, &err), "keys_out's last row on the threshold");
	REFUSED_DEV(clo_select_with_device_data(s4, cq, NULL, ki, vi, th, ko, vo_in_ko, cnt, 16, &err), "values_out on keys_out's row numel - 1");
	REFUSED_DEV(clo_select_with_device_data(s4, cq, NULL, ki, vi, th, ko, vi, cnt, 16, &err), "values_out on values_in");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, cnt_in_ko, 16, &err), "num_out inside keys_out");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, cnt_in_ki, 16, &err), "num_out inside keys_in");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, cnt_on_th, 16, &err), "num_out on the threshold");
	REFUSED_HOST(clo_select_with_host_data(s4, cq, NULL, h, hv, &t, ho, ho + 15, 16, &hn, &err), "values_out on keys_out's last row, host");
	REFUSED_HOST(clo_select_with_host_data(s0, cq, NULL, ho + 8, NULL, &t, ho, NULL, 16, &hn, &err), "keys_in inside keys_out, host");
	REFUSED_HOST(clo_select_with_host_data(s0, cq, NULL, h, NULL, ho + 3, ho, NULL, 16, &hn, &err), "the threshold inside keys_out, host");
	REFUSED_HOST(clo_select_with_host_data(s0, cq, NULL, h, NULL, &t, ho, NULL, 16, (size_t*) (ho + 14), &err), "num_out inside keys_out, host");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, cnt, 17, &err), "numel beyond the buffers");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko_short, NULL, cnt, 16, &err), "keys_out below numel rows");
	REFUSED_DEV(clo_select_with_device_data(f0, cq, NULL, ki, NULL, fl_short, ko, NULL, cnt, 16, &err), "flags below numel bytes");
	REFUSED_DEV(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th_short, ko, NULL, cnt, 16, &err), "a threshold below one key");
	/* err == NULL */
	CHECK(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ki, NULL, cnt, 16, NULL) == NULL, "in place, err NULL");
	CHECK(clo_select_with_device_data(s0, cq, NULL, ki, NULL, th, ko, NULL, NULL, 16, NULL) == NULL, "num_out NULL, err NULL");
	CHECK(!clo_select_with_host_data(s4, NULL, NULL, h, hv, &t, ho, hvo, (size_t) 1 << 32, &hn, NULL), "numel 2^32, host, err NULL");
	CHECK(!clo_select_with_host_data(s0, NULL, NULL, h, NULL, &t, NULL, NULL, 16, &hn, NULL), "both outputs NULL, host, err NULL");
	for (int i = 0; i < 24; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	CHECK(hn == 777, "a refused call wrote num_out");
	/* adjacent, disjoint views of one allocation are accepted */
	CHECK(clo_select_with_device_data(s4, cq, NULL, ki, vi, th, ko, vo, cnt, 16, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_select_with_device_data(f4, cq, NULL, NULL, NULL, fl, NULL, vo, cnt, 16, &err) != NULL, "flagged, indices alone");
	expect(&err, 0, "flagged, indices alone");
	/* numel 0: success, num_out 0, nothing else written, no queue needed in the host form, inputs may be NULL */
	CHECK(clo_select_with_host_data(s4, NULL, NULL, NULL, NULL, &t, ho, hvo, 0, &hn, &err), "empty, host");
	expect(&err, 0, "empty, host");
	CHECK(hn == 0, "empty, host: num_out %zu", hn);
	hn = 777;
	CHECK(clo_select_with_host_data(f4, NULL, NULL, NULL, NULL, NULL, ho, hvo, 0, &hn, &err), "empty flagged, host");
	expect(&err, 0, "empty flagged, host");
	CHECK(hn == 0, "empty flagged, host: num_out %zu", hn);
	cl_ulong dn = 777;
	ccl_buffer_enqueue_write(cnt, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	CHECK(clo_select_with_device_data(s4, cq, NULL, NULL, NULL, th, ko, vo, cnt, 0, &err) != NULL, "empty, device");
	expect(&err, 0, "empty, device");
	ccl_buffer_enqueue_read(cnt, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	expect(&err, 0, "read");
	CHECK(dn == 0, "empty, device: num_out %llu", (unsigned long long) dn);
	for (int i = 0; i < 24; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "an empty call wrote an output at %d", i);

	clo_select_destroy(s0); clo_select_destroy(s4); clo_select_destroy(p8); clo_select_destroy(f0); clo_select_destroy(f4);
	CCLBuffer* all[] = { ki, vi, fl, th, ko, vo, cnt, ko_on_ki, ko_on_fl, ko_on_th, vo_in_ko, cnt_in_ko, cnt_in_ki, cnt_on_th, cnt_odd, cnt_small,
		fl_short, th_short, ko_short, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType types[] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };
	/* large -> small -> large on one object per op, pred, type and mode, with numel 0 in between */
	static const size_t sizes[] = { 9001, 37, 0, 1, 12000 };
	for (int op = 0; op < 2; ++op) {
		for (int pred = 0; pred < 7; ++pred) {
			for (size_t t = 0; t < sizeof(types) / sizeof(types[0]); ++t) {
				for (int mode = KEYS_ONLY; mode <= (pred == 0 ? ARG_NO_KEYS : ARG_ONLY); ++mode) {
					CloSelect* sel = clo_select_new(op_names[op], pred_names[pred], NULL, ctx, types[t], mode == KEYS_ONLY ? 0 : mode == VAL8 ? 8 : 4, &err);
					expect(&err, 0, "clo_select_new");
					if (!sel) continue;
					for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z)
						for (int host_form = 0; host_form < 2; ++host_form)
							run_select(ctx, cq, sel, op, pred, types[t], mode, sizes[z], host_form);
					clo_select_destroy(sel);
				}
			}
		}
	}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("select host ok\n");
	return failures ? 1 : 0;
}
