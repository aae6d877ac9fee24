/*
 * segscan_host_test.c — CloSegScan (include/clo_segscan.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_segscan_cpu.py). The three ops, both kinds, both
 * forms, both count types and every legal pair of value and sum type; num_in below, equal to and above numel_seg and
 * absent; numel 0, below, equal to and above total (segments clipped, tail rows left alone); all-zero counts and one
 * count that covers everything; offsets with offsets[0] != 0; descending offsets and wrapping sums (the call returns,
 * ASan stays silent); the host-data form; in place; one object used large -> small -> large (its workspace grows once
 * and is reused); every refusal the driver makes (err == NULL included), with the outputs left alone; a clean destroy.
 * The expected rows come from a plain loop over the segments in 64-bit arithmetic.
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

enum { PAT_RANDOM, PAT_ZEROS, PAT_ONE_BIG, PAT_ONES, PAT_COUNT };
enum { NUM_ABSENT, NUM_BELOW, NUM_EQUAL, NUM_ABOVE, NUM_MODES };
enum { ROWS_ZERO, ROWS_BELOW, ROWS_EQUAL, ROWS_ABOVE, ROWS_MODES };
static const char* const op_names[3] = { "sum", "min", "max" };
static const char* const form_names[2] = { "counts", "offsets" };
static const char* const kind_options[2] = { NULL, "inclusive=1" };
static const CloType int_types[4] = { CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG };
static int is_signed(CloType t) { return t == CLO_INT || t == CLO_LONG; }

/* (sum type) value as the bits of a 64-bit word, the low 4 bytes for a 32-bit sum */
static uint64_t value_as_sum(const unsigned char* values, size_t i, CloType vt, CloType st) {
	uint64_t v;
	if (clo_type_sizeof(vt) == 8) memcpy(&v, values + i * 8, 8);
	else {
		uint32_t v4;
		memcpy(&v4, values + i * 4, 4);
		v = is_signed(vt) ? (uint64_t) (int64_t) (int32_t) v4 : v4;
	}
	return clo_type_sizeof(st) == 4 ? (uint32_t) v : v;
}

/* a < b in the sum type */
static int sum_less(uint64_t a, uint64_t b, CloType st) {
	if (!is_signed(st)) return a < b;
	if (clo_type_sizeof(st) == 4) return (int32_t) (uint32_t) a < (int32_t) (uint32_t) b;
	return (int64_t) a < (int64_t) b;
}

/* in_place: the values' array is the output (equal widths only) */
static void run_segscan(CCLContext* ctx, CCLQueue* cq, CloSegScan* ss, int op, int incl, int form, CloType ct, CloType vt, CloType st, int pattern, size_t m_h,
	int num_mode, int rows_mode, uint64_t base, int host_form, int in_place) {
	GError* err = NULL;
	const size_t cs = clo_type_sizeof(ct), vs = clo_type_sizeof(vt), sums = clo_type_sizeof(st);
	if (vs != sums) in_place = 0;
	uint64_t* counts = (uint64_t*) malloc((m_h + 1) * sizeof(uint64_t));
	for (size_t r = 0; r < m_h; ++r)
		counts[r] = pattern == PAT_ZEROS ? 0 : pattern == PAT_ONES ? 1 : pattern == PAT_ONE_BIG ? (r == m_h / 2 ? 5000 : 0) : (rnd() % 3 ? rnd() % 9 : 0);
	size_t num_in = num_mode == NUM_BELOW ? m_h - (m_h + 2) / 3 : num_mode == NUM_ABOVE ? m_h + 7 : m_h;
	const size_t m = num_in < m_h ? num_in : m_h;
	uint64_t total = 0;
	for (size_t r = 0; r < m; ++r) total += counts[r];
	const size_t n = rows_mode == ROWS_ZERO ? 0 : rows_mode == ROWS_BELOW ? (size_t) (total - (total + 3) / 4) : rows_mode == ROWS_EQUAL ? (size_t) total : (size_t) total + 100;
	const size_t rows = total < n ? (size_t) total : n;   /* the rows that are written */
	/* the values: extremes among small numbers, so that wrapped sums and the signed and unsigned orders differ */
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	for (size_t i = 0; i < n * 8 + 8; ++i) hv[i] = (rnd() & 3) ? (unsigned char) (rnd() & 1 ? 0xFF : 0x00) : (unsigned char) rnd();
	/* the expected rows: a plain loop */
	const uint64_t mask = sums == 8 ? ~0ull : 0xffffffffull;
	const uint64_t top = sums == 8 ? 1ull << 63 : 1ull << 31;
	uint64_t* want = (uint64_t*) malloc((n + 1) * sizeof(uint64_t));
	uint64_t at = 0;
	for (size_t r = 0; r < m; ++r) {
		uint64_t acc = op == 0 ? 0 : op == 1 ? (is_signed(st) ? top - 1 : mask) : (is_signed(st) ? top : 0);
		for (uint64_t k = 0; k < counts[r]; ++k, ++at) {
			if (at >= n) continue;
			const uint64_t x = value_as_sum(hv, (size_t) at, vt, st);
			uint64_t after;
			if (op == 0) after = (acc + x) & mask;
			else if (op == 1) after = sum_less(x, acc, st) ? x : acc;
			else after = sum_less(acc, x, st) ? x : acc;
			want[at] = incl ? after : acc;
			acc = after;
		}
	}
	/* the input in the form's layout and the count type */
	const size_t src_n = m_h + (form ? 1 : 0);
	unsigned char* src = (unsigned char*) malloc(src_n * cs + 8);
	uint64_t run = base;
	for (size_t r = 0; r < src_n; ++r) {
		const uint64_t w = form ? run : counts[r];
		if (cs == 8) memcpy(src + r * 8, &w, 8);
		else { const uint32_t w4 = (uint32_t) w; memcpy(src + r * 4, &w4, 4); }
		if (r < m_h) run += counts[r];
	}
	const size_t held = n + 4;   /* rows of the output allocation: the rows past n are checked too */
	unsigned char* got_d = (unsigned char*) malloc(held * 8);
	memset(got_d, 0xEE, held * 8);
	if (in_place) memcpy(got_d, hv, n * vs);
	size_t got = 12345;
	if (host_form) {
		CHECK(clo_segscan_with_host_data(ss, (m_h & 1) ? cq : NULL, NULL, src, num_mode == NUM_ABSENT ? NULL : &num_in, n ? (in_place ? got_d : hv) : NULL,
			n ? got_d : NULL, &got, m_h, n, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[5];   /* counts or offsets, num_in, values, data out, num_out */
		const size_t bytes[5] = { src_n * cs, 8, n * vs, held * sums, 8 };
		cl_ulong count = 12345, dn = num_in;
		for (int i = 0; i < 5; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], src, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, 8, &dn, NULL, &err);
		if (n) ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3], got_d, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "write");
		CCLBuffer* vin = n ? (in_place ? b[3] : b[2]) : NULL;
		CCLEvent* evt = clo_segscan_with_device_data(ss, cq, NULL, b[0], num_mode == NUM_ABSENT ? NULL : b[1], vin, n ? b[3] : NULL, b[4], m_h, n, &err);
		expect(&err, 0, "segscan");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[3], cq, CL_TRUE, 0, bytes[3], got_d, NULL, &err);
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "read");
		got = (size_t) count;
		for (int i = 0; i < 5; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "%s incl %d %s count size %zu value %d sum %d pattern %d m_h %zu num %d rows %d host %d in place %d"
#define WHERE_ARGS op_names[op], incl, form_names[form], cs, (int) vt, (int) st, pattern, m_h, num_mode, rows_mode, host_form, in_place
	CHECK(got == total, WHERE ": num_out = %zu, expected %llu", WHERE_ARGS, got, (unsigned long long) total);
	for (size_t i = 0; i < rows; ++i) {
		uint64_t a = 0;
		memcpy(&a, got_d + i * sums, sums);   /* (little endian) */
		CHECK(a == want[i], WHERE ": data_out[%zu] = %llx, expected %llx", WHERE_ARGS, i, (unsigned long long) a, (unsigned long long) want[i]);
	}
	if (in_place) {   /* the rows at and beyond min(total, n) keep their values */
		CHECK(memcmp(got_d + rows * sums, hv + rows * vs, (n - rows) * vs) == 0, WHERE ": a row beyond the total was written", WHERE_ARGS);
		for (size_t i = n * sums; i < held * sums; ++i) CHECK(got_d[i] == 0xEE, WHERE ": data_out written at byte %zu", WHERE_ARGS, i);
	} else {
		for (size_t i = rows * sums; i < held * sums; ++i) CHECK(got_d[i] == 0xEE, WHERE ": data_out written at byte %zu", WHERE_ARGS, i);
	}
	free(counts); free(want); free(src); free(hv); free(got_d);
}

/* offsets that descend, counts whose sum wraps 2^64, a num_in far above numel_seg: the call returns and ASan sees every
 * access */
static void test_broken_preconditions(CCLQueue* cq, CCLContext* ctx) {
	GError* err = NULL;
	enum { M = 300, N = 5000 };
	for (int which = 0; which < 3; ++which) {
		for (int op = 0; op < 3; ++op) {
			CloSegScan* ss = clo_segscan_new(op_names[op], which == 1 ? "counts" : "offsets", kind_options[op & 1], ctx, CLO_INT, CLO_LONG, CLO_ULONG, &err);
			expect(&err, 0, "clo_segscan_new");
			if (!ss) continue;
			uint64_t src[M + 1];
			int32_t vals[N];
			int64_t out[N];
			for (int r = 0; r <= M; ++r)
				src[r] = which == 0 ? (uint64_t) (M - r) * 20 : which == 1 ? ~0ull / 3 + rnd() : (uint64_t) rnd() % 8000;   /* descending; wrapping; unordered */
			for (int i = 0; i < N; ++i) vals[i] = (int32_t) rnd();
			size_t num_in = (size_t) 1 << 40, total = 0;
			CHECK(clo_segscan_with_host_data(ss, cq, NULL, src, &num_in, vals, out, &total, M, N, &err), "broken preconditions %d", which);
			expect(&err, 0, "broken preconditions");
			clo_segscan_destroy(ss);
		}
	}
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_segscan_new("mean", "counts", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "an unknown op");
	REFUSED_NEW(clo_segscan_new(NULL, "counts", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "a NULL op");
	REFUSED_NEW(clo_segscan_new("Sum", "counts", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "an op in another case");
	REFUSED_NEW(clo_segscan_new("sum", "lengths", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "an unknown form");
	REFUSED_NEW(clo_segscan_new("sum", NULL, NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "a NULL form");
	REFUSED_NEW(clo_segscan_new("sum", "counts", "tile=1024", ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "an unknown option");
	REFUSED_NEW(clo_segscan_new("sum", "counts", "inclusive=2", ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "inclusive=2");
	REFUSED_NEW(clo_segscan_new("sum", "counts", "inclusive", ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "inclusive without a value");
	REFUSED_NEW(clo_segscan_new("sum", "counts", NULL, ctx, CLO_UINT, CLO_UINT, CLO_INT, &err), "count_type int");
	REFUSED_NEW(clo_segscan_new("sum", "offsets", NULL, ctx, CLO_UINT, CLO_UINT, CLO_LONG, &err), "count_type long");
	REFUSED_NEW(clo_segscan_new("sum", "offsets", NULL, ctx, CLO_UINT, CLO_UINT, CLO_FLOAT, &err), "count_type float");
	REFUSED_NEW(clo_segscan_new("sum", "counts", NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_UINT, &err), "float values");
	REFUSED_NEW(clo_segscan_new("max", "counts", NULL, ctx, CLO_UINT, CLO_DOUBLE, CLO_UINT, &err), "double sums");
	REFUSED_NEW(clo_segscan_new("min", "counts", NULL, ctx, CLO_USHORT, CLO_UINT, CLO_UINT, &err), "ushort values");
	REFUSED_NEW(clo_segscan_new("sum", "counts", NULL, ctx, CLO_LONG, CLO_UINT, CLO_UINT, &err), "a sum type narrower than the value type");
	REFUSED_NEW(clo_segscan_new("sum", "counts", NULL, ctx, (CloType) 11, CLO_UINT, CLO_UINT, &err), "an unknown value type");
	REFUSED_NEW(clo_segscan_new("sum", "counts", NULL, NULL, CLO_UINT, CLO_UINT, CLO_UINT, &err), "no context");
	CHECK(clo_segscan_new("avg", "counts", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, NULL) == NULL, "an unknown op, err NULL");
	CHECK(clo_segscan_new("sum", "count", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, NULL) == NULL, "an unknown form, err NULL");
	CHECK(clo_segscan_new("sum", "counts", "exclusive", ctx, CLO_UINT, CLO_UINT, CLO_UINT, NULL) == NULL, "options, err NULL");
	CHECK(clo_segscan_new("sum", "counts", NULL, ctx, CLO_ULONG, CLO_INT, CLO_UINT, NULL) == NULL, "a narrower sum type, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	memset(base, 0, 4096);   /* (the stub's device memory is the host's) */
	/* 16 segments, 16 rows */
	CCLBuffer* cn = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);               /* 16 counts */
	CCLBuffer* of = ccl_buffer_new_from_device_ptr(ctx, base, 68, &err);               /* 17 offsets */
	CCLBuffer* ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* vi = ccl_buffer_new_from_device_ptr(ctx, base + 80, 64, &err);          /* adjacent to ni */
	CCLBuffer* dout = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* dout8 = ccl_buffer_new_from_device_ptr(ctx, base + 1536, 128, &err);    /* 16 rows of 8 bytes */
	CCLBuffer* no = ccl_buffer_new_from_device_ptr(ctx, base + 576, 8, &err);          /* adjacent to dout */
	CCLBuffer* do_on_cn = ccl_buffer_new_from_device_ptr(ctx, base + 60, 64, &err);    /* one shared element with the counts */
	CCLBuffer* do_on_of = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);    /* adjacent to the counts, on the 17th offset */
	CCLBuffer* do_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 76, 64, &err);    /* the second half of num_in */
	CCLBuffer* do_on_vi = ccl_buffer_new_from_device_ptr(ctx, base + 140, 64, &err);   /* the last row of values_in */
	CCLBuffer* do_shift = ccl_buffer_new_from_device_ptr(ctx, base + 84, 64, &err);    /* values_in shifted by one element */
	CCLBuffer* do8_on_vi = ccl_buffer_new_from_device_ptr(ctx, base + 80, 128, &err);  /* at values_in, rows twice as wide */
	CCLBuffer* no_in_do = ccl_buffer_new_from_device_ptr(ctx, base + 568, 8, &err);    /* the last 8 bytes of data_out */
	CCLBuffer* no_in_cn = ccl_buffer_new_from_device_ptr(ctx, base + 8, 8, &err);
	CCLBuffer* no_in_vi = ccl_buffer_new_from_device_ptr(ctx, base + 88, 8, &err);
	CCLBuffer* no_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* no_odd = ccl_buffer_new_from_device_ptr(ctx, base + 708, 8, &err);      /* not 8-byte aligned */
	CCLBuffer* no_small = ccl_buffer_new_from_device_ptr(ctx, base + 712, 4, &err);
	CCLBuffer* ni_odd = ccl_buffer_new_from_device_ptr(ctx, base + 1028, 8, &err);
	CCLBuffer* ni_small = ccl_buffer_new_from_device_ptr(ctx, base + 1032, 4, &err);
	CCLBuffer* cn_short = ccl_buffer_new_from_device_ptr(ctx, base, 60, &err);
	CCLBuffer* vi_short = ccl_buffer_new_from_device_ptr(ctx, base + 80, 60, &err);
	CCLBuffer* do_short = ccl_buffer_new_from_device_ptr(ctx, base + 2048, 60, &err);  /* 15 rows */
	expect(&err, 0, "buffers");
	uint32_t hc[17] = { 0 }, hv[16] = { 0 }, hdo[24];
	for (int i = 0; i < 24; ++i) hdo[i] = 0xABCD0000u + (uint32_t) i;
	size_t hn = 777, hm = 16;
	CloSegScan* c4 = clo_segscan_new("sum", "counts", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err);
	CloSegScan* o4 = clo_segscan_new("min", "offsets", "inclusive=1", ctx, CLO_INT, CLO_INT, CLO_UINT, &err);
	CloSegScan* c8 = clo_segscan_new("max", "counts", "inclusive=0", ctx, CLO_INT, CLO_LONG, CLO_ULONG, &err);
	CloSegScan* e4 = clo_segscan_new("max", "counts", "", ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err);
	expect(&err, 0, "objects");
	if (!c4 || !o4 || !c8 || !e4) return;
	CHECK(clo_segscan_get_context(o4) == ctx && clo_segscan_get_value_type(o4) == CLO_INT && clo_segscan_get_value_size(o4) == 4
		&& clo_segscan_get_sum_type(c8) == CLO_LONG && clo_segscan_get_sum_size(c8) == 8 && clo_segscan_get_sum_size(c4) == 4
		&& clo_segscan_get_value_size(c8) == 4 && clo_segscan_get_count_type(c8) == CLO_ULONG && clo_segscan_get_count_size(c8) == 8
		&& clo_segscan_get_count_size(c4) == 4 && !strcmp(clo_segscan_get_form(c4), "counts") && !strcmp(clo_segscan_get_form(o4), "offsets")
		&& !strcmp(clo_segscan_get_op(c4), "sum") && !strcmp(clo_segscan_get_op(o4), "min") && !strcmp(clo_segscan_get_op(c8), "max")
		&& !clo_segscan_get_inclusive(c4) && clo_segscan_get_inclusive(o4) && !clo_segscan_get_inclusive(c8) && !clo_segscan_get_inclusive(e4), "getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no, (size_t) 1 << 32, 16, &err), "numel_seg 2^32");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no, 16, (size_t) 1 << 32, &err), "numel 2^32");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, NULL, hv, hdo, &hn, (size_t) 1 << 32, 16, &err), "numel_seg 2^32, host");
	REFUSED_HOST(clo_segscan_with_host_data(o4, cq, NULL, hc, NULL, hv, hdo, &hn, 16, (size_t) 1 << 33, &err), "numel 2^33, host");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, NULL, NULL, vi, dout, no, 16, 16, &err), "counts NULL");
	REFUSED_HOST(clo_segscan_with_host_data(o4, cq, NULL, NULL, NULL, hv, hdo, &hn, 16, 16, &err), "offsets NULL, host");
	REFUSED_DEV(clo_segscan_with_device_data(o4, cq, NULL, NULL, NULL, NULL, NULL, no, 0, 0, &err), "offsets NULL with numel_seg 0");
	REFUSED_HOST(clo_segscan_with_host_data(o4, cq, NULL, NULL, NULL, NULL, NULL, &hn, 0, 0, &err), "offsets NULL with numel_seg 0, host");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, NULL, dout, no, 16, 16, &err), "values_in NULL");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, NULL, NULL, hdo, &hn, 16, 16, &err), "values_in NULL, host");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, NULL, NULL, NULL, hdo, &hn, 0, 3, &err), "values_in NULL without a segment, host");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, NULL, no, 16, 16, &err), "data_out NULL");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, NULL, hv, NULL, &hn, 16, 16, &err), "data_out NULL, host");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, NULL, 16, 16, &err), "num_out NULL");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, NULL, hv, hdo, NULL, 16, 16, &err), "num_out NULL, host");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no_odd, 16, 16, &err), "num_out misaligned");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no_small, 16, 16, &err), "num_out of 4 bytes");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, ni_odd, vi, dout, no, 16, 16, &err), "num_in misaligned");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, ni_small, vi, dout, no, 16, 16, &err), "num_in of 4 bytes");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no, 17, 16, &err), "numel_seg beyond the counts");
	REFUSED_DEV(clo_segscan_with_device_data(o4, cq, NULL, cn, NULL, vi, dout, no, 16, 16, &err), "16 offsets for 16 segments");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn_short, NULL, vi, dout, no, 16, 16, &err), "counts below numel_seg");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi_short, dout, no, 16, 16, &err), "values_in below numel rows");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no, 16, 17, &err), "numel beyond values_in");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, do_short, no, 16, 16, &err), "data_out below numel rows");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, ni, vi, do_short, no, 4, 16, &err), "data_out below numel rows, few segments");
	REFUSED_DEV(clo_segscan_with_device_data(c8, cq, NULL, cn, NULL, vi, dout, no, 8, 16, &err), "data_out below numel rows of 8 bytes");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, cn, no, 16, 16, &err), "data_out on the counts");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, do_on_cn, no, 16, 16, &err), "data_out sharing the counts' last element");
	REFUSED_DEV(clo_segscan_with_device_data(o4, cq, NULL, of, NULL, vi, do_on_of, no, 16, 16, &err), "data_out on the last offset");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, ni, vi, do_on_ni, no, 16, 16, &err), "data_out on num_in");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, do_on_vi, no, 16, 16, &err), "data_out on values_in's last row");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, do_shift, no, 16, 16, &err), "data_out on values_in shifted by one element");
	REFUSED_DEV(clo_segscan_with_device_data(c8, cq, NULL, cn, NULL, vi, do8_on_vi, no, 16, 16, &err), "data_out at values_in with a wider sum type");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no_in_do, 16, 16, &err), "num_out inside data_out");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no_in_cn, 16, 16, &err), "num_out inside the counts");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, no_in_vi, 16, 16, &err), "num_out inside values_in");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, vi, no_in_vi, 16, 16, &err), "num_out inside values_in, in place");
	REFUSED_DEV(clo_segscan_with_device_data(c4, cq, NULL, cn, ni, vi, dout, no_on_ni, 16, 16, &err), "num_out on num_in");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hdo + 8, NULL, hv, hdo, &hn, 16, 16, &err), "the counts inside data_out, host");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, NULL, hdo + 7, hdo, &hn, 16, 8, &err), "values_in on data_out's last row, host");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, NULL, hdo + 1, hdo, &hn, 16, 16, &err), "values_in one element into data_out, host");
	REFUSED_HOST(clo_segscan_with_host_data(c8, cq, NULL, hc, NULL, hdo, hdo, &hn, 8, 8, &err), "in place with a wider sum type, host");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, (size_t*) (hdo + 2), hv, hdo, &hn, 16, 16, &err), "num_in inside data_out, host");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, NULL, hv, hdo, (size_t*) (hdo + 14), 16, 16, &err), "num_out inside data_out, host");
	REFUSED_HOST(clo_segscan_with_host_data(c4, cq, NULL, hc, &hn, hv, hdo, &hn, 16, 16, &err), "num_out on num_in, host");
	/* err == NULL */
	CHECK(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, cn, no, 16, 16, NULL) == NULL, "data_out on the counts, err NULL");
	CHECK(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, dout, NULL, 16, 16, NULL) == NULL, "num_out NULL, err NULL");
	CHECK(clo_segscan_with_device_data(c4, cq, NULL, cn, NULL, vi, do_shift, no, 16, 16, NULL) == NULL, "a shifted alias, err NULL");
	CHECK(!clo_segscan_with_host_data(c4, NULL, NULL, hc, NULL, hv, hdo, &hn, (size_t) 1 << 32, 16, NULL), "numel_seg 2^32, host, err NULL");
	CHECK(!clo_segscan_with_host_data(c4, NULL, NULL, hc, NULL, hv, NULL, &hn, 16, 16, NULL), "data_out NULL, host, err NULL");
	for (int i = 0; i < 24; ++i) CHECK(hdo[i] == 0xABCD0000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	CHECK(hn == 777 && hm == 16, "a refused call wrote num_out or num_in");
	for (int i = 0; i < 4096; ++i) CHECK(base[i] == 0, "a refused call wrote device memory at %d", i);
	/* adjacent, disjoint views of one allocation are accepted; so is the exact in-place alias */
	CHECK(clo_segscan_with_device_data(c4, cq, NULL, cn, ni, vi, dout, no, 16, 16, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_segscan_with_device_data(o4, cq, NULL, of, ni, vi, dout, no, 16, 16, &err) != NULL, "disjoint views of one allocation, offsets");
	expect(&err, 0, "disjoint views of one allocation, offsets");
	CHECK(clo_segscan_with_device_data(c4, cq, NULL, cn, ni, vi, vi, no, 16, 16, &err) != NULL, "in place");
	expect(&err, 0, "in place");
	CHECK(clo_segscan_with_device_data(c8, cq, NULL, cn, NULL, vi, dout8, no, 8, 16, &err) != NULL, "a wider sum type in its own buffer");
	expect(&err, 0, "a wider sum type in its own buffer");
	/* m == 0: success, num_out 0, nothing else written, no queue needed in the host form, the counts may be NULL */
	CHECK(clo_segscan_with_host_data(c4, NULL, NULL, NULL, NULL, hv, hdo, &hn, 0, 16, &err), "empty, host");
	expect(&err, 0, "empty, host");
	CHECK(hn == 0, "empty, host: num_out %zu", hn);
	hn = 777; hm = 0;
	CHECK(clo_segscan_with_host_data(o4, NULL, NULL, hc, &hm, hv, hdo, &hn, 16, 16, &err), "num_in 0, host");
	expect(&err, 0, "num_in 0, host");
	CHECK(hn == 0, "num_in 0, host: num_out %zu", hn);
	cl_ulong dn = 777;
	ccl_buffer_enqueue_write(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	CHECK(clo_segscan_with_device_data(c4, cq, NULL, NULL, NULL, vi, dout, no, 0, 16, &err) != NULL, "empty, device");
	expect(&err, 0, "empty, device");
	ccl_buffer_enqueue_read(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	expect(&err, 0, "read");
	CHECK(dn == 0, "empty, device: num_out %llu", (unsigned long long) dn);
	for (int i = 0; i < 24; ++i) CHECK(hdo[i] == 0xABCD0000u + (uint32_t) i, "an empty call wrote an output at %d", i);

	clo_segscan_destroy(c4); clo_segscan_destroy(o4); clo_segscan_destroy(c8); clo_segscan_destroy(e4);
	CCLBuffer* all[] = { cn, of, ni, vi, dout, dout8, no, do_on_cn, do_on_of, do_on_ni, do_on_vi, do_shift, do8_on_vi, no_in_do, no_in_cn, no_in_vi, no_on_ni,
		no_odd, no_small, ni_odd, ni_small, cn_short, vi_short, do_short, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType count_types[2] = { CLO_UINT, CLO_ULONG };
	/* large -> small -> large on one object per op, kind, form, count type and type pair; the patterns, the num_in and
	 * row modes, the two forms of the call and in place take turns */
	static const size_t sizes[] = { 2500, 7, 1, 4000 };
	unsigned turn = 0;
	for (int op = 0; op < 3; ++op) {
		for (int incl = 0; incl < 2; ++incl) {
			for (int form = 0; form < 2; ++form) {
				for (int c = 0; c < 2; ++c) {
					for (int v = 0; v < 4; ++v) {
						for (int s = 0; s < 4; ++s) {
							if (clo_type_sizeof(int_types[s]) < clo_type_sizeof(int_types[v])) continue;
							CloSegScan* ss = clo_segscan_new(op_names[op], form_names[form], kind_options[incl], ctx, int_types[v], int_types[s], count_types[c], &err);
							expect(&err, 0, "clo_segscan_new");
							if (!ss) continue;
							for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z) {
								for (int num_mode = 0; num_mode < NUM_MODES; ++num_mode, ++turn)
									run_segscan(ctx, cq, ss, op, incl, form, count_types[c], int_types[v], int_types[s], (int) (turn % PAT_COUNT), sizes[z], num_mode,
										(int) ((turn / PAT_COUNT) % ROWS_MODES), form ? 12345u * (turn % 3) : 0, (int) ((turn / 7) & 1), (int) ((turn / 3) & 1));
							}
							clo_segscan_destroy(ss);
						}
					}
				}
			}
		}
	}
	/* every pattern x every row mode x both forms of the call x in place or not, once per op and kind */
	for (int op = 0; op < 3; ++op) {
		for (int incl = 0; incl < 2; ++incl) {
			for (int form = 0; form < 2; ++form) {
				CloSegScan* ss = clo_segscan_new(op_names[op], form_names[form], kind_options[incl], ctx, CLO_INT, (op + incl) & 1 ? CLO_LONG : CLO_INT, CLO_UINT, &err);
				expect(&err, 0, "clo_segscan_new");
				for (int pattern = 0; ss && pattern < PAT_COUNT; ++pattern)
					for (int rows_mode = 0; rows_mode < ROWS_MODES; ++rows_mode)
						for (int host_form = 0; host_form < 2; ++host_form)
							for (int in_place = 0; in_place < 2; ++in_place)
								run_segscan(ctx, cq, ss, op, incl, form, CLO_UINT, CLO_INT, (op + incl) & 1 ? CLO_LONG : CLO_INT, pattern, 333,
									(pattern + rows_mode) % NUM_MODES, rows_mode, form ? 777 : 0, host_form, in_place);
				if (ss) clo_segscan_destroy(ss);
			}
		}
	}
	test_broken_preconditions(cq, ctx);
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("segscan host ok\n");
	return failures ? 1 : 0;
}
