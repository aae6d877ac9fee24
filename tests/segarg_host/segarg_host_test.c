/*
 * segarg_host_test.c — CloSegArg (include/clo_segarg.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_segarg_cpu.py). Both ops, both ties, both forms,
 * both count types and the six value types; num_in below, equal to and above numel_seg and absent; numel below, equal to
 * and above total (segments clipped in the middle and clipped away); all-zero counts and one count that covers
 * everything; offsets with offsets[0] != 0; descending offsets (the call returns, ASan stays silent); val_out absent;
 * the host-data form; one object used large -> small -> large (its workspace grows once and is reused); every refusal
 * the driver makes (err == NULL included), with the outputs left alone; a clean destroy. The expected rows come from a
 * plain loop over the segments that compares signed integers, and floats as sign and magnitude.
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
static const char* const op_names[2] = { "argmin", "argmax" };
static const char* const tie_names[2] = { "first", "last" };
static const char* const form_names[2] = { "counts", "offsets" };
static const CloType value_types[6] = { CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_FLOAT, CLO_DOUBLE };

static uint64_t bits_at(const unsigned char* values, size_t i, size_t vs) {
	uint64_t v = 0;
	memcpy(&v, values + i * vs, vs);   /* (little endian) */
	return v;
}

/* -1, 0, 1: a before, equal to, after b in the type's order; floats in the IEEE total order, as sign and magnitude */
static int order(uint64_t a, uint64_t b, CloType t) {
	const int wide = clo_type_sizeof(t) == 8;
	if (t == CLO_UINT || t == CLO_ULONG) return a < b ? -1 : a > b;
	int64_t x = wide ? (int64_t) a : (int64_t) (int32_t) (uint32_t) a, y = wide ? (int64_t) b : (int64_t) (int32_t) (uint32_t) b;
	if (t == CLO_FLOAT || t == CLO_DOUBLE) {
		/* the sign bit set: the magnitude is x - lowest, and the larger it is the earlier the number comes; -0.0, magnitude 0,
		 * becomes -1, just before +0.0 */
		const int64_t lowest = wide ? INT64_MIN : (int64_t) INT32_MIN;
		if (x < 0) x = (lowest - x) - 1;
		if (y < 0) y = (lowest - y) - 1;
	}
	return x < y ? -1 : x > y;
}

static void run_segarg(CCLContext* ctx, CCLQueue* cq, CloSegArg* sa, int op, int tie, int form, CloType ct, CloType vt, int pattern, size_t m_h,
	int num_mode, int rows_mode, uint64_t base, int host_form, int with_val) {
	GError* err = NULL;
	const size_t cs = clo_type_sizeof(ct), vs = clo_type_sizeof(vt);
	uint64_t* counts = (uint64_t*) malloc((m_h + 1) * sizeof(uint64_t));
	for (size_t r = 0; r < m_h; ++r)
		counts[r] = pattern == PAT_ZEROS ? 0 : pattern == PAT_ONES ? 1 : pattern == PAT_ONE_BIG ? (r == m_h / 2 ? 5000 : 0) : (rnd() % 3 ? rnd() % 9 : 0);
	size_t num_in = num_mode == NUM_BELOW ? m_h - (m_h + 2) / 3 : num_mode == NUM_ABOVE ? m_h + 7 : m_h;
	const size_t m = num_in < m_h ? num_in : m_h;
	uint64_t total = 0;
	for (size_t r = 0; r < m; ++r) total += counts[r];
	const size_t n = rows_mode == ROWS_ZERO ? 0 : rows_mode == ROWS_BELOW ? (size_t) (total - (total + 3) / 4) : rows_mode == ROWS_EQUAL ? (size_t) total : (size_t) total + 100;
	/* the values: bytes that are mostly 0x00 or 0xFF, so that ties, extremes, infinities' neighbours and NaNs of both signs abound */
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	for (size_t i = 0; i < n * 8 + 8; ++i) hv[i] = (rnd() & 3) ? (unsigned char) (rnd() & 1 ? 0xFF : 0x00) : (unsigned char) (rnd() & 1 ? 0x7F : 0x80);
	/* the expected rows: a plain loop */
	uint32_t* want_i = (uint32_t*) malloc((m + 1) * sizeof(uint32_t));
	uint64_t* want_v = (uint64_t*) malloc((m + 1) * sizeof(uint64_t));
	uint64_t at = 0;
	for (size_t r = 0; r < m; ++r) {
		uint32_t best = CLO_SEGARG_NONE;
		for (uint64_t k = 0; k < counts[r]; ++k, ++at) {
			if (at >= n) continue;
			if (best == CLO_SEGARG_NONE) { best = (uint32_t) at; continue; }
			int c = order(bits_at(hv, (size_t) at, vs), bits_at(hv, best, vs), vt);
			if (op == 1) c = -c;
			if (c < 0 || (c == 0 && tie == 1)) best = (uint32_t) at;
		}
		want_i[r] = best;
		if (best != CLO_SEGARG_NONE) want_v[r] = bits_at(hv, best, vs);
		else {
			const uint64_t ones = vs == 8 ? ~0ull : 0xffffffffull, top = vs == 8 ? 1ull << 63 : 1ull << 31;
			want_v[r] = (vt == CLO_UINT || vt == CLO_ULONG) ? (op ? 0 : ones) : (vt == CLO_INT || vt == CLO_LONG) ? (op ? top : top - 1) : (op ? ones : top - 1);
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
	const size_t held = m_h + 4;   /* rows of the output allocations: the rows past m are checked too */
	unsigned char* got_i = (unsigned char*) malloc(held * 4);
	unsigned char* got_v = (unsigned char*) malloc(held * 8);
	memset(got_i, 0xEE, held * 4);
	memset(got_v, 0xEE, held * 8);
	size_t got = 12345;
	if (host_form) {
		CHECK(clo_segarg_with_host_data(sa, (m_h & 1) ? cq : NULL, NULL, src, num_mode == NUM_ABSENT ? NULL : &num_in, n ? hv : NULL,
			(cl_uint*) got_i, with_val ? got_v : NULL, &got, m_h, n, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[6];   /* counts or offsets, num_in, values, idx out, val out, num_out */
		const size_t bytes[6] = { src_n * cs, 8, n * vs, held * 4, held * vs, 8 };
		cl_ulong count = 12345, dn = num_in;
		for (int i = 0; i < 6; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], src, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, 8, &dn, NULL, &err);
		if (n) ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3], got_i, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, bytes[4], got_v, NULL, &err);
		ccl_buffer_enqueue_write(b[5], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_segarg_with_device_data(sa, cq, NULL, b[0], num_mode == NUM_ABSENT ? NULL : b[1], n ? b[2] : NULL, b[3], with_val ? b[4] : NULL,
			b[5], m_h, n, &err);
		expect(&err, 0, "segarg");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[3], cq, CL_TRUE, 0, bytes[3], got_i, NULL, &err);
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, bytes[4], got_v, NULL, &err);
		ccl_buffer_enqueue_read(b[5], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "read");
		got = (size_t) count;
		for (int i = 0; i < 6; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "%s %s %s count size %zu value %d pattern %d m_h %zu num %d rows %d host %d val %d"
#define WHERE_ARGS op_names[op], tie_names[tie], form_names[form], cs, (int) vt, pattern, m_h, num_mode, rows_mode, host_form, with_val
	CHECK(got == total, WHERE ": num_out = %zu, expected %llu", WHERE_ARGS, got, (unsigned long long) total);
	for (size_t r = 0; r < m; ++r) {
		uint32_t i4;
		memcpy(&i4, got_i + r * 4, 4);
		CHECK(i4 == want_i[r], WHERE ": idx_out[%zu] = %u, expected %u", WHERE_ARGS, r, i4, want_i[r]);
		if (with_val) {
			const uint64_t v = bits_at(got_v, r, vs);
			CHECK(v == want_v[r], WHERE ": val_out[%zu] = %llx, expected %llx", WHERE_ARGS, r, (unsigned long long) v, (unsigned long long) want_v[r]);
		}
	}
	for (size_t i = m * 4; i < held * 4; ++i) CHECK(got_i[i] == 0xEE, WHERE ": idx_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = with_val ? m * vs : 0; i < held * 8; ++i) CHECK(got_v[i] == 0xEE, WHERE ": val_out written at byte %zu", WHERE_ARGS, i);
	free(counts); free(want_i); free(want_v); free(src); free(hv); free(got_i); free(got_v);
}

/* offsets that descend, counts whose sum wraps 2^64, a num_in far above numel_seg: the call returns and ASan sees every
 * access */
static void test_broken_preconditions(CCLQueue* cq, CCLContext* ctx) {
	GError* err = NULL;
	enum { M = 300, N = 5000 };
	for (int which = 0; which < 3; ++which) {
		for (int op = 0; op < 2; ++op) {
			CloSegArg* sa = clo_segarg_new(op_names[op], tie_names[which & 1], which == 1 ? "counts" : "offsets", NULL, ctx, CLO_DOUBLE, CLO_ULONG, &err);
			expect(&err, 0, "clo_segarg_new");
			if (!sa) continue;
			uint64_t src[M + 1];
			uint64_t vals[N];
			uint32_t out_i[M];
			uint64_t out_v[M];
			for (int r = 0; r <= M; ++r)
				src[r] = which == 0 ? (uint64_t) (M - r) * 20 : which == 1 ? ~0ull / 3 + rnd() : (uint64_t) rnd() % 8000;   /* descending; wrapping; unordered */
			for (int i = 0; i < N; ++i) vals[i] = ((uint64_t) rnd() << 32) | rnd();
			size_t num_in = (size_t) 1 << 40, total = 0;
			CHECK(clo_segarg_with_host_data(sa, cq, NULL, src, &num_in, vals, out_i, out_v, &total, M, N, &err), "broken preconditions %d", which);
			expect(&err, 0, "broken preconditions");
			clo_segarg_destroy(sa);
		}
	}
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_segarg_new("min", "first", "counts", NULL, ctx, CLO_UINT, CLO_UINT, &err), "an unknown op");
	REFUSED_NEW(clo_segarg_new(NULL, "first", "counts", NULL, ctx, CLO_UINT, CLO_UINT, &err), "a NULL op");
	REFUSED_NEW(clo_segarg_new("Argmin", "first", "counts", NULL, ctx, CLO_UINT, CLO_UINT, &err), "an op in another case");
	REFUSED_NEW(clo_segarg_new("argmin", "any", "counts", NULL, ctx, CLO_UINT, CLO_UINT, &err), "an unknown tie");
	REFUSED_NEW(clo_segarg_new("argmin", NULL, "counts", NULL, ctx, CLO_UINT, CLO_UINT, &err), "a NULL tie");
	REFUSED_NEW(clo_segarg_new("argmin", "first", "lengths", NULL, ctx, CLO_UINT, CLO_UINT, &err), "an unknown form");
	REFUSED_NEW(clo_segarg_new("argmin", "first", NULL, NULL, ctx, CLO_UINT, CLO_UINT, &err), "a NULL form");
	REFUSED_NEW(clo_segarg_new("argmin", "first", "counts", "tile=1024", ctx, CLO_UINT, CLO_UINT, &err), "options");
	REFUSED_NEW(clo_segarg_new("argmin", "first", "counts", NULL, ctx, CLO_UINT, CLO_INT, &err), "count_type int");
	REFUSED_NEW(clo_segarg_new("argmin", "first", "offsets", NULL, ctx, CLO_UINT, CLO_LONG, &err), "count_type long");
	REFUSED_NEW(clo_segarg_new("argmin", "first", "offsets", NULL, ctx, CLO_UINT, CLO_FLOAT, &err), "count_type float");
	REFUSED_NEW(clo_segarg_new("argmax", "last", "counts", NULL, ctx, CLO_HALF, CLO_UINT, &err), "half values");
	REFUSED_NEW(clo_segarg_new("argmax", "last", "counts", NULL, ctx, CLO_USHORT, CLO_UINT, &err), "ushort values");
	REFUSED_NEW(clo_segarg_new("argmax", "last", "counts", NULL, ctx, CLO_CHAR, CLO_UINT, &err), "char values");
	REFUSED_NEW(clo_segarg_new("argmin", "first", "counts", NULL, ctx, (CloType) 11, CLO_UINT, &err), "an unknown value type");
	REFUSED_NEW(clo_segarg_new("argmin", "first", "counts", NULL, NULL, CLO_UINT, CLO_UINT, &err), "no context");
	CHECK(clo_segarg_new("arg", "first", "counts", NULL, ctx, CLO_UINT, CLO_UINT, NULL) == NULL, "an unknown op, err NULL");
	CHECK(clo_segarg_new("argmin", "middle", "counts", NULL, ctx, CLO_UINT, CLO_UINT, NULL) == NULL, "an unknown tie, err NULL");
	CHECK(clo_segarg_new("argmin", "first", "count", NULL, ctx, CLO_UINT, CLO_UINT, NULL) == NULL, "an unknown form, err NULL");
	CHECK(clo_segarg_new("argmin", "first", "counts", NULL, ctx, CLO_HALF, CLO_UINT, NULL) == NULL, "half values, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	memset(base, 0, 4096);   /* (the stub's device memory is the host's) */
	/* 16 segments, 16 rows */
	CCLBuffer* cn = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);               /* 16 counts */
	CCLBuffer* of = ccl_buffer_new_from_device_ptr(ctx, base, 68, &err);               /* 17 offsets */
	CCLBuffer* ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* vi = ccl_buffer_new_from_device_ptr(ctx, base + 80, 64, &err);          /* adjacent to ni */
	CCLBuffer* io = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* no = ccl_buffer_new_from_device_ptr(ctx, base + 576, 8, &err);          /* adjacent to io */
	CCLBuffer* vo = ccl_buffer_new_from_device_ptr(ctx, base + 584, 64, &err);         /* adjacent to no */
	CCLBuffer* vo8 = ccl_buffer_new_from_device_ptr(ctx, base + 1536, 128, &err);
	CCLBuffer* io_on_cn = ccl_buffer_new_from_device_ptr(ctx, base + 60, 64, &err);    /* one shared element with the counts */
	CCLBuffer* io_on_of = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);    /* adjacent to the counts, on the 17th offset */
	CCLBuffer* io_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 76, 64, &err);    /* the second half of num_in */
	CCLBuffer* io_on_vi = ccl_buffer_new_from_device_ptr(ctx, base + 140, 64, &err);   /* the last row of values_in */
	CCLBuffer* vo_on_io = ccl_buffer_new_from_device_ptr(ctx, base + 572, 64, &err);   /* the last row of idx_out */
	CCLBuffer* no_in_io = ccl_buffer_new_from_device_ptr(ctx, base + 568, 8, &err);    /* the last 8 bytes of idx_out */
	CCLBuffer* no_in_vo = ccl_buffer_new_from_device_ptr(ctx, base + 584, 8, &err);    /* the first 8 bytes of val_out */
	CCLBuffer* no_in_cn = ccl_buffer_new_from_device_ptr(ctx, base + 8, 8, &err);
	CCLBuffer* no_in_vi = ccl_buffer_new_from_device_ptr(ctx, base + 88, 8, &err);
	CCLBuffer* no_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* no_odd = ccl_buffer_new_from_device_ptr(ctx, base + 708, 8, &err);      /* not 8-byte aligned */
	CCLBuffer* no_small = ccl_buffer_new_from_device_ptr(ctx, base + 712, 4, &err);
	CCLBuffer* ni_odd = ccl_buffer_new_from_device_ptr(ctx, base + 1028, 8, &err);
	CCLBuffer* ni_small = ccl_buffer_new_from_device_ptr(ctx, base + 1032, 4, &err);
	CCLBuffer* cn_short = ccl_buffer_new_from_device_ptr(ctx, base, 60, &err);
	CCLBuffer* vi_short = ccl_buffer_new_from_device_ptr(ctx, base + 80, 60, &err);
	CCLBuffer* io_short = ccl_buffer_new_from_device_ptr(ctx, base + 2048, 60, &err);  /* 15 rows: below numel_seg even where num_in is small */
	CCLBuffer* vo_short = ccl_buffer_new_from_device_ptr(ctx, base + 2560, 60, &err);
	expect(&err, 0, "buffers");
	uint32_t hc[17] = { 0 }, hv[16] = { 0 }, hio[24], hvo[24];
	for (int i = 0; i < 24; ++i) { hio[i] = 0xABCD0000u + (uint32_t) i; hvo[i] = 0xDCBA0000u + (uint32_t) i; }
	size_t hn = 777, hm = 16;
	CloSegArg* c4 = clo_segarg_new("argmin", "first", "counts", NULL, ctx, CLO_UINT, CLO_UINT, &err);
	CloSegArg* o4 = clo_segarg_new("argmax", "last", "offsets", "", ctx, CLO_FLOAT, CLO_UINT, &err);
	CloSegArg* c8 = clo_segarg_new("argmax", "first", "counts", NULL, ctx, CLO_DOUBLE, CLO_ULONG, &err);
	expect(&err, 0, "objects");
	if (!c4 || !o4 || !c8) return;
	CHECK(clo_segarg_get_context(o4) == ctx && clo_segarg_get_value_type(o4) == CLO_FLOAT && clo_segarg_get_value_size(o4) == 4
		&& clo_segarg_get_value_type(c8) == CLO_DOUBLE && clo_segarg_get_value_size(c8) == 8 && clo_segarg_get_count_type(c8) == CLO_ULONG
		&& clo_segarg_get_count_size(c8) == 8 && clo_segarg_get_count_size(c4) == 4 && !strcmp(clo_segarg_get_form(c4), "counts")
		&& !strcmp(clo_segarg_get_form(o4), "offsets") && !strcmp(clo_segarg_get_op(c4), "argmin") && !strcmp(clo_segarg_get_op(o4), "argmax")
		&& !strcmp(clo_segarg_get_tie(c4), "first") && !strcmp(clo_segarg_get_tie(o4), "last"), "getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no, (size_t) 1 << 32, 16, &err), "numel_seg 2^32");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no, 16, (size_t) 1 << 32, &err), "numel 2^32");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, NULL, hv, hio, hvo, &hn, (size_t) 1 << 32, 16, &err), "numel_seg 2^32, host");
	REFUSED_HOST(clo_segarg_with_host_data(o4, cq, NULL, hc, NULL, hv, hio, hvo, &hn, 16, (size_t) 1 << 33, &err), "numel 2^33, host");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, NULL, NULL, vi, io, vo, no, 16, 16, &err), "counts NULL");
	REFUSED_HOST(clo_segarg_with_host_data(o4, cq, NULL, NULL, NULL, hv, hio, hvo, &hn, 16, 16, &err), "offsets NULL, host");
	REFUSED_DEV(clo_segarg_with_device_data(o4, cq, NULL, NULL, NULL, NULL, NULL, NULL, no, 0, 0, &err), "offsets NULL with numel_seg 0");
	REFUSED_HOST(clo_segarg_with_host_data(o4, cq, NULL, NULL, NULL, NULL, NULL, NULL, &hn, 0, 0, &err), "offsets NULL with numel_seg 0, host");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, NULL, io, vo, no, 16, 16, &err), "values_in NULL");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, NULL, NULL, hio, hvo, &hn, 16, 16, &err), "values_in NULL, host");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, NULL, vo, no, 16, 16, &err), "idx_out NULL");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, NULL, hv, NULL, hvo, &hn, 16, 16, &err), "idx_out NULL, host");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, NULL, 16, 16, &err), "num_out NULL");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, NULL, hv, hio, hvo, NULL, 16, 16, &err), "num_out NULL, host");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no_odd, 16, 16, &err), "num_out misaligned");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no_small, 16, 16, &err), "num_out of 4 bytes");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, ni_odd, vi, io, vo, no, 16, 16, &err), "num_in misaligned");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, ni_small, vi, io, vo, no, 16, 16, &err), "num_in of 4 bytes");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no, 17, 16, &err), "numel_seg beyond the counts");
	REFUSED_DEV(clo_segarg_with_device_data(o4, cq, NULL, cn, NULL, vi, io, vo, no, 16, 16, &err), "16 offsets for 16 segments");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn_short, NULL, vi, io, vo, no, 16, 16, &err), "counts below numel_seg");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi_short, io, vo, no, 16, 16, &err), "values_in below numel rows");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no, 16, 17, &err), "numel beyond values_in");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io_short, vo, no, 16, 16, &err), "idx_out below numel_seg rows");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, ni, vi, io_short, NULL, no, 16, 16, &err), "idx_out below numel_seg rows, with num_in");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo_short, no, 16, 16, &err), "val_out below numel_seg rows");
	REFUSED_DEV(clo_segarg_with_device_data(c8, cq, NULL, vo8, NULL, NULL, io, vo, no, 16, 0, &err), "val_out below numel_seg rows of 8 bytes");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, cn, vo, no, 16, 16, &err), "idx_out on the counts");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, cn, no, 16, 16, &err), "val_out on the counts");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io_on_cn, vo, no, 16, 16, &err), "idx_out sharing the counts' last element");
	REFUSED_DEV(clo_segarg_with_device_data(o4, cq, NULL, of, NULL, vi, io_on_of, vo, no, 16, 16, &err), "idx_out on the last offset");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, ni, vi, io_on_ni, vo, no, 16, 16, &err), "idx_out on num_in");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io_on_vi, vo, no, 16, 16, &err), "idx_out on values_in's last row");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, io_on_vi, no, 16, 16, &err), "val_out on values_in's last row");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, vi, vo, no, 16, 16, &err), "idx_out on values_in");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vi, no, 16, 16, &err), "val_out on values_in");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, io, no, 16, 16, &err), "val_out on idx_out");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo_on_io, no, 16, 16, &err), "val_out on idx_out's last row");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no_in_io, 16, 16, &err), "num_out inside idx_out");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no_in_vo, 16, 16, &err), "num_out inside val_out");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no_in_cn, 16, 16, &err), "num_out inside the counts");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, no_in_vi, 16, 16, &err), "num_out inside values_in");
	REFUSED_DEV(clo_segarg_with_device_data(c4, cq, NULL, cn, ni, vi, io, vo, no_on_ni, 16, 16, &err), "num_out on num_in");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hio + 8, NULL, hv, hio, hvo, &hn, 16, 16, &err), "the counts inside idx_out, host");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, NULL, hvo + 15, hio, hvo, &hn, 16, 8, &err), "values_in on val_out's last row, host");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, (size_t*) (hio + 2), hv, hio, hvo, &hn, 16, 16, &err), "num_in inside idx_out, host");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, NULL, hv, hio, hvo, (size_t*) (hvo + 14), 16, 16, &err), "num_out inside val_out, host");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, NULL, hv, hio, (void*) (hio + 15), &hn, 16, 16, &err), "val_out on idx_out's last row, host");
	REFUSED_HOST(clo_segarg_with_host_data(c4, cq, NULL, hc, &hn, hv, hio, hvo, &hn, 16, 16, &err), "num_out on num_in, host");
	/* err == NULL */
	CHECK(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, cn, vo, no, 16, 16, NULL) == NULL, "idx_out on the counts, err NULL");
	CHECK(clo_segarg_with_device_data(c4, cq, NULL, cn, NULL, vi, io, vo, NULL, 16, 16, NULL) == NULL, "num_out NULL, err NULL");
	CHECK(!clo_segarg_with_host_data(c4, NULL, NULL, hc, NULL, hv, hio, hvo, &hn, (size_t) 1 << 32, 16, NULL), "numel_seg 2^32, host, err NULL");
	CHECK(!clo_segarg_with_host_data(c4, NULL, NULL, hc, NULL, hv, NULL, hvo, &hn, 16, 16, NULL), "idx_out NULL, host, err NULL");
	for (int i = 0; i < 24; ++i) CHECK(hio[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0xDCBA0000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	CHECK(hn == 777 && hm == 16, "a refused call wrote num_out or num_in");
	for (int i = 0; i < 4096; ++i) CHECK(base[i] == 0, "a refused call wrote device memory at %d", i);
	/* adjacent, disjoint views of one allocation are accepted */
	CHECK(clo_segarg_with_device_data(c4, cq, NULL, cn, ni, vi, io, vo, no, 16, 16, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_segarg_with_device_data(o4, cq, NULL, of, ni, vi, io, NULL, no, 16, 16, &err) != NULL, "disjoint views of one allocation, offsets, no val_out");
	expect(&err, 0, "disjoint views of one allocation, offsets, no val_out");
	/* m == 0: success, num_out 0, nothing else written, no queue needed in the host form, inputs may be NULL */
	CHECK(clo_segarg_with_host_data(c4, NULL, NULL, NULL, NULL, hv, NULL, NULL, &hn, 0, 16, &err), "empty, host");
	expect(&err, 0, "empty, host");
	CHECK(hn == 0, "empty, host: num_out %zu", hn);
	hn = 777; hm = 0;
	CHECK(clo_segarg_with_host_data(o4, NULL, NULL, hc, &hm, hv, hio, hvo, &hn, 16, 16, &err), "num_in 0, host");
	expect(&err, 0, "num_in 0, host");
	CHECK(hn == 0, "num_in 0, host: num_out %zu", hn);
	cl_ulong dn = 777;
	ccl_buffer_enqueue_write(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	CHECK(clo_segarg_with_device_data(c4, cq, NULL, NULL, NULL, vi, NULL, NULL, no, 0, 16, &err) != NULL, "empty, device");
	expect(&err, 0, "empty, device");
	ccl_buffer_enqueue_read(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	expect(&err, 0, "read");
	CHECK(dn == 0, "empty, device: num_out %llu", (unsigned long long) dn);
	for (int i = 0; i < 24; ++i) CHECK(hio[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0xDCBA0000u + (uint32_t) i, "an empty call wrote an output at %d", i);

	clo_segarg_destroy(c4); clo_segarg_destroy(o4); clo_segarg_destroy(c8);
	CCLBuffer* all[] = { cn, of, ni, vi, io, no, vo, vo8, io_on_cn, io_on_of, io_on_ni, io_on_vi, vo_on_io, no_in_io, no_in_vo, no_in_cn, no_in_vi, no_on_ni,
		no_odd, no_small, ni_odd, ni_small, cn_short, vi_short, io_short, vo_short, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType count_types[2] = { CLO_UINT, CLO_ULONG };
	/* large -> small -> large on one object per op, tie, form, count type and value type; the patterns, the num_in and
	 * row modes, the two forms of the call and val_out present or absent take turns */
	static const size_t sizes[] = { 2500, 7, 1, 4000 };
	unsigned turn = 0;
	for (int op = 0; op < 2; ++op) {
		for (int tie = 0; tie < 2; ++tie) {
			for (int form = 0; form < 2; ++form) {
				for (int c = 0; c < 2; ++c) {
					for (int v = 0; v < 6; ++v) {
						CloSegArg* sa = clo_segarg_new(op_names[op], tie_names[tie], form_names[form], NULL, ctx, value_types[v], count_types[c], &err);
						expect(&err, 0, "clo_segarg_new");
						if (!sa) continue;
						for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z) {
							for (int num_mode = 0; num_mode < NUM_MODES; ++num_mode, ++turn)
								run_segarg(ctx, cq, sa, op, tie, form, count_types[c], value_types[v], (int) (turn % PAT_COUNT), sizes[z], num_mode,
									(int) ((turn / PAT_COUNT) % ROWS_MODES), form ? 12345u * (turn % 3) : 0, (int) ((turn / 7) & 1), (turn % 5) != 0);
						}
						clo_segarg_destroy(sa);
					}
				}
			}
		}
	}
	/* every pattern x every row mode x both forms of the call, once per op and tie */
	for (int op = 0; op < 2; ++op) {
		for (int tie = 0; tie < 2; ++tie) {
			for (int form = 0; form < 2; ++form) {
				CloSegArg* sa = clo_segarg_new(op_names[op], tie_names[tie], form_names[form], NULL, ctx, CLO_FLOAT, CLO_UINT, &err);
				expect(&err, 0, "clo_segarg_new");
				for (int pattern = 0; sa && pattern < PAT_COUNT; ++pattern)
					for (int rows_mode = 0; rows_mode < ROWS_MODES; ++rows_mode)
						for (int host_form = 0; host_form < 2; ++host_form)
							run_segarg(ctx, cq, sa, op, tie, form, CLO_UINT, CLO_FLOAT, pattern, 333, (pattern + rows_mode) % NUM_MODES, rows_mode, form ? 777 : 0,
								host_form, 1);
				if (sa) clo_segarg_destroy(sa);
			}
		}
	}
	test_broken_preconditions(cq, ctx);
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("segarg host ok\n");
	return failures ? 1 : 0;
}
