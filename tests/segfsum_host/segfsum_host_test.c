/*
 * segfsum_host_test.c — CloSegFSum (include/clo_segfsum.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_segfsum_cpu.py). Both forms, both count types and
 * the four pairs of types; num_in below, equal to and above numel_seg and absent; numel below, equal to and above total
 * (segments clipped in the middle and clipped away); all-zero counts and one count that covers everything; offsets with
 * offsets[0] != 0; descending offsets (the call returns, ASan stays silent); the host-data form; one object used large ->
 * small -> large (its workspace grows once and is reused); every refusal the driver makes (err == NULL included), with
 * the outputs left alone; a clean destroy. The values are small integers, which every type holds and every partial sum
 * keeps exactly, so the stub's serial order and any other order agree and the expected sums come from integer
 * arithmetic.
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
static const char* const form_names[2] = { "counts", "offsets" };
static const CloType pair_types[4][2] = { { CLO_HALF, CLO_FLOAT }, { CLO_FLOAT, CLO_FLOAT }, { CLO_FLOAT, CLO_DOUBLE }, { CLO_DOUBLE, CLO_DOUBLE } };

/* the half with the value of the integer v, |v| <= 2048 */
static uint16_t half_of(int v) {
	const uint16_t sign = v < 0 ? 0x8000u : 0u;
	unsigned a = (unsigned) (v < 0 ? -v : v);
	if (a == 0) return sign;
	int e = 0;
	while ((a >> (e + 1)) != 0) ++e;   /* a in [2^e, 2^(e+1)) */
	return (uint16_t) (sign | ((unsigned) (e + 15) << 10) | ((a << (10 - e)) & 0x3ffu));
}

static void put_value(unsigned char* values, size_t i, CloType vt, int v) {
	if (vt == CLO_HALF) { const uint16_t h = half_of(v); memcpy(values + i * 2, &h, 2); }
	else if (vt == CLO_FLOAT) { const float f = (float) v; memcpy(values + i * 4, &f, 4); }
	else { const double d = (double) v; memcpy(values + i * 8, &d, 8); }
}

static void run_segfsum(CCLContext* ctx, CCLQueue* cq, CloSegFSum* sf, int form, CloType ct, int pair, int pattern, size_t m_h,
	int num_mode, int rows_mode, uint64_t base, int host_form) {
	GError* err = NULL;
	const CloType vt = pair_types[pair][0], st = pair_types[pair][1];
	const size_t cs = clo_type_sizeof(ct), vs = clo_type_sizeof(vt), ss = clo_type_sizeof(st);
	uint64_t* counts = (uint64_t*) malloc((m_h + 1) * sizeof(uint64_t));
	for (size_t r = 0; r < m_h; ++r)
		counts[r] = pattern == PAT_ZEROS ? 0 : pattern == PAT_ONES ? 1 : pattern == PAT_ONE_BIG ? (r == m_h / 2 ? 5000 : 0) : (rnd() % 3 ? rnd() % 9 : 0);
	size_t num_in = num_mode == NUM_BELOW ? m_h - (m_h + 2) / 3 : num_mode == NUM_ABOVE ? m_h + 7 : m_h;
	const size_t m = num_in < m_h ? num_in : m_h;
	uint64_t total = 0;
	for (size_t r = 0; r < m; ++r) total += counts[r];
	const size_t n = rows_mode == ROWS_ZERO ? 0 : rows_mode == ROWS_BELOW ? (size_t) (total - (total + 3) / 4) : rows_mode == ROWS_EQUAL ? (size_t) total : (size_t) total + 100;
	/* the values: integers in [-1000, 1000]; a segment of 5000 rows stays below 2^23 */
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	int* iv = (int*) malloc((n + 1) * sizeof(int));
	for (size_t i = 0; i < n; ++i) { iv[i] = (int) (rnd() % 2001u) - 1000; put_value(hv, i, vt, iv[i]); }
	/* the expected sums: a plain loop over integers */
	int64_t* want = (int64_t*) malloc((m + 1) * sizeof(int64_t));
	uint64_t at = 0;
	for (size_t r = 0; r < m; ++r) {
		int64_t acc = 0;
		for (uint64_t k = 0; k < counts[r]; ++k, ++at) if (at < n) acc += iv[at];
		want[r] = acc;
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
	const size_t held = m_h + 4;   /* rows of the output allocation: the rows past m are checked too */
	unsigned char* got_s = (unsigned char*) malloc(held * 8);
	memset(got_s, 0xEE, held * 8);
	size_t got = 12345;
	if (host_form) {
		CHECK(clo_segfsum_with_host_data(sf, (m_h & 1) ? cq : NULL, NULL, src, num_mode == NUM_ABSENT ? NULL : &num_in, n ? hv : NULL,
			got_s, &got, m_h, n, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[5];   /* counts or offsets, num_in, values, sums out, num_out */
		const size_t bytes[5] = { src_n * cs, 8, n * vs, held * ss, 8 };
		cl_ulong count = 12345, dn = num_in;
		for (int i = 0; i < 5; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], src, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, 8, &dn, NULL, &err);
		if (n) ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3], got_s, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_segfsum_with_device_data(sf, cq, NULL, b[0], num_mode == NUM_ABSENT ? NULL : b[1], n ? b[2] : NULL, b[3], b[4], m_h, n, &err);
		expect(&err, 0, "segfsum");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[3], cq, CL_TRUE, 0, bytes[3], got_s, NULL, &err);
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "read");
		got = (size_t) count;
		for (int i = 0; i < 5; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "%s count size %zu pair %d pattern %d m_h %zu num %d rows %d host %d"
#define WHERE_ARGS form_names[form], cs, pair, pattern, m_h, num_mode, rows_mode, host_form
	CHECK(got == total, WHERE ": num_out = %zu, expected %llu", WHERE_ARGS, got, (unsigned long long) total);
	for (size_t r = 0; r < m; ++r) {
		double v;
		if (ss == 4) { float f; memcpy(&f, got_s + r * 4, 4); v = (double) f; }
		else memcpy(&v, got_s + r * 8, 8);
		CHECK(v == (double) want[r], WHERE ": sums_out[%zu] = %g, expected %lld", WHERE_ARGS, r, v, (long long) want[r]);
		if (want[r] == 0) CHECK(got_s[r * ss + ss - 1] == 0, WHERE ": sums_out[%zu] is -0", WHERE_ARGS, r);   /* (little endian) */
	}
	for (size_t i = m * ss; i < held * 8; ++i) CHECK(got_s[i] == 0xEE, WHERE ": sums_out written at byte %zu", WHERE_ARGS, i);
	free(counts); free(want); free(src); free(hv); free(iv); free(got_s);
}

/* offsets that descend, counts whose sum wraps 2^64, a num_in far above numel_seg: the call returns and ASan sees every
 * access */
static void test_broken_preconditions(CCLQueue* cq, CCLContext* ctx) {
	GError* err = NULL;
	enum { M = 300, N = 5000 };
	for (int which = 0; which < 3; ++which) {
		CloSegFSum* sf = clo_segfsum_new(which == 1 ? "counts" : "offsets", NULL, ctx, CLO_DOUBLE, CLO_DOUBLE, CLO_ULONG, &err);
		expect(&err, 0, "clo_segfsum_new");
		if (!sf) continue;
		uint64_t src[M + 1];
		double vals[N];
		double out[M];
		for (int r = 0; r <= M; ++r)
			src[r] = which == 0 ? (uint64_t) (M - r) * 20 : which == 1 ? ~0ull / 3 + rnd() : (uint64_t) rnd() % 8000;   /* descending; wrapping; unordered */
		for (int i = 0; i < N; ++i) vals[i] = (double) (rnd() % 100u);
		size_t num_in = (size_t) 1 << 40, total = 0;
		CHECK(clo_segfsum_with_host_data(sf, cq, NULL, src, &num_in, vals, out, &total, M, N, &err), "broken preconditions %d", which);
		expect(&err, 0, "broken preconditions");
		clo_segfsum_destroy(sf);
	}
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_segfsum_new("lengths", NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_UINT, &err), "an unknown form");
	REFUSED_NEW(clo_segfsum_new(NULL, NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_UINT, &err), "a NULL form");
	REFUSED_NEW(clo_segfsum_new("Counts", NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_UINT, &err), "a form in another case");
	REFUSED_NEW(clo_segfsum_new("counts", "tile=1024", ctx, CLO_FLOAT, CLO_FLOAT, CLO_UINT, &err), "options");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_INT, &err), "count_type int");
	REFUSED_NEW(clo_segfsum_new("offsets", NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_LONG, &err), "count_type long");
	REFUSED_NEW(clo_segfsum_new("offsets", NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_FLOAT, &err), "count_type float");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err), "uint into uint");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_INT, CLO_FLOAT, CLO_UINT, &err), "int values");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_FLOAT, CLO_ULONG, CLO_UINT, &err), "ulong sums");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_USHORT, CLO_FLOAT, CLO_UINT, &err), "ushort values");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_HALF, CLO_HALF, CLO_UINT, &err), "half sums");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_FLOAT, CLO_HALF, CLO_UINT, &err), "float into half");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_DOUBLE, CLO_FLOAT, CLO_UINT, &err), "double into float");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, CLO_HALF, CLO_DOUBLE, CLO_UINT, &err), "half into double");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, ctx, (CloType) 11, CLO_FLOAT, CLO_UINT, &err), "an unknown value type");
	REFUSED_NEW(clo_segfsum_new("counts", NULL, NULL, CLO_FLOAT, CLO_FLOAT, CLO_UINT, &err), "no context");
	CHECK(clo_segfsum_new("count", NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_UINT, NULL) == NULL, "an unknown form, err NULL");
	CHECK(clo_segfsum_new("counts", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, NULL) == NULL, "uint into uint, err NULL");
	CHECK(clo_segfsum_new("counts", NULL, ctx, CLO_HALF, CLO_DOUBLE, CLO_UINT, NULL) == NULL, "half into double, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	memset(base, 0, 4096);   /* (the stub's device memory is the host's) */
	/* 16 segments, 16 rows */
	CCLBuffer* cn = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);               /* 16 counts */
	CCLBuffer* of = ccl_buffer_new_from_device_ptr(ctx, base, 68, &err);               /* 17 offsets */
	CCLBuffer* ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* vi = ccl_buffer_new_from_device_ptr(ctx, base + 80, 64, &err);          /* adjacent to ni */
	CCLBuffer* so = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* no = ccl_buffer_new_from_device_ptr(ctx, base + 576, 8, &err);          /* adjacent to so */
	CCLBuffer* so8 = ccl_buffer_new_from_device_ptr(ctx, base + 1536, 64, &err);       /* 8 rows of 8 bytes */
	CCLBuffer* so_on_cn = ccl_buffer_new_from_device_ptr(ctx, base + 60, 64, &err);    /* one shared element with the counts */
	CCLBuffer* so_on_of = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);    /* adjacent to the counts, on the 17th offset */
	CCLBuffer* so_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 76, 64, &err);    /* the second half of num_in */
	CCLBuffer* so_on_vi = ccl_buffer_new_from_device_ptr(ctx, base + 140, 64, &err);   /* the last row of values_in */
	CCLBuffer* no_in_so = ccl_buffer_new_from_device_ptr(ctx, base + 568, 8, &err);    /* the last 8 bytes of sums_out */
	CCLBuffer* no_in_cn = ccl_buffer_new_from_device_ptr(ctx, base + 8, 8, &err);
	CCLBuffer* no_in_vi = ccl_buffer_new_from_device_ptr(ctx, base + 88, 8, &err);
	CCLBuffer* no_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* no_odd = ccl_buffer_new_from_device_ptr(ctx, base + 708, 8, &err);      /* not 8-byte aligned */
	CCLBuffer* no_small = ccl_buffer_new_from_device_ptr(ctx, base + 712, 4, &err);
	CCLBuffer* ni_odd = ccl_buffer_new_from_device_ptr(ctx, base + 1028, 8, &err);
	CCLBuffer* ni_small = ccl_buffer_new_from_device_ptr(ctx, base + 1032, 4, &err);
	CCLBuffer* cn_short = ccl_buffer_new_from_device_ptr(ctx, base, 60, &err);
	CCLBuffer* vi_short = ccl_buffer_new_from_device_ptr(ctx, base + 80, 60, &err);
	CCLBuffer* so_short = ccl_buffer_new_from_device_ptr(ctx, base + 2048, 60, &err);  /* 15 rows: below numel_seg even where num_in is small */
	expect(&err, 0, "buffers");
	uint32_t hc[17] = { 0 }, hso[24];
	float hv[16] = { 0 };
	for (int i = 0; i < 24; ++i) hso[i] = 0xABCD0000u + (uint32_t) i;
	size_t hn = 777, hm = 16;
	CloSegFSum* c4 = clo_segfsum_new("counts", NULL, ctx, CLO_FLOAT, CLO_FLOAT, CLO_UINT, &err);
	CloSegFSum* o4 = clo_segfsum_new("offsets", "", ctx, CLO_HALF, CLO_FLOAT, CLO_UINT, &err);
	CloSegFSum* c8 = clo_segfsum_new("counts", NULL, ctx, CLO_FLOAT, CLO_DOUBLE, CLO_ULONG, &err);
	expect(&err, 0, "objects");
	if (!c4 || !o4 || !c8) return;
	CHECK(clo_segfsum_get_context(o4) == ctx && clo_segfsum_get_value_type(o4) == CLO_HALF && clo_segfsum_get_value_size(o4) == 2
		&& clo_segfsum_get_sum_type(o4) == CLO_FLOAT && clo_segfsum_get_sum_size(o4) == 4 && clo_segfsum_get_value_type(c8) == CLO_FLOAT
		&& clo_segfsum_get_sum_type(c8) == CLO_DOUBLE && clo_segfsum_get_sum_size(c8) == 8 && clo_segfsum_get_count_type(c8) == CLO_ULONG
		&& clo_segfsum_get_count_size(c8) == 8 && clo_segfsum_get_count_size(c4) == 4 && !strcmp(clo_segfsum_get_form(c4), "counts")
		&& !strcmp(clo_segfsum_get_form(o4), "offsets"), "getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no, (size_t) 1 << 32, 16, &err), "numel_seg 2^32");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no, 16, (size_t) 1 << 32, &err), "numel 2^32");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hc, NULL, hv, hso, &hn, (size_t) 1 << 32, 16, &err), "numel_seg 2^32, host");
	REFUSED_HOST(clo_segfsum_with_host_data(o4, cq, NULL, hc, NULL, hv, hso, &hn, 16, (size_t) 1 << 33, &err), "numel 2^33, host");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, NULL, NULL, vi, so, no, 16, 16, &err), "counts NULL");
	REFUSED_HOST(clo_segfsum_with_host_data(o4, cq, NULL, NULL, NULL, hv, hso, &hn, 16, 16, &err), "offsets NULL, host");
	REFUSED_DEV(clo_segfsum_with_device_data(o4, cq, NULL, NULL, NULL, NULL, NULL, no, 0, 0, &err), "offsets NULL with numel_seg 0");
	REFUSED_HOST(clo_segfsum_with_host_data(o4, cq, NULL, NULL, NULL, NULL, NULL, &hn, 0, 0, &err), "offsets NULL with numel_seg 0, host");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, NULL, so, no, 16, 16, &err), "values_in NULL");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hc, NULL, NULL, hso, &hn, 16, 16, &err), "values_in NULL, host");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, NULL, no, 16, 16, &err), "sums_out NULL");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hc, NULL, hv, NULL, &hn, 16, 16, &err), "sums_out NULL, host");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, NULL, 16, 16, &err), "num_out NULL");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hc, NULL, hv, hso, NULL, 16, 16, &err), "num_out NULL, host");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no_odd, 16, 16, &err), "num_out misaligned");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no_small, 16, 16, &err), "num_out of 4 bytes");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, ni_odd, vi, so, no, 16, 16, &err), "num_in misaligned");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, ni_small, vi, so, no, 16, 16, &err), "num_in of 4 bytes");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no, 17, 16, &err), "numel_seg beyond the counts");
	REFUSED_DEV(clo_segfsum_with_device_data(o4, cq, NULL, cn, NULL, vi, so, no, 16, 16, &err), "16 offsets for 16 segments");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn_short, NULL, vi, so, no, 16, 16, &err), "counts below numel_seg");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi_short, so, no, 16, 16, &err), "values_in below numel rows");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no, 16, 17, &err), "numel beyond values_in");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so_short, no, 16, 16, &err), "sums_out below numel_seg rows");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, ni, vi, so_short, no, 16, 16, &err), "sums_out below numel_seg rows, with num_in");
	REFUSED_DEV(clo_segfsum_with_device_data(c8, cq, NULL, so8, NULL, vi, so_short, no, 8, 8, &err), "sums_out below numel_seg rows of 8 bytes");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, cn, no, 16, 16, &err), "sums_out on the counts");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so_on_cn, no, 16, 16, &err), "sums_out sharing the counts' last element");
	REFUSED_DEV(clo_segfsum_with_device_data(o4, cq, NULL, of, NULL, vi, so_on_of, no, 16, 16, &err), "sums_out on the last offset");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, ni, vi, so_on_ni, no, 16, 16, &err), "sums_out on num_in");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so_on_vi, no, 16, 16, &err), "sums_out on values_in's last row");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, vi, no, 16, 16, &err), "sums_out on values_in");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no_in_so, 16, 16, &err), "num_out inside sums_out");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no_in_cn, 16, 16, &err), "num_out inside the counts");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, no_in_vi, 16, 16, &err), "num_out inside values_in");
	REFUSED_DEV(clo_segfsum_with_device_data(c4, cq, NULL, cn, ni, vi, so, no_on_ni, 16, 16, &err), "num_out on num_in");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hso + 8, NULL, hv, hso, &hn, 16, 16, &err), "the counts inside sums_out, host");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hc, NULL, hso + 15, hso, &hn, 16, 8, &err), "values_in on sums_out's last row, host");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hc, (size_t*) (hso + 2), hv, hso, &hn, 16, 16, &err), "num_in inside sums_out, host");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hc, NULL, hv, hso, (size_t*) (hso + 14), 16, 16, &err), "num_out inside sums_out, host");
	REFUSED_HOST(clo_segfsum_with_host_data(c4, cq, NULL, hc, &hn, hv, hso, &hn, 16, 16, &err), "num_out on num_in, host");
	/* err == NULL */
	CHECK(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, cn, no, 16, 16, NULL) == NULL, "sums_out on the counts, err NULL");
	CHECK(clo_segfsum_with_device_data(c4, cq, NULL, cn, NULL, vi, so, NULL, 16, 16, NULL) == NULL, "num_out NULL, err NULL");
	CHECK(!clo_segfsum_with_host_data(c4, NULL, NULL, hc, NULL, hv, hso, &hn, (size_t) 1 << 32, 16, NULL), "numel_seg 2^32, host, err NULL");
	CHECK(!clo_segfsum_with_host_data(c4, NULL, NULL, hc, NULL, hv, NULL, &hn, 16, 16, NULL), "sums_out NULL, host, err NULL");
	for (int i = 0; i < 24; ++i) CHECK(hso[i] == 0xABCD0000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	CHECK(hn == 777 && hm == 16, "a refused call wrote num_out or num_in");
	for (int i = 0; i < 4096; ++i) CHECK(base[i] == 0, "a refused call wrote device memory at %d", i);
	/* adjacent, disjoint views of one allocation are accepted */
	CHECK(clo_segfsum_with_device_data(c4, cq, NULL, cn, ni, vi, so, no, 16, 16, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_segfsum_with_device_data(o4, cq, NULL, of, ni, vi, so, no, 16, 16, &err) != NULL, "disjoint views of one allocation, offsets");
	expect(&err, 0, "disjoint views of one allocation, offsets");
	/* m == 0: success, num_out 0, nothing else written, no queue needed in the host form, inputs may be NULL */
	CHECK(clo_segfsum_with_host_data(c4, NULL, NULL, NULL, NULL, hv, NULL, &hn, 0, 16, &err), "empty, host");
	expect(&err, 0, "empty, host");
	CHECK(hn == 0, "empty, host: num_out %zu", hn);
	hn = 777; hm = 0;
	CHECK(clo_segfsum_with_host_data(o4, NULL, NULL, hc, &hm, hv, hso, &hn, 16, 16, &err), "num_in 0, host");
	expect(&err, 0, "num_in 0, host");
	CHECK(hn == 0, "num_in 0, host: num_out %zu", hn);
	cl_ulong dn = 777;
	ccl_buffer_enqueue_write(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	CHECK(clo_segfsum_with_device_data(c4, cq, NULL, NULL, NULL, vi, NULL, no, 0, 16, &err) != NULL, "empty, device");
	expect(&err, 0, "empty, device");
	ccl_buffer_enqueue_read(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	expect(&err, 0, "read");
	CHECK(dn == 0, "empty, device: num_out %llu", (unsigned long long) dn);
	for (int i = 0; i < 24; ++i) CHECK(hso[i] == 0xABCD0000u + (uint32_t) i, "an empty call wrote an output at %d", i);

	clo_segfsum_destroy(c4); clo_segfsum_destroy(o4); clo_segfsum_destroy(c8);
	CCLBuffer* all[] = { cn, of, ni, vi, so, no, so8, so_on_cn, so_on_of, so_on_ni, so_on_vi, no_in_so, no_in_cn, no_in_vi, no_on_ni,
		no_odd, no_small, ni_odd, ni_small, cn_short, vi_short, so_short, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType count_types[2] = { CLO_UINT, CLO_ULONG };
	/* large -> small -> large on one object per form, count type and pair; the patterns, the num_in and row modes and the
	 * two forms of the call take turns */
	static const size_t sizes[] = { 2500, 7, 1, 4000 };
	unsigned turn = 0;
	for (int form = 0; form < 2; ++form) {
		for (int c = 0; c < 2; ++c) {
			for (int pair = 0; pair < 4; ++pair) {
				CloSegFSum* sf = clo_segfsum_new(form_names[form], NULL, ctx, pair_types[pair][0], pair_types[pair][1], count_types[c], &err);
				expect(&err, 0, "clo_segfsum_new");
				if (!sf) continue;
				for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z) {
					for (int num_mode = 0; num_mode < NUM_MODES; ++num_mode, ++turn)
						run_segfsum(ctx, cq, sf, form, count_types[c], pair, (int) (turn % PAT_COUNT), sizes[z], num_mode,
							(int) ((turn / PAT_COUNT) % ROWS_MODES), form ? 12345u * (turn % 3) : 0, (int) ((turn / 7) & 1));
				}
				clo_segfsum_destroy(sf);
			}
		}
	}
	/* every pattern x every row mode x both forms of the call, once per form and pair */
	for (int form = 0; form < 2; ++form) {
		for (int pair = 0; pair < 4; ++pair) {
			CloSegFSum* sf = clo_segfsum_new(form_names[form], NULL, ctx, pair_types[pair][0], pair_types[pair][1], CLO_UINT, &err);
			expect(&err, 0, "clo_segfsum_new");
			for (int pattern = 0; sf && pattern < PAT_COUNT; ++pattern)
				for (int rows_mode = 0; rows_mode < ROWS_MODES; ++rows_mode)
					for (int host_form = 0; host_form < 2; ++host_form)
						run_segfsum(ctx, cq, sf, form, CLO_UINT, pair, pattern, 333, (pattern + rows_mode) % NUM_MODES, rows_mode, form ? 777 : 0, host_form);
			if (sf) clo_segfsum_destroy(sf);
		}
	}
	test_broken_preconditions(cq, ctx);
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("segfsum host ok\n");
	return failures ? 1 : 0;
}
