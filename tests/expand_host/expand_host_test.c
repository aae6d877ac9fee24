/*
 * expand_host_test.c — CloExpand (include/clo_expand.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_expand_cpu.py). Both forms, both count types,
 * values of 1, 2, 4 and 8 bytes and every subset of the three outputs; num_in below, equal to and above numel_in and
 * absent; capacity 0, below, equal to and above total; all-zero counts and one count that covers everything; offsets
 * with offsets[0] != 0; descending offsets (the call returns, ASan stays silent); the host-data form; one object used
 * large -> small -> large (its workspace grows once and is reused); every refusal the driver makes (err == NULL
 * included), with the outputs left alone; a clean destroy. The expected rows come from a plain loop over the segments.
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
enum { CAP_ZERO, CAP_BELOW, CAP_EQUAL, CAP_ABOVE, CAP_MODES };
static const char* const form_names[2] = { "counts", "offsets" };
static const CloType value_types[4] = { CLO_UCHAR, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };   /* 1, 2, 4 and 8 bytes */

/* outs: bit 0 values, bit 1 seg, bit 2 rank. base: offsets[0] of the offsets form. */
static void run_expand(CCLContext* ctx, CCLQueue* cq, CloExpand* ex, int form, CloType ct, CloType vt, int outs, int pattern, size_t m_h,
	int num_mode, int cap_mode, uint64_t base, int host_form) {
	GError* err = NULL;
	const size_t cs = clo_type_sizeof(ct), vs = clo_type_sizeof(vt);
	uint64_t* counts = (uint64_t*) malloc((m_h + 1) * sizeof(uint64_t));
	for (size_t r = 0; r < m_h; ++r)
		counts[r] = pattern == PAT_ZEROS ? 0 : pattern == PAT_ONES ? 1 : pattern == PAT_ONE_BIG ? (r == m_h / 2 ? 5000 : 0) : (rnd() % 3 ? rnd() % 9 : 0);
	size_t num_in = num_mode == NUM_BELOW ? m_h - (m_h + 2) / 3 : num_mode == NUM_ABOVE ? m_h + 7 : m_h;
	const size_t m = num_in < m_h ? num_in : m_h;
	/* the expected rows: a plain loop */
	uint64_t total = 0;
	for (size_t r = 0; r < m; ++r) total += counts[r];
	uint32_t* want_seg = (uint32_t*) malloc((total + 1) * sizeof(uint32_t));
	uint32_t* want_rank = (uint32_t*) malloc((total + 1) * sizeof(uint32_t));
	size_t j = 0;
	for (size_t r = 0; r < m; ++r)
		for (uint64_t k = 0; k < counts[r]; ++k, ++j) { want_seg[j] = (uint32_t) r; want_rank[j] = (uint32_t) k; }
	const size_t capacity = cap_mode == CAP_ZERO ? 0 : cap_mode == CAP_BELOW ? (size_t) (total - (total + 3) / 4) : cap_mode == CAP_EQUAL ? (size_t) total : (size_t) total + 100;
	const size_t rows = total < capacity ? (size_t) total : capacity;
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
	unsigned char* hv = (unsigned char*) malloc(m_h * 8 + 8);
	for (size_t i = 0; i < m_h * 8 + 8; ++i) hv[i] = (unsigned char) rnd();
	const size_t held = capacity + 4;   /* rows of the output allocations: the rows past capacity are checked too */
	unsigned char* got_v = (unsigned char*) malloc(held * 8);
	uint32_t* got_s = (uint32_t*) malloc(held * 4);
	uint32_t* got_r = (uint32_t*) malloc(held * 4);
	memset(got_v, 0xEE, held * 8); memset(got_s, 0xEE, held * 4); memset(got_r, 0xEE, held * 4);
	const int wv = outs & 1, ws = (outs >> 1) & 1, wr = (outs >> 2) & 1;
	size_t got = 12345;
	if (host_form) {
		CHECK(clo_expand_with_host_data(ex, (m_h & 1) ? cq : NULL, NULL, src, num_mode == NUM_ABSENT ? NULL : &num_in, wv ? hv : NULL,
			wv ? got_v : NULL, ws ? got_s : NULL, wr ? got_r : NULL, &got, m_h, capacity, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[7];   /* counts or offsets, num_in, values, values out, seg out, rank out, num_out */
		const size_t bytes[7] = { src_n * cs, 8, m_h * vs, held * vs, held * 4, held * 4, 8 };
		cl_ulong count = 12345, dn = num_in;
		for (int i = 0; i < 7; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], src, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, 8, &dn, NULL, &err);
		ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3], got_v, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, bytes[4], got_s, NULL, &err);
		ccl_buffer_enqueue_write(b[5], cq, CL_TRUE, 0, bytes[5], got_r, NULL, &err);
		ccl_buffer_enqueue_write(b[6], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_expand_with_device_data(ex, cq, NULL, b[0], num_mode == NUM_ABSENT ? NULL : b[1], wv ? b[2] : NULL,
			wv ? b[3] : NULL, ws ? b[4] : NULL, wr ? b[5] : NULL, b[6], m_h, capacity, &err);
		expect(&err, 0, "expand");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[3], cq, CL_TRUE, 0, bytes[3], got_v, NULL, &err);
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, bytes[4], got_s, NULL, &err);
		ccl_buffer_enqueue_read(b[5], cq, CL_TRUE, 0, bytes[5], got_r, NULL, &err);
		ccl_buffer_enqueue_read(b[6], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "read");
		got = (size_t) count;
		for (int i = 0; i < 7; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "%s count size %zu value size %zu outs %d pattern %d m_h %zu num %d cap %d host %d"
#define WHERE_ARGS form_names[form], cs, vs, outs, pattern, m_h, num_mode, cap_mode, host_form
	CHECK(got == total, WHERE ": num_out = %zu, expected %llu", WHERE_ARGS, got, (unsigned long long) total);
	for (size_t i = 0; i < rows; ++i) {
		if (wv) CHECK(memcmp(got_v + i * vs, hv + (size_t) want_seg[i] * vs, vs) == 0, WHERE ": wrong value in row %zu", WHERE_ARGS, i);
		if (ws) CHECK(got_s[i] == want_seg[i], WHERE ": seg_out[%zu] = %u, expected %u", WHERE_ARGS, i, got_s[i], want_seg[i]);
		if (wr) CHECK(got_r[i] == want_rank[i], WHERE ": rank_out[%zu] = %u, expected %u", WHERE_ARGS, i, got_r[i], want_rank[i]);
	}
	for (size_t i = wv ? rows * vs : 0; i < held * 8; ++i) CHECK(got_v[i] == 0xEE, WHERE ": values_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = ws ? rows : 0; i < held; ++i) CHECK(got_s[i] == 0xEEEEEEEEu, WHERE ": seg_out written at row %zu", WHERE_ARGS, i);
	for (size_t i = wr ? rows : 0; i < held; ++i) CHECK(got_r[i] == 0xEEEEEEEEu, WHERE ": rank_out written at row %zu", WHERE_ARGS, i);
	free(counts); free(want_seg); free(want_rank); free(src); free(hv); free(got_v); free(got_s); free(got_r);
}

/* offsets that descend, counts whose sum wraps 2^64, a num_in far above numel_in: the call returns, every segment id
 * is below numel_in, and ASan sees every access */
static void test_broken_preconditions(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	enum { M = 300, CAP = 5000 };
	for (int which = 0; which < 3; ++which) {
		CloExpand* ex = clo_expand_new(which == 1 ? "counts" : "offsets", NULL, ctx, CLO_UINT, CLO_ULONG, &err);
		expect(&err, 0, "clo_expand_new");
		if (!ex) continue;
		uint64_t src[M + 1];
		uint32_t vals[M], vo[CAP], so[CAP], ro[CAP];
		for (int r = 0; r <= M; ++r)
			src[r] = which == 0 ? (uint64_t) (M - r) * 20 : which == 1 ? ~0ull / 3 + rnd() : (uint64_t) rnd() % 4000;   /* descending; wrapping; unordered */
		for (int r = 0; r < M; ++r) vals[r] = 0xC0DE0000u + (uint32_t) r;
		memset(so, 0, sizeof so);
		size_t num_in = (size_t) 1 << 40, total = 0;
		CHECK(clo_expand_with_host_data(ex, cq, NULL, src, &num_in, vals, vo, so, ro, &total, M, CAP, &err), "broken preconditions %d", which);
		expect(&err, 0, "broken preconditions");
		const size_t rows = total < CAP ? total : CAP;
		for (size_t i = 0; i < rows; ++i) CHECK(so[i] < M && vo[i] == 0xC0DE0000u + so[i], "broken preconditions %d: seg_out[%zu] = %u", which, i, so[i]);
		clo_expand_destroy(ex);
	}
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_expand_new("lengths", NULL, ctx, CLO_UINT, CLO_UINT, &err), "an unknown form");
	REFUSED_NEW(clo_expand_new(NULL, NULL, ctx, CLO_UINT, CLO_UINT, &err), "a NULL form");
	REFUSED_NEW(clo_expand_new("Counts", NULL, ctx, CLO_UINT, CLO_UINT, &err), "a form in another case");
	REFUSED_NEW(clo_expand_new("counts", "tile=1024", ctx, CLO_UINT, CLO_UINT, &err), "options");
	REFUSED_NEW(clo_expand_new("counts", NULL, ctx, CLO_UINT, CLO_INT, &err), "count_type int");
	REFUSED_NEW(clo_expand_new("offsets", NULL, ctx, CLO_UINT, CLO_LONG, &err), "count_type long");
	REFUSED_NEW(clo_expand_new("offsets", NULL, ctx, CLO_UINT, CLO_FLOAT, &err), "count_type float");
	REFUSED_NEW(clo_expand_new("counts", NULL, ctx, (CloType) 11, CLO_UINT, &err), "an unknown value type");
	REFUSED_NEW(clo_expand_new("counts", NULL, ctx, (CloType) -1, CLO_UINT, &err), "a negative value type");
	CHECK(clo_expand_new("count", NULL, ctx, CLO_UINT, CLO_UINT, NULL) == NULL, "an unknown form, err NULL");
	CHECK(clo_expand_new("counts", NULL, ctx, CLO_UINT, CLO_USHORT, NULL) == NULL, "count_type ushort, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	memset(base, 0, 4096);   /* (the stub's device memory is the host's) */
	/* 16 segments, capacity 16 */
	CCLBuffer* cn = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);               /* 16 counts */
	CCLBuffer* of = ccl_buffer_new_from_device_ptr(ctx, base, 68, &err);               /* 17 offsets */
	CCLBuffer* ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* vi = ccl_buffer_new_from_device_ptr(ctx, base + 80, 64, &err);          /* adjacent to ni */
	CCLBuffer* vo = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* so = ccl_buffer_new_from_device_ptr(ctx, base + 576, 64, &err);         /* adjacent to vo */
	CCLBuffer* ro = ccl_buffer_new_from_device_ptr(ctx, base + 640, 64, &err);         /* adjacent to so */
	CCLBuffer* no = ccl_buffer_new_from_device_ptr(ctx, base + 704, 8, &err);          /* adjacent to ro */
	CCLBuffer* so_on_cn = ccl_buffer_new_from_device_ptr(ctx, base + 60, 64, &err);    /* one shared element with the counts */
	CCLBuffer* so_on_of = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);    /* adjacent to the counts, on the 17th offset */
	CCLBuffer* so_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 76, 64, &err);    /* the second half of num_in */
	CCLBuffer* ro_on_vi = ccl_buffer_new_from_device_ptr(ctx, base + 140, 64, &err);   /* the last row of values_in */
	CCLBuffer* ro_in_so = ccl_buffer_new_from_device_ptr(ctx, base + 636, 64, &err);   /* starts on seg_out's row capacity - 1 */
	CCLBuffer* no_in_so = ccl_buffer_new_from_device_ptr(ctx, base + 632, 8, &err);    /* the last 8 bytes of seg_out */
	CCLBuffer* no_in_cn = ccl_buffer_new_from_device_ptr(ctx, base + 8, 8, &err);
	CCLBuffer* no_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* no_odd = ccl_buffer_new_from_device_ptr(ctx, base + 708, 8, &err);      /* not 8-byte aligned */
	CCLBuffer* no_small = ccl_buffer_new_from_device_ptr(ctx, base + 712, 4, &err);
	CCLBuffer* ni_odd = ccl_buffer_new_from_device_ptr(ctx, base + 1028, 8, &err);
	CCLBuffer* ni_small = ccl_buffer_new_from_device_ptr(ctx, base + 1032, 4, &err);
	CCLBuffer* cn_short = ccl_buffer_new_from_device_ptr(ctx, base, 60, &err);
	CCLBuffer* vi_short = ccl_buffer_new_from_device_ptr(ctx, base + 80, 60, &err);
	CCLBuffer* so_short = ccl_buffer_new_from_device_ptr(ctx, base + 2048, 60, &err);  /* 15 rows: below capacity even where total is small */
	CCLBuffer* vo_short = ccl_buffer_new_from_device_ptr(ctx, base + 2112, 60, &err);
	expect(&err, 0, "buffers");
	uint32_t hc[17] = { 0 }, hv[16] = { 0 }, hso[24], hvo[24];
	for (int i = 0; i < 24; ++i) { hso[i] = 0xABCD0000u + (uint32_t) i; hvo[i] = 0x12340000u + (uint32_t) i; }
	size_t hn = 777, hm = 16;
	CloExpand* c4 = clo_expand_new("counts", NULL, ctx, CLO_UINT, CLO_UINT, &err);
	CloExpand* o4 = clo_expand_new("offsets", "", ctx, CLO_FLOAT, CLO_UINT, &err);
	CloExpand* c8 = clo_expand_new("counts", NULL, ctx, CLO_DOUBLE, CLO_ULONG, &err);
	expect(&err, 0, "objects");
	if (!c4 || !o4 || !c8) return;
	CHECK(clo_expand_get_context(o4) == ctx && clo_expand_get_value_type(o4) == CLO_FLOAT && clo_expand_get_value_size(o4) == 4
		&& clo_expand_get_value_size(c8) == 8 && clo_expand_get_count_type(c8) == CLO_ULONG && clo_expand_get_count_size(c8) == 8
		&& clo_expand_get_count_size(c4) == 4 && !strcmp(clo_expand_get_form(c4), "counts") && !strcmp(clo_expand_get_form(o4), "offsets"), "getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, no, (size_t) 1 << 32, 16, &err), "numel_in 2^32");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, no, 16, (size_t) 1 << 32, &err), "capacity 2^32");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, NULL, NULL, NULL, hso, NULL, &hn, (size_t) 1 << 32, 16, &err), "numel_in 2^32, host");
	REFUSED_HOST(clo_expand_with_host_data(o4, cq, NULL, hc, NULL, NULL, NULL, hso, NULL, &hn, 16, (size_t) 1 << 33, &err), "capacity 2^33, host");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, NULL, NULL, NULL, NULL, so, NULL, no, 16, 16, &err), "counts NULL");
	REFUSED_HOST(clo_expand_with_host_data(o4, cq, NULL, NULL, NULL, NULL, NULL, hso, NULL, &hn, 16, 16, &err), "offsets NULL, host");
	REFUSED_DEV(clo_expand_with_device_data(o4, cq, NULL, NULL, NULL, NULL, NULL, so, NULL, no, 0, 16, &err), "offsets NULL with numel_in 0 and a capacity");
	REFUSED_HOST(clo_expand_with_host_data(o4, cq, NULL, NULL, NULL, NULL, NULL, hso, NULL, &hn, 0, 1, &err), "offsets NULL with numel_in 0 and a capacity, host");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, NULL, NULL, no, 16, 16, &err), "all outputs NULL");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, NULL, NULL, NULL, NULL, NULL, &hn, 16, 16, &err), "all outputs NULL, host");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, vi, NULL, so, NULL, no, 16, 16, &err), "values_in without values_out");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, vo, so, NULL, no, 16, 16, &err), "values_out without values_in");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, NULL, hv, NULL, hso, NULL, &hn, 16, 16, &err), "values_in without values_out, host");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, NULL, NULL, hvo, NULL, NULL, &hn, 16, 16, &err), "values_out without values_in, host");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, NULL, 16, 16, &err), "num_out NULL");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, NULL, NULL, NULL, hso, NULL, NULL, 16, 16, &err), "num_out NULL, host");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, no_odd, 16, 16, &err), "num_out misaligned");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, no_small, 16, 16, &err), "num_out of 4 bytes");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, ni_odd, NULL, NULL, so, NULL, no, 16, 16, &err), "num_in misaligned");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, ni_small, NULL, NULL, so, NULL, no, 16, 16, &err), "num_in of 4 bytes");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, no, 17, 16, &err), "numel_in beyond the counts");
	REFUSED_DEV(clo_expand_with_device_data(o4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, no, 16, 16, &err), "16 offsets for 16 segments");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn_short, NULL, NULL, NULL, so, NULL, no, 16, 16, &err), "counts below numel_in");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, vi_short, vo, so, NULL, no, 16, 16, &err), "values_in below numel_in rows");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so_short, NULL, no, 16, 16, &err), "seg_out below capacity rows");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, NULL, so_short, no, 16, 16, &err), "rank_out below capacity rows");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, vi, vo_short, NULL, NULL, no, 16, 16, &err), "values_out below capacity rows");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, cn, NULL, no, 16, 16, &err), "seg_out on the counts");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so_on_cn, NULL, no, 16, 16, &err), "seg_out sharing the counts' last element");
	REFUSED_DEV(clo_expand_with_device_data(o4, cq, NULL, of, NULL, NULL, NULL, so_on_of, NULL, no, 16, 16, &err), "seg_out on the last offset");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, ni, NULL, NULL, so_on_ni, NULL, no, 16, 16, &err), "seg_out on num_in");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, vi, vo, NULL, ro_on_vi, no, 16, 16, &err), "rank_out on values_in's last row");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, vi, vi, so, NULL, no, 16, 16, &err), "values_out on values_in");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, ro_in_so, no, 16, 16, &err), "rank_out on seg_out's row capacity - 1");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, so, no, 16, 16, &err), "rank_out on seg_out");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, no_in_so, 16, 16, &err), "num_out inside seg_out");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, no_in_cn, 16, 16, &err), "num_out inside the counts");
	REFUSED_DEV(clo_expand_with_device_data(c4, cq, NULL, cn, ni, NULL, NULL, so, NULL, no_on_ni, 16, 16, &err), "num_out on num_in");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, NULL, NULL, NULL, hso, hso + 15, &hn, 16, 16, &err), "rank_out on seg_out's last row, host");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hso + 8, NULL, NULL, NULL, hso, NULL, &hn, 16, 24, &err), "the counts inside seg_out, host");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, (size_t*) (hso + 2), NULL, NULL, hso, NULL, &hn, 16, 16, &err), "num_in inside seg_out, host");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, NULL, NULL, NULL, hso, NULL, (size_t*) (hso + 14), 16, 16, &err), "num_out inside seg_out, host");
	REFUSED_HOST(clo_expand_with_host_data(c4, cq, NULL, hc, &hn, NULL, NULL, hso, NULL, &hn, 16, 16, &err), "num_out on num_in, host");
	/* err == NULL */
	CHECK(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, cn, NULL, no, 16, 16, NULL) == NULL, "seg_out on the counts, err NULL");
	CHECK(clo_expand_with_device_data(c4, cq, NULL, cn, NULL, NULL, NULL, so, NULL, NULL, 16, 16, NULL) == NULL, "num_out NULL, err NULL");
	CHECK(!clo_expand_with_host_data(c4, NULL, NULL, hc, NULL, NULL, NULL, hso, NULL, &hn, (size_t) 1 << 32, 16, NULL), "numel_in 2^32, host, err NULL");
	CHECK(!clo_expand_with_host_data(c4, NULL, NULL, hc, NULL, NULL, NULL, NULL, NULL, &hn, 16, 16, NULL), "all outputs NULL, host, err NULL");
	for (int i = 0; i < 24; ++i) CHECK(hso[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	CHECK(hn == 777 && hm == 16, "a refused call wrote num_out or num_in");
	for (int i = 0; i < 4096; ++i) CHECK(base[i] == 0, "a refused call wrote device memory at %d", i);
	/* adjacent, disjoint views of one allocation are accepted */
	CHECK(clo_expand_with_device_data(c4, cq, NULL, cn, ni, vi, vo, so, ro, no, 16, 16, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_expand_with_device_data(o4, cq, NULL, of, ni, vi, vo, so, ro, no, 16, 16, &err) != NULL, "disjoint views of one allocation, offsets");
	expect(&err, 0, "disjoint views of one allocation, offsets");
	/* m == 0: success, num_out 0, nothing else written, no queue needed in the host form, inputs may be NULL */
	CHECK(clo_expand_with_host_data(c4, NULL, NULL, NULL, NULL, NULL, NULL, hso, NULL, &hn, 0, 16, &err), "empty, host");
	expect(&err, 0, "empty, host");
	CHECK(hn == 0, "empty, host: num_out %zu", hn);
	hn = 777; hm = 0;
	CHECK(clo_expand_with_host_data(o4, NULL, NULL, hc, &hm, hv, hvo, hso, NULL, &hn, 16, 16, &err), "num_in 0, host");
	expect(&err, 0, "num_in 0, host");
	CHECK(hn == 0, "num_in 0, host: num_out %zu", hn);
	cl_ulong dn = 777;
	ccl_buffer_enqueue_write(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	CHECK(clo_expand_with_device_data(c4, cq, NULL, NULL, NULL, NULL, NULL, so, NULL, no, 0, 16, &err) != NULL, "empty, device");
	expect(&err, 0, "empty, device");
	ccl_buffer_enqueue_read(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	expect(&err, 0, "read");
	CHECK(dn == 0, "empty, device: num_out %llu", (unsigned long long) dn);
	for (int i = 0; i < 24; ++i) CHECK(hso[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "an empty call wrote an output at %d", i);

	clo_expand_destroy(c4); clo_expand_destroy(o4); clo_expand_destroy(c8);
	CCLBuffer* all[] = { cn, of, ni, vi, vo, so, ro, no, so_on_cn, so_on_of, so_on_ni, ro_on_vi, ro_in_so, no_in_so, no_in_cn, no_on_ni, no_odd, no_small,
		ni_odd, ni_small, cn_short, vi_short, so_short, vo_short, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType count_types[2] = { CLO_UINT, CLO_ULONG };
	/* large -> small -> large on one object per form, count type and value size; the patterns, the num_in and capacity
	 * modes and the two forms of the call take turns so that every one of them meets every subset of the outputs */
	static const size_t sizes[] = { 2500, 7, 1, 4000 };
	unsigned turn = 0;
	for (int form = 0; form < 2; ++form) {
		for (int c = 0; c < 2; ++c) {
			for (int v = 0; v < 4; ++v) {
				CloExpand* ex = clo_expand_new(form_names[form], NULL, ctx, value_types[v], count_types[c], &err);
				expect(&err, 0, "clo_expand_new");
				if (!ex) continue;
				for (int outs = 1; outs < 8; ++outs) {
					for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z) {
						for (int num_mode = 0; num_mode < NUM_MODES; ++num_mode, ++turn)
							run_expand(ctx, cq, ex, form, count_types[c], value_types[v], outs, (int) (turn % PAT_COUNT), sizes[z], num_mode,
								(int) ((turn / PAT_COUNT) % CAP_MODES), form ? 12345u * (turn % 3) : 0, (int) ((turn / 7) & 1));
					}
				}
				clo_expand_destroy(ex);
			}
		}
	}
	/* every pattern x every capacity mode x both forms of the call, once */
	for (int form = 0; form < 2; ++form) {
		CloExpand* ex = clo_expand_new(form_names[form], NULL, ctx, CLO_UINT, CLO_UINT, &err);
		expect(&err, 0, "clo_expand_new");
		for (int pattern = 0; ex && pattern < PAT_COUNT; ++pattern)
			for (int cap_mode = 0; cap_mode < CAP_MODES; ++cap_mode)
				for (int host_form = 0; host_form < 2; ++host_form)
					run_expand(ctx, cq, ex, form, CLO_UINT, CLO_UINT, 7, pattern, 333, (pattern + cap_mode) % NUM_MODES, cap_mode, form ? 777 : 0, host_form);
		if (ex) clo_expand_destroy(ex);
	}
	test_broken_preconditions(ctx, cq);
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("expand host ok\n");
	return failures ? 1 : 0;
}
