/*
 * segtopk_host_test.c — CloSegTopK (include/clo_segtopk.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_segtopk_cpu.py). Both which, both forms, both
 * count types, key types of every size and kind, keys only, 4- and 8-byte values, the arg form with and without
 * keys_out; k from 1 to the cap and 0; num_in below, equal to and above numel_seg and absent; numel below, equal to and
 * above total; all-zero counts and one count that covers everything; offsets with offsets[0] != 0; descending offsets
 * (the call returns, ASan stays silent); the host-data form, which leaves the slots that are not written as the caller
 * filled them; one object used large -> small -> large (its workspace grows once and is reused); every refusal the
 * driver makes (err == NULL included), with the outputs left alone; a clean destroy. The expected rows come from a plain
 * selection: the j-th row of a segment is the one with the j-th smallest (order key, row).
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
enum { MODE_KEYS, MODE_V4, MODE_V8, MODE_ARG, MODE_ARG_NO_KEYS, MODE_COUNT };
static const size_t mode_value_size[MODE_COUNT] = { 0, 4, 8, 4, 4 };
static const char* const form_names[2] = { "counts", "offsets" };
static const char* const which_names[2] = { "smallest", "largest" };

static uint64_t word(const unsigned char* p, size_t i, size_t size) {
	uint64_t v = 0;
	memcpy(&v, p + i * size, size);   /* (little endian) */
	return v;
}

/* the key as an unsigned number whose order is the sort's: unsigned by bits, signed numerically, floating point in
 * IEEE total order; complemented for "largest" */
static uint64_t order_of(uint64_t x, CloType kt, int largest) {
	const size_t ks = clo_type_sizeof(kt);
	const uint64_t sign = 1ull << (8 * ks - 1), field = ks == 8 ? ~0ull : (1ull << (8 * ks)) - 1;
	uint64_t o = x;
	if (kt == CLO_HALF || kt == CLO_FLOAT || kt == CLO_DOUBLE) o = x ^ ((x & sign) ? field : sign);
	else if (kt == CLO_CHAR || kt == CLO_SHORT || kt == CLO_INT || kt == CLO_LONG) o = x ^ sign;
	return largest ? o ^ field : o;
}

static void run_segtopk(CCLContext* ctx, CCLQueue* cq, CloSegTopK* st, int which, int form, CloType ct, CloType kt, int mode, int pattern, size_t m_h,
	size_t k, int num_mode, int rows_mode, uint64_t base, int host_form) {
	GError* err = NULL;
	const size_t cs = clo_type_sizeof(ct), ks = clo_type_sizeof(kt), vs = mode_value_size[mode];
	uint64_t* counts = (uint64_t*) malloc((m_h + 1) * sizeof(uint64_t));
	for (size_t r = 0; r < m_h; ++r)
		counts[r] = pattern == PAT_ZEROS ? 0 : pattern == PAT_ONES ? 1 : pattern == PAT_ONE_BIG ? (r == m_h / 2 ? 900 : 0) : (rnd() % 3 ? rnd() % 9 : 0);
	size_t num_in = num_mode == NUM_BELOW ? m_h - (m_h + 2) / 3 : num_mode == NUM_ABOVE ? m_h + 7 : m_h;
	const size_t m = num_in < m_h ? num_in : m_h;
	uint64_t total = 0;
	for (size_t r = 0; r < m; ++r) total += counts[r];
	const size_t n = rows_mode == ROWS_ZERO ? 0 : rows_mode == ROWS_BELOW ? (size_t) (total - (total + 3) / 4) : rows_mode == ROWS_EQUAL ? (size_t) total : (size_t) total + 100;
	/* the keys: few distinct bytes, so that ties are common and the signed, unsigned and floating-point orders differ */
	unsigned char* hk = (unsigned char*) malloc(n * ks + 8);
	for (size_t i = 0; i < n * ks + 8; ++i) hk[i] = (rnd() & 3) ? (unsigned char) (rnd() & 1 ? 0xFF : 0x00) : (unsigned char) (rnd() & 0x83);
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	for (size_t i = 0; i < n * 8 + 8; ++i) hv[i] = (unsigned char) rnd();
	/* the expected rows: want[r * k + j] = the row with the j-th smallest (order key, row) of the clipped segment, or
	 * NONE for the slots that are not written */
	const uint32_t NONE = 0xffffffffu;
	const size_t slots = m_h * k;
	uint32_t* want = (uint32_t*) malloc((slots + 1) * sizeof(uint32_t));
	uint32_t* want_c = (uint32_t*) malloc((m_h + 1) * sizeof(uint32_t));
	for (size_t i = 0; i < slots; ++i) want[i] = NONE;
	uint64_t at = 0;
	for (size_t r = 0; r < m; ++r) {
		const uint64_t from = at < n ? at : n, to = at + counts[r] < n ? at + counts[r] : n;
		const size_t c = to - from < k ? (size_t) (to - from) : k;
		uint64_t last_x = 0, last_i = 0;
		for (size_t j = 0; j < c; ++j) {   /* the smallest (x, i) above the last one taken */
			uint64_t best_x = 0, best_i = to;
			for (uint64_t i = from; i < to; ++i) {
				const uint64_t x = order_of(word(hk, (size_t) i, ks), kt, which);
				if (j > 0 && (x < last_x || (x == last_x && i <= last_i))) continue;
				if (best_i == to || x < best_x) { best_x = x; best_i = i; }
			}
			want[r * k + j] = (uint32_t) best_i;
			last_x = best_x; last_i = best_i;
		}
		want_c[r] = (uint32_t) c;
		at += counts[r];
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
	const size_t held = slots + 4;   /* slots of the output allocations: those past m_h * k are checked too */
	unsigned char* got_k = (unsigned char*) malloc(held * 8);
	unsigned char* got_v = (unsigned char*) malloc(held * 8);
	uint32_t* got_c = (uint32_t*) malloc((m_h + 4) * sizeof(uint32_t));
	memset(got_k, 0xEE, held * 8);
	memset(got_v, 0xEE, held * 8);
	memset(got_c, 0xEE, (m_h + 4) * sizeof(uint32_t));
	const int with_keys = mode != MODE_ARG_NO_KEYS, with_vin = mode == MODE_V4 || mode == MODE_V8;
	size_t got = 12345;
	if (host_form) {
		CHECK(clo_segtopk_with_host_data(st, (m_h & 1) ? cq : NULL, NULL, src, num_mode == NUM_ABSENT ? NULL : &num_in, n ? hk : NULL,
			with_vin ? hv : NULL, with_keys ? got_k : NULL, vs ? got_v : NULL, got_c, &got, m_h, n, k, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[8];   /* counts or offsets, num_in, keys, values, keys out, values out, counts out, num_out */
		const size_t bytes[8] = { src_n * cs, 8, n * ks, n * vs, held * ks, held * vs, (m_h + 4) * 4, 8 };
		cl_ulong count = 12345, dn = num_in;
		for (int i = 0; i < 8; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], src, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, 8, &dn, NULL, &err);
		if (n) ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], hk, NULL, &err);
		if (n && vs) ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, bytes[4], got_k, NULL, &err);
		if (vs) ccl_buffer_enqueue_write(b[5], cq, CL_TRUE, 0, bytes[5], got_v, NULL, &err);
		ccl_buffer_enqueue_write(b[6], cq, CL_TRUE, 0, bytes[6], got_c, NULL, &err);
		ccl_buffer_enqueue_write(b[7], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_segtopk_with_device_data(st, cq, NULL, b[0], num_mode == NUM_ABSENT ? NULL : b[1], n ? b[2] : NULL, with_vin ? b[3] : NULL,
			with_keys ? b[4] : NULL, vs ? b[5] : NULL, b[6], b[7], m_h, n, k, &err);
		expect(&err, 0, "segtopk");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, bytes[4], got_k, NULL, &err);
		if (vs) ccl_buffer_enqueue_read(b[5], cq, CL_TRUE, 0, bytes[5], got_v, NULL, &err);
		ccl_buffer_enqueue_read(b[6], cq, CL_TRUE, 0, bytes[6], got_c, NULL, &err);
		ccl_buffer_enqueue_read(b[7], cq, CL_TRUE, 0, 8, &count, NULL, &err);
		expect(&err, 0, "read");
		got = (size_t) count;
		for (int i = 0; i < 8; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "%s %zu %s count size %zu key %d mode %d pattern %d m_h %zu num %d rows %d host %d"
#define WHERE_ARGS which_names[which], k, form_names[form], cs, (int) kt, mode, pattern, m_h, num_mode, rows_mode, host_form
	CHECK(got == total, WHERE ": num_out = %zu, expected %llu", WHERE_ARGS, got, (unsigned long long) total);
	const uint64_t pad_k = word((const unsigned char*) "\xEE\xEE\xEE\xEE\xEE\xEE\xEE\xEE", 0, ks);
	const uint64_t pad_v = word((const unsigned char*) "\xEE\xEE\xEE\xEE\xEE\xEE\xEE\xEE", 0, vs ? vs : 1);
	for (size_t j = 0; j < slots; ++j) {
		const uint32_t row = want[j];
		if (with_keys) {
			const uint64_t wk = row == NONE ? pad_k : word(hk, row, ks);
			CHECK(word(got_k, j, ks) == wk, WHERE ": keys_out[%zu] = %llx, expected %llx", WHERE_ARGS, j, (unsigned long long) word(got_k, j, ks), (unsigned long long) wk);
		}
		if (vs) {
			const uint64_t wv = row == NONE ? pad_v : with_vin ? word(hv, row, vs) : row;
			CHECK(word(got_v, j, vs) == wv, WHERE ": values_out[%zu] = %llx, expected %llx", WHERE_ARGS, j, (unsigned long long) word(got_v, j, vs), (unsigned long long) wv);
		}
	}
	for (size_t r = 0; r < m_h + 4; ++r)
		CHECK(got_c[r] == (r < m && k > 0 ? want_c[r] : 0xEEEEEEEEu), WHERE ": counts_out[%zu] = %x", WHERE_ARGS, r, got_c[r]);
	for (size_t i = (with_keys ? slots * ks : 0); i < held * ks; ++i) CHECK(got_k[i] == 0xEE, WHERE ": keys_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = slots * vs; i < held * 8; ++i) CHECK(got_v[i] == 0xEE, WHERE ": values_out written at byte %zu", WHERE_ARGS, i);
	free(counts); free(want); free(want_c); free(src); free(hk); free(hv); free(got_k); free(got_v); free(got_c);
}

/* offsets that descend, counts whose sum wraps 2^64, a num_in far above numel_seg: the call returns and ASan sees every
 * access */
static void test_broken_preconditions(CCLQueue* cq, CCLContext* ctx) {
	GError* err = NULL;
	enum { M = 300, N = 5000, K = 7 };
	for (int which = 0; which < 3; ++which) {
		for (int vs = 0; vs <= 8; vs += 4) {
			CloSegTopK* st = clo_segtopk_new(which_names[which & 1], which == 1 ? "counts" : "offsets", NULL, ctx, CLO_INT, (size_t) vs, CLO_ULONG, &err);
			expect(&err, 0, "clo_segtopk_new");
			if (!st) continue;
			uint64_t src[M + 1];
			static int32_t keys[N], ko[M * K];
			static uint64_t vals[N], vo[M * K];
			static cl_uint co[M];
			for (int r = 0; r <= M; ++r)
				src[r] = which == 0 ? (uint64_t) (M - r) * 20 : which == 1 ? ~0ull / 3 + rnd() : (uint64_t) rnd() % 8000;   /* descending; wrapping; unordered */
			for (int i = 0; i < N; ++i) { keys[i] = (int32_t) rnd(); vals[i] = rnd(); }
			size_t num_in = (size_t) 1 << 40, total = 0;
			CHECK(clo_segtopk_with_host_data(st, cq, NULL, src, &num_in, keys, vs ? vals : NULL, ko, vs ? vo : NULL, co, &total, M, N, K, &err), "broken preconditions %d", which);
			expect(&err, 0, "broken preconditions");
			clo_segtopk_destroy(st);
		}
	}
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	const size_t cap = clo_hip_segtopk_k_max(4, 4);
	CHECK(cap >= 256 && clo_hip_segtopk_k_max(3, 4) == 0 && clo_hip_segtopk_k_max(4, 2) == 0, "the cap");
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_segtopk_new("biggest", "counts", NULL, ctx, CLO_UINT, 0, CLO_UINT, &err), "an unknown which");
	REFUSED_NEW(clo_segtopk_new(NULL, "counts", NULL, ctx, CLO_UINT, 0, CLO_UINT, &err), "a NULL which");
	REFUSED_NEW(clo_segtopk_new("Largest", "counts", NULL, ctx, CLO_UINT, 0, CLO_UINT, &err), "a which in another case");
	REFUSED_NEW(clo_segtopk_new("largest", "lengths", NULL, ctx, CLO_UINT, 0, CLO_UINT, &err), "an unknown form");
	REFUSED_NEW(clo_segtopk_new("largest", NULL, NULL, ctx, CLO_UINT, 0, CLO_UINT, &err), "a NULL form");
	REFUSED_NEW(clo_segtopk_new("smallest", "counts", "k=4", ctx, CLO_UINT, 0, CLO_UINT, &err), "options");
	REFUSED_NEW(clo_segtopk_new("smallest", "counts", NULL, ctx, CLO_UINT, 0, CLO_INT, &err), "count_type int");
	REFUSED_NEW(clo_segtopk_new("smallest", "offsets", NULL, ctx, CLO_UINT, 0, CLO_FLOAT, &err), "count_type float");
	REFUSED_NEW(clo_segtopk_new("smallest", "counts", NULL, ctx, CLO_UINT, 2, CLO_UINT, &err), "value_size 2");
	REFUSED_NEW(clo_segtopk_new("smallest", "counts", NULL, ctx, CLO_UINT, 16, CLO_UINT, &err), "value_size 16");
	REFUSED_NEW(clo_segtopk_new("smallest", "counts", NULL, ctx, (CloType) 11, 0, CLO_UINT, &err), "an unknown key type");
	REFUSED_NEW(clo_segtopk_new("smallest", "counts", NULL, NULL, CLO_UINT, 0, CLO_UINT, &err), "no context");
	CHECK(clo_segtopk_new("small", "counts", NULL, ctx, CLO_UINT, 0, CLO_UINT, NULL) == NULL, "an unknown which, err NULL");
	CHECK(clo_segtopk_new("smallest", "counts", NULL, ctx, CLO_UINT, 3, CLO_UINT, NULL) == NULL, "value_size 3, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	memset(base, 0, 4096);   /* (the stub's device memory is the host's) */
	/* 8 segments, 16 rows of 4-byte keys and 4-byte values, k = 2: outputs of 16 slots */
	CCLBuffer* cn = ccl_buffer_new_from_device_ptr(ctx, base, 32, &err);               /* 8 counts */
	CCLBuffer* of = ccl_buffer_new_from_device_ptr(ctx, base, 36, &err);               /* 9 offsets */
	CCLBuffer* ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* ki = ccl_buffer_new_from_device_ptr(ctx, base + 80, 64, &err);          /* adjacent to ni */
	CCLBuffer* vi = ccl_buffer_new_from_device_ptr(ctx, base + 144, 64, &err);         /* adjacent to ki */
	CCLBuffer* ko = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* vo = ccl_buffer_new_from_device_ptr(ctx, base + 576, 64, &err);         /* adjacent to ko */
	CCLBuffer* co = ccl_buffer_new_from_device_ptr(ctx, base + 640, 32, &err);         /* adjacent to vo */
	CCLBuffer* no = ccl_buffer_new_from_device_ptr(ctx, base + 672, 8, &err);          /* adjacent to co */
	CCLBuffer* ko_on_cn = ccl_buffer_new_from_device_ptr(ctx, base + 28, 64, &err);    /* one shared element with the counts */
	CCLBuffer* ko_on_of = ccl_buffer_new_from_device_ptr(ctx, base + 32, 64, &err);    /* adjacent to the counts, on the 9th offset */
	CCLBuffer* vo_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 76, 64, &err);    /* the second half of num_in */
	CCLBuffer* ko_on_ki = ccl_buffer_new_from_device_ptr(ctx, base + 140, 64, &err);   /* the last row of keys_in */
	CCLBuffer* vo_on_vi = ccl_buffer_new_from_device_ptr(ctx, base + 204, 64, &err);   /* the last row of values_in */
	CCLBuffer* vo_on_ko = ccl_buffer_new_from_device_ptr(ctx, base + 572, 64, &err);   /* the last slot of keys_out */
	CCLBuffer* co_on_vo = ccl_buffer_new_from_device_ptr(ctx, base + 636, 32, &err);   /* the last slot of values_out */
	CCLBuffer* co_on_ki = ccl_buffer_new_from_device_ptr(ctx, base + 112, 32, &err);
	CCLBuffer* no_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 568, 8, &err);
	CCLBuffer* no_in_co = ccl_buffer_new_from_device_ptr(ctx, base + 648, 8, &err);
	CCLBuffer* no_in_cn = ccl_buffer_new_from_device_ptr(ctx, base + 8, 8, &err);
	CCLBuffer* no_on_ni = ccl_buffer_new_from_device_ptr(ctx, base + 72, 8, &err);
	CCLBuffer* no_odd = ccl_buffer_new_from_device_ptr(ctx, base + 708, 8, &err);      /* not 8-byte aligned */
	CCLBuffer* no_small = ccl_buffer_new_from_device_ptr(ctx, base + 712, 4, &err);
	CCLBuffer* ni_odd = ccl_buffer_new_from_device_ptr(ctx, base + 1028, 8, &err);
	CCLBuffer* ni_small = ccl_buffer_new_from_device_ptr(ctx, base + 1032, 4, &err);
	CCLBuffer* cn_short = ccl_buffer_new_from_device_ptr(ctx, base, 28, &err);
	CCLBuffer* ki_short = ccl_buffer_new_from_device_ptr(ctx, base + 80, 60, &err);
	CCLBuffer* ko_short = ccl_buffer_new_from_device_ptr(ctx, base + 2048, 60, &err);  /* 15 slots */
	CCLBuffer* vo_short = ccl_buffer_new_from_device_ptr(ctx, base + 2112, 60, &err);
	CCLBuffer* co_short = ccl_buffer_new_from_device_ptr(ctx, base + 2176, 28, &err);  /* 7 counts */
	expect(&err, 0, "buffers");
	uint32_t hc[9] = { 0 }, hk[16] = { 0 }, hv[16] = { 0 }, hko[24], hvo[24];
	cl_uint hco[12];
	for (int i = 0; i < 24; ++i) { hko[i] = 0xABCD0000u + (uint32_t) i; hvo[i] = 0xDCBA0000u + (uint32_t) i; }
	for (int i = 0; i < 12; ++i) hco[i] = 0xC0C00000u + (uint32_t) i;
	size_t hn = 777, hm = 8;
	CloSegTopK* k0 = clo_segtopk_new("smallest", "counts", NULL, ctx, CLO_UINT, 0, CLO_UINT, &err);
	CloSegTopK* c4 = clo_segtopk_new("largest", "counts", NULL, ctx, CLO_UINT, 4, CLO_UINT, &err);
	CloSegTopK* o4 = clo_segtopk_new("smallest", "offsets", "", ctx, CLO_FLOAT, 4, CLO_UINT, &err);
	CloSegTopK* c8 = clo_segtopk_new("largest", "counts", NULL, ctx, CLO_SHORT, 8, CLO_ULONG, &err);
	expect(&err, 0, "objects");
	if (!k0 || !c4 || !o4 || !c8) return;
	CHECK(clo_segtopk_get_context(o4) == ctx && clo_segtopk_get_key_type(o4) == CLO_FLOAT && clo_segtopk_get_key_size(o4) == 4
		&& clo_segtopk_get_key_type(c8) == CLO_SHORT && clo_segtopk_get_key_size(c8) == 2 && clo_segtopk_get_value_size(c8) == 8
		&& clo_segtopk_get_value_size(k0) == 0 && clo_segtopk_get_value_size(c4) == 4 && clo_segtopk_get_count_type(c8) == CLO_ULONG
		&& clo_segtopk_get_count_size(c8) == 8 && clo_segtopk_get_count_size(c4) == 4 && !strcmp(clo_segtopk_get_form(c4), "counts")
		&& !strcmp(clo_segtopk_get_form(o4), "offsets") && !strcmp(clo_segtopk_get_which(c4), "largest") && !strcmp(clo_segtopk_get_which(o4), "smallest"),
		"getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define DEV(obj, a, b, c, d, e, f, g, h, m_h, n, k) clo_segtopk_with_device_data(obj, cq, NULL, a, b, c, d, e, f, g, h, m_h, n, k, &err)
#define HOST(obj, a, b, c, d, e, f, g, h, m_h, n, k) clo_segtopk_with_host_data(obj, cq, NULL, a, b, c, d, e, f, g, h, m_h, n, k, &err)
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no, (size_t) 1 << 32, 16, 2), "numel_seg 2^32");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no, 8, (size_t) 1 << 32, 2), "numel 2^32");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hvo, hco, &hn, (size_t) 1 << 32, 16, 2), "numel_seg 2^32, host");
	REFUSED_HOST(HOST(o4, hc, NULL, hk, hv, hko, hvo, hco, &hn, 8, (size_t) 1 << 33, 2), "numel 2^33, host");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no, 8, 16, cap + 1), "k above the cap");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hvo, hco, &hn, 8, 16, cap + 1), "k above the cap, host");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hvo, hco, &hn, 8, 16, (size_t) 1 << 40), "k 2^40, host");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hvo, hco, &hn, (size_t) 1 << 24, 16, 256), "numel_seg * k = 2^32, host");
	REFUSED_DEV(DEV(c4, NULL, NULL, ki, vi, ko, vo, co, no, 8, 16, 2), "counts NULL");
	REFUSED_HOST(HOST(o4, NULL, NULL, hk, hv, hko, hvo, hco, &hn, 8, 16, 2), "offsets NULL, host");
	REFUSED_DEV(DEV(o4, NULL, NULL, NULL, NULL, ko, vo, co, no, 0, 0, 2), "offsets NULL with numel_seg 0");
	REFUSED_DEV(DEV(c4, cn, NULL, NULL, vi, ko, vo, co, no, 8, 16, 2), "keys_in NULL");
	REFUSED_HOST(HOST(c4, hc, NULL, NULL, hv, hko, hvo, hco, &hn, 8, 16, 2), "keys_in NULL, host");
	REFUSED_DEV(DEV(k0, cn, NULL, ki, vi, ko, NULL, co, no, 8, 16, 2), "values_in with value_size 0");
	REFUSED_DEV(DEV(k0, cn, NULL, ki, NULL, ko, vo, co, no, 8, 16, 2), "values_out with value_size 0");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, NULL, co, no, 8, 16, 2), "values_out NULL with value_size 4");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, NULL, hko, NULL, hco, &hn, 8, 16, 2), "values_out NULL in the arg form, host");
	REFUSED_DEV(DEV(c8, cn, NULL, ki, NULL, ko, vo, co, no, 4, 8, 1), "values_in NULL with value_size 8");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, NULL, vo, co, no, 8, 16, 2), "keys_out NULL outside the arg form");
	REFUSED_DEV(DEV(k0, cn, NULL, ki, NULL, NULL, NULL, co, no, 8, 16, 2), "keys_out NULL with value_size 0");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, NULL, no, 8, 16, 2), "counts_out NULL");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hvo, NULL, &hn, 8, 16, 2), "counts_out NULL, host");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, NULL, 8, 16, 2), "num_out NULL");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hvo, hco, NULL, 8, 16, 2), "num_out NULL, host");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no_odd, 8, 16, 2), "num_out misaligned");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no_small, 8, 16, 2), "num_out of 4 bytes");
	REFUSED_DEV(DEV(c4, cn, ni_odd, ki, vi, ko, vo, co, no, 8, 16, 2), "num_in misaligned");
	REFUSED_DEV(DEV(c4, cn, ni_small, ki, vi, ko, vo, co, no, 8, 16, 2), "num_in of 4 bytes");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no, 9, 16, 1), "numel_seg beyond the counts");
	REFUSED_DEV(DEV(o4, cn, NULL, ki, vi, ko, vo, co, no, 8, 16, 2), "8 offsets for 8 segments");
	REFUSED_DEV(DEV(c4, cn_short, NULL, ki, vi, ko, vo, co, no, 8, 16, 2), "counts below numel_seg");
	REFUSED_DEV(DEV(c4, cn, NULL, ki_short, vi, ko, vo, co, no, 8, 16, 2), "keys_in below numel rows");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no, 8, 17, 2), "numel beyond the rows");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no, 8, 16, 3), "k beyond the outputs' slots");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko_short, vo, co, no, 8, 16, 2), "keys_out below numel_seg * k slots");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo_short, co, no, 8, 16, 2), "values_out below numel_seg * k slots");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co_short, no, 8, 16, 2), "counts_out below numel_seg");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, cn, vo, co, no, 8, 16, 1), "keys_out on the counts");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko_on_cn, vo, co, no, 8, 16, 2), "keys_out sharing the counts' last element");
	REFUSED_DEV(DEV(o4, of, NULL, ki, vi, ko_on_of, vo, co, no, 8, 16, 2), "keys_out on the last offset");
	REFUSED_DEV(DEV(c4, cn, ni, ki, vi, ko, vo_on_ni, co, no, 8, 16, 2), "values_out on num_in");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko_on_ki, vo, co, no, 8, 16, 2), "keys_out on keys_in's last row");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ki, vo, co, no, 8, 16, 2), "keys_out on keys_in: no in-place form");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo_on_vi, co, no, 8, 16, 2), "values_out on values_in's last row");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo_on_ko, co, no, 8, 16, 2), "values_out on keys_out's last slot");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, ko, co, no, 8, 16, 2), "values_out on keys_out");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co_on_vo, no, 8, 16, 2), "counts_out on values_out's last slot");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co_on_ki, no, 8, 16, 2), "counts_out inside keys_in");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, cn, no, 8, 16, 2), "counts_out on the counts");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no_in_ko, 8, 16, 2), "num_out inside keys_out");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no_in_co, 8, 16, 2), "num_out inside counts_out");
	REFUSED_DEV(DEV(c4, cn, NULL, ki, vi, ko, vo, co, no_in_cn, 8, 16, 2), "num_out inside the counts");
	REFUSED_DEV(DEV(c4, cn, ni, ki, vi, ko, vo, co, no_on_ni, 8, 16, 2), "num_out on num_in");
	REFUSED_HOST(HOST(c4, hko + 8, NULL, hk, hv, hko, hvo, hco, &hn, 8, 16, 2), "the counts inside keys_out, host");
	REFUSED_HOST(HOST(c4, hc, NULL, hvo + 15, hv, hko, hvo, hco, &hn, 8, 8, 2), "keys_in on values_out's last slot, host");
	REFUSED_HOST(HOST(c4, hc, (size_t*) (hko + 2), hk, hv, hko, hvo, hco, &hn, 8, 16, 2), "num_in inside keys_out, host");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hvo, hco, (size_t*) (hvo + 14), 8, 16, 2), "num_out inside values_out, host");
	REFUSED_HOST(HOST(c4, hc, &hn, hk, hv, hko, hvo, hco, &hn, 8, 16, 2), "num_out on num_in, host");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hko + 15, hco, &hn, 8, 16, 2), "values_out on keys_out's last slot, host");
	REFUSED_HOST(HOST(c4, hc, NULL, hk, hv, hko, hvo, (cl_uint*) (hvo + 15), &hn, 8, 16, 2), "counts_out on values_out's last slot, host");
	/* err == NULL */
	CHECK(clo_segtopk_with_device_data(c4, cq, NULL, cn, NULL, ki, vi, cn, vo, co, no, 8, 16, 1, NULL) == NULL, "keys_out on the counts, err NULL");
	CHECK(clo_segtopk_with_device_data(c4, cq, NULL, cn, NULL, ki, vi, ko, vo, co, NULL, 8, 16, 2, NULL) == NULL, "num_out NULL, err NULL");
	CHECK(clo_segtopk_with_device_data(c4, cq, NULL, cn, NULL, ki, vi, ko, vo, co, no, 8, 16, cap + 1, NULL) == NULL, "k above the cap, err NULL");
	CHECK(!clo_segtopk_with_host_data(c4, NULL, NULL, hc, NULL, hk, hv, hko, hvo, hco, &hn, (size_t) 1 << 32, 16, 2, NULL), "numel_seg 2^32, host, err NULL");
	CHECK(!clo_segtopk_with_host_data(c4, NULL, NULL, hc, NULL, hk, hv, NULL, hvo, hco, &hn, 8, 16, 2, NULL), "keys_out NULL, host, err NULL");
	for (int i = 0; i < 24; ++i) CHECK(hko[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0xDCBA0000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	for (int i = 0; i < 12; ++i) CHECK(hco[i] == 0xC0C00000u + (uint32_t) i, "a refused call wrote counts_out at %d", i);
	CHECK(hn == 777 && hm == 8, "a refused call wrote num_out or num_in");
	for (int i = 0; i < 4096; ++i) CHECK(base[i] == 0, "a refused call wrote device memory at %d", i);
	/* adjacent, disjoint views of one allocation are accepted */
	CHECK(DEV(c4, cn, ni, ki, vi, ko, vo, co, no, 8, 16, 2) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(DEV(o4, of, ni, ki, NULL, NULL, vo, co, no, 8, 16, 2) != NULL, "disjoint views of one allocation, offsets, arg form without keys_out");
	expect(&err, 0, "disjoint views of one allocation, offsets");
	/* m == 0: success, num_out 0, nothing else written, no queue needed in the host form, inputs may be NULL */
	CHECK(clo_segtopk_with_host_data(c4, NULL, NULL, NULL, NULL, hk, hv, hko, hvo, NULL, &hn, 0, 16, 2, &err), "empty, host");
	expect(&err, 0, "empty, host");
	CHECK(hn == 0, "empty, host: num_out %zu", hn);
	hn = 777; hm = 0;
	CHECK(clo_segtopk_with_host_data(o4, NULL, NULL, hc, &hm, hk, hv, hko, hvo, hco, &hn, 8, 16, 2, &err), "num_in 0, host");
	expect(&err, 0, "num_in 0, host");
	CHECK(hn == 0, "num_in 0, host: num_out %zu", hn);
	/* k == 0: success, num_out = total, nothing else written; counts_out may be NULL */
	for (int r = 0; r < 8; ++r) hc[r] = 2;
	hn = 777;
	CHECK(clo_segtopk_with_host_data(c4, cq, NULL, hc, NULL, hk, hv, hko, hvo, NULL, &hn, 8, 16, 0, &err), "k 0, host");
	expect(&err, 0, "k 0, host");
	CHECK(hn == 16, "k 0, host: num_out %zu", hn);
	cl_ulong dn = 777;
	ccl_buffer_enqueue_write(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	CHECK(DEV(c4, NULL, NULL, ki, vi, ko, vo, NULL, no, 0, 16, 2) != NULL, "empty, device");
	expect(&err, 0, "empty, device");
	ccl_buffer_enqueue_read(no, cq, CL_TRUE, 0, 8, &dn, NULL, &err);
	expect(&err, 0, "read");
	CHECK(dn == 0, "empty, device: num_out %llu", (unsigned long long) dn);
	for (int i = 0; i < 24; ++i) CHECK(hko[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0xDCBA0000u + (uint32_t) i, "an empty call wrote an output at %d", i);
	for (int i = 0; i < 12; ++i) CHECK(hco[i] == 0xC0C00000u + (uint32_t) i, "an empty call wrote counts_out at %d", i);

	clo_segtopk_destroy(k0); clo_segtopk_destroy(c4); clo_segtopk_destroy(o4); clo_segtopk_destroy(c8);
	CCLBuffer* all[] = { cn, of, ni, ki, vi, ko, vo, co, no, ko_on_cn, ko_on_of, vo_on_ni, ko_on_ki, vo_on_vi, vo_on_ko, co_on_vo, co_on_ki, no_in_ko, no_in_co,
		no_in_cn, no_on_ni, no_odd, no_small, ni_odd, ni_small, cn_short, ki_short, ko_short, vo_short, co_short, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType count_types[2] = { CLO_UINT, CLO_ULONG };
	static const CloType key_types[] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };
	const size_t cap = clo_hip_segtopk_k_max(4, 0);
	/* large -> small -> large on one object per which, form, count type, key type and mode; the patterns, k, the num_in
	 * and row modes and the two forms of the call take turns */
	static const size_t sizes[] = { 300, 7, 1, 450 };
	const size_t ks_[] = { 1, 2, 3, 8, 5, cap, 64, 0 };
	unsigned turn = 0;
	for (int form = 0; form < 2; ++form) {
		for (int c = 0; c < 2; ++c) {
			for (size_t kt = 0; kt < sizeof(key_types) / sizeof(key_types[0]); ++kt) {
				for (int mode = 0; mode < MODE_COUNT; ++mode) {
					const int which = (int) ((turn / 4) & 1);
					CloSegTopK* st = clo_segtopk_new(which_names[which], form_names[form], NULL, ctx, key_types[kt], mode_value_size[mode], count_types[c], &err);
					expect(&err, 0, "clo_segtopk_new");
					if (!st) continue;
					for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z, ++turn) {
						size_t k = ks_[turn % (sizeof(ks_) / sizeof(ks_[0]))];
						if (k == cap && sizes[z] > 7) k = 9;   /* (the cap on a few segments only: the slots are checked one by one) */
						run_segtopk(ctx, cq, st, which, form, count_types[c], key_types[kt], mode, (int) (turn % PAT_COUNT), sizes[z], k, (int) (turn % NUM_MODES),
							(int) ((turn / PAT_COUNT) % ROWS_MODES), form ? 12345u * (turn % 3) : 0, (int) ((turn / 7) & 1));
					}
					clo_segtopk_destroy(st);
				}
			}
		}
	}
	/* every pattern x every row mode x every num_in mode x both forms of the call x both which */
	for (int form = 0; form < 2; ++form) {
		for (int which = 0; which < 2; ++which) {
			CloSegTopK* st = clo_segtopk_new(which_names[which], form_names[form], NULL, ctx, CLO_INT, 4, CLO_UINT, &err);
			expect(&err, 0, "clo_segtopk_new");
			for (int pattern = 0; st && pattern < PAT_COUNT; ++pattern)
				for (int rows_mode = 0; rows_mode < ROWS_MODES; ++rows_mode)
					for (int num_mode = 0; num_mode < NUM_MODES; ++num_mode)
						for (int host_form = 0; host_form < 2; ++host_form)
							run_segtopk(ctx, cq, st, which, form, CLO_UINT, CLO_INT, MODE_V4 + 2 * (num_mode & 1), pattern, 133, pattern == PAT_ONE_BIG ? cap : 4,
								num_mode, rows_mode, form ? 777 : 0, host_form);
			if (st) clo_segtopk_destroy(st);
		}
	}
	test_broken_preconditions(cq, ctx);
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("segtopk host ok\n");
	return failures ? 1 : 0;
}
