/*
 * topk_host_test.c — CloTopK (include/clo_topk.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_topk_cpu.py). Both directions and both orders,
 * every key type; keys only, 4- and 8-byte values, the arg form with and without keys_out, the k-th key alone; k 0, 1,
 * inside a tie run, numel, above numel; numel 0; outputs of exactly m rows; the host-data form; one object used large ->
 * small -> large (its workspace grows once and is reused); every refusal the driver makes (err == NULL included), with
 * the outputs left alone; a clean destroy. The expected rows are computed here by a qsort of the indices
 * under signed / unsigned / sign-magnitude comparisons of the keys, not taken from the stub.
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

enum { KEYS_ONLY, VAL4, VAL8, ARG, ARG_ONLY, KTH_ONLY };
static const char* const which_names[2] = { "smallest", "largest" };
static const char* const order_names[2] = { "input", "sorted" };

/* the sort the contract names, as a qsort of indices: by key (reversed for "largest"), ties by index */
static const uint64_t* cmp_bits;
static size_t cmp_ks;
static int cmp_kind, cmp_largest;
static int by_key_then_index(const void* a, const void* b) {
	const uint32_t i = *(const uint32_t*) a, j = *(const uint32_t*) b;
	int c = compare_keys(cmp_bits[i], cmp_bits[j], cmp_ks, cmp_kind);
	if (cmp_largest) c = -c;
	return c ? c : i < j ? -1 : i > j;
}
static int by_index(const void* a, const void* b) {
	const uint32_t i = *(const uint32_t*) a, j = *(const uint32_t*) b;
	return i < j ? -1 : i > j;
}

static void run_topk(CCLContext* ctx, CCLQueue* cq, CloTopK* topk, int which, int order, CloType kt, int mode, size_t n, size_t k, int host_form) {
	GError* err = NULL;
	const size_t ks = clo_type_sizeof(kt), vs = mode == KEYS_ONLY || mode == KTH_ONLY ? 0 : mode == VAL8 ? 8 : 4;
	const int kind = kind_of(kt), vals = mode == VAL4 || mode == VAL8, keys_out = mode != ARG_ONLY && mode != KTH_ONLY;
	const size_t m = k < n ? k : n;
	unsigned char* hk = (unsigned char*) malloc(n * ks + 8);
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	uint64_t* bits = (uint64_t*) malloc((n + 1) * sizeof(uint64_t));
	/* few distinct keys around the type's sign change: every cut falls inside a tie run */
	for (size_t i = 0; i < n; ++i) {
		uint64_t b = (uint64_t) (rnd() % 23) - 11u;   /* -11 .. 11 as two's complement */
		if (kind == 2) b = (rnd() & 1 ? 1ull << (8 * ks - 1) : 0ull) | (rnd() % 7);   /* +-0 and small denormals */
		bits[i] = ks == 8 ? b : b & ((1ull << (8 * ks)) - 1ull);
		const uint64_t v = ((uint64_t) rnd() << 32) | rnd();
		memcpy(hk + i * ks, &bits[i], ks);
		memcpy(hv + i * vs, &v, vs);
	}
	/* the expected rows: the m first of the sort; then by index for "input" */
	uint32_t* want_p = (uint32_t*) malloc((n + 1) * sizeof(uint32_t));
	for (size_t i = 0; i < n; ++i) want_p[i] = (uint32_t) i;
	cmp_bits = bits; cmp_ks = ks; cmp_kind = kind; cmp_largest = which;
	qsort(want_p, n, sizeof(uint32_t), by_key_then_index);
	const uint32_t kth_index = m ? want_p[m - 1] : 0;
	if (order == 0) qsort(want_p, m, sizeof(uint32_t), by_index);
	/* outputs of exactly m rows, so that a write at row m shows under ASan; 8 spare bytes of canary in the host form only */
	unsigned char* got_k = (unsigned char*) malloc(m * ks + 8);
	unsigned char* got_v = (unsigned char*) malloc(m * 8 + 8);
	memset(got_k, 0xEE, m * ks + 8);
	memset(got_v, 0xEE, m * 8 + 8);
	uint64_t kth = 0xEEEEEEEEEEEEEEEEull;
	if (host_form) {
		CHECK(clo_topk_with_host_data(topk, (n & 1) ? cq : NULL, NULL, hk, vals ? hv : NULL, keys_out ? got_k : NULL, vs ? got_v : NULL,
			(k & 1) || mode == KTH_ONLY ? &kth : NULL, n, k, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[5];   /* keys, values, keys out, values out, the k-th key */
		const size_t bytes[5] = { n * ks, n * vs, m * ks, m * vs, ks };
		for (int i = 0; i < 5; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] ? bytes[i] : 1, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], hk, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, bytes[1], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2], got_k, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3], got_v, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, ks, &kth, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_topk_with_device_data(topk, cq, NULL, b[0], vals ? b[1] : NULL, keys_out ? b[2] : NULL, vs ? b[3] : NULL,
			(k & 1) || mode == KTH_ONLY ? b[4] : NULL, n, k, &err);
		expect(&err, 0, "topk");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[2], cq, CL_TRUE, 0, bytes[2], got_k, NULL, &err);
		ccl_buffer_enqueue_read(b[3], cq, CL_TRUE, 0, bytes[3], got_v, NULL, &err);
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, ks, &kth, NULL, &err);
		expect(&err, 0, "read");
		for (int i = 0; i < 5; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "%s %s key type %d mode %d n %zu k %zu host %d"
#define WHERE_ARGS which_names[which], order_names[order], (int) kt, mode, n, k, host_form
	for (size_t j = 0; j < m; ++j) {
		const size_t i = want_p[j];
		if (keys_out) CHECK(memcmp(got_k + j * ks, hk + i * ks, ks) == 0, WHERE ": wrong key in row %zu", WHERE_ARGS, j);
		if (vals) CHECK(memcmp(got_v + j * vs, hv + i * vs, vs) == 0, WHERE ": wrong value in row %zu", WHERE_ARGS, j);
		else if (vs) CHECK(memcmp(got_v + j * 4, &want_p[j], 4) == 0, WHERE ": wrong index in row %zu", WHERE_ARGS, j);
	}
	for (size_t i = keys_out ? m * ks : 0; i < m * ks + 8; ++i) CHECK(got_k[i] == 0xEE, WHERE ": keys_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = m * vs; i < m * 8 + 8; ++i) CHECK(got_v[i] == 0xEE, WHERE ": values_out written at byte %zu", WHERE_ARGS, i);
	if (((k & 1) || mode == KTH_ONLY) && m > 0) CHECK(memcmp(&kth, hk + (size_t) kth_index * ks, ks) == 0, WHERE ": wrong k-th key", WHERE_ARGS);
	else CHECK(kth == 0xEEEEEEEEEEEEEEEEull, WHERE ": kth_out written", WHERE_ARGS);
	free(hk); free(hv); free(bits); free(want_p); free(got_k); free(got_v);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_topk_new("smallest", "input", NULL, ctx, CLO_UINT, 2, &err), "value_size 2");
	REFUSED_NEW(clo_topk_new("smallest", "input", NULL, ctx, CLO_UINT, 16, &err), "value_size 16");
	REFUSED_NEW(clo_topk_new("smallest", "input", "descending", ctx, CLO_UINT, 0, &err), "options");
	REFUSED_NEW(clo_topk_new("smallest", "input", NULL, ctx, (CloType) 11, 0, &err), "an unknown key type");
	REFUSED_NEW(clo_topk_new("least", "input", NULL, ctx, CLO_UINT, 0, &err), "an unknown which");
	REFUSED_NEW(clo_topk_new(NULL, "input", NULL, ctx, CLO_UINT, 0, &err), "a NULL which");
	REFUSED_NEW(clo_topk_new("Largest", "input", NULL, ctx, CLO_UINT, 0, &err), "a which in another case");
	REFUSED_NEW(clo_topk_new("largest", "ascending", NULL, ctx, CLO_UINT, 0, &err), "an unknown order");
	REFUSED_NEW(clo_topk_new("largest", NULL, NULL, ctx, CLO_UINT, 0, &err), "a NULL order");
	CHECK(clo_topk_new("smallest", "input", NULL, ctx, CLO_UINT, 3, NULL) == NULL, "value_size 3, err NULL");
	CHECK(clo_topk_new("small", "input", NULL, ctx, CLO_UINT, 4, NULL) == NULL, "an unknown which, err NULL");
	CHECK(clo_topk_new("smallest", "sort", NULL, ctx, CLO_UINT, 4, NULL) == NULL, "an unknown order, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 65536, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* ki = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);               /* 16 uint keys */
	CCLBuffer* vi = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);          /* adjacent to ki */
	CCLBuffer* ko = ccl_buffer_new_from_device_ptr(ctx, base + 512, 32, &err);         /* 8 rows */
	CCLBuffer* vo = ccl_buffer_new_from_device_ptr(ctx, base + 544, 32, &err);         /* adjacent to ko */
	CCLBuffer* vo8 = ccl_buffer_new_from_device_ptr(ctx, base + 1024, 64, &err);
	CCLBuffer* kth = ccl_buffer_new_from_device_ptr(ctx, base + 576, 4, &err);         /* adjacent to vo */
	CCLBuffer* ko_on_ki = ccl_buffer_new_from_device_ptr(ctx, base + 60, 32, &err);    /* one shared element with ki */
	CCLBuffer* vo_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 540, 32, &err);   /* starts on ko's row m - 1 */
	CCLBuffer* kth_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 540, 4, &err);   /* ko's row 7 */
	CCLBuffer* kth_in_ki = ccl_buffer_new_from_device_ptr(ctx, base + 8, 4, &err);
	CCLBuffer* kth_odd = ccl_buffer_new_from_device_ptr(ctx, base + 578, 4, &err);     /* not aligned to the key */
	CCLBuffer* kth_small = ccl_buffer_new_from_device_ptr(ctx, base + 580, 2, &err);
	CCLBuffer* ko_short = ccl_buffer_new_from_device_ptr(ctx, base + 2048, 28, &err);  /* 7 rows: one below m = 8 */
	CCLBuffer* large_in = ccl_buffer_new_from_device_ptr(ctx, base + 4096, 4 * 5000, &err);
	CCLBuffer* large_out = ccl_buffer_new_from_device_ptr(ctx, base + 32768, 4 * 5000, &err);
	expect(&err, 0, "buffers");
	uint32_t h[16] = { 0 }, hv[16] = { 0 }, ho[24], hvo[24], hk = 777;
	for (int i = 0; i < 24; ++i) { ho[i] = 0xABCD0000u + (uint32_t) i; hvo[i] = 0x12340000u + (uint32_t) i; }
	CloTopK* s0 = clo_topk_new("smallest", "input", NULL, ctx, CLO_UINT, 0, &err);
	CloTopK* s4 = clo_topk_new("largest", "input", "", ctx, CLO_UINT, 4, &err);
	CloTopK* s8 = clo_topk_new("smallest", "input", NULL, ctx, CLO_UINT, 8, &err);
	CloTopK* so = clo_topk_new("largest", "sorted", NULL, ctx, CLO_UINT, 0, &err);
	expect(&err, 0, "objects");
	if (!s0 || !s4 || !s8 || !so) return;
	CHECK(clo_topk_get_context(s4) == ctx && clo_topk_get_key_type(s4) == CLO_UINT && clo_topk_get_key_size(s4) == 4
		&& clo_topk_get_value_size(s4) == 4 && clo_topk_get_value_size(s0) == 0 && clo_topk_get_value_size(s8) == 8
		&& !strcmp(clo_topk_get_which(s4), "largest") && !strcmp(clo_topk_get_which(s0), "smallest")
		&& !strcmp(clo_topk_get_order(so), "sorted") && !strcmp(clo_topk_get_order(s4), "input"), "getters");
	const size_t cap = clo_hip_topk_sorted_max(4, 0);
	CHECK(cap >= 1024 && cap < 5000, "the cap of the sorted order: %zu", cap);

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko, NULL, kth, (size_t) 1 << 32, 8, &err), "numel 2^32");
	REFUSED_HOST(clo_topk_with_host_data(s4, cq, NULL, h, hv, ho, hvo, &hk, (size_t) 1 << 32, 8, &err), "numel 2^32, host");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, NULL, NULL, ko, NULL, kth, 16, 8, &err), "keys_in NULL");
	REFUSED_HOST(clo_topk_with_host_data(s4, cq, NULL, NULL, NULL, NULL, hvo, NULL, 16, 8, &err), "keys_in NULL in arg form, host");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, vi, ko, NULL, kth, 16, 8, &err), "values with value_size 0");
	REFUSED_HOST(clo_topk_with_host_data(s0, cq, NULL, h, NULL, ho, hvo, NULL, 16, 8, &err), "values_out with value_size 0, host");
	REFUSED_DEV(clo_topk_with_device_data(s4, cq, NULL, ki, vi, ko, NULL, kth, 16, 8, &err), "values_out NULL");
	REFUSED_DEV(clo_topk_with_device_data(s8, cq, NULL, ki, NULL, ko, vo8, NULL, 8, 8, &err), "NULL values with value_size 8");
	REFUSED_HOST(clo_topk_with_host_data(s8, cq, NULL, h, NULL, ho, hvo, NULL, 8, 8, &err), "NULL values with value_size 8, host");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, NULL, NULL, NULL, 16, 8, &err), "both outputs and kth_out NULL");
	REFUSED_HOST(clo_topk_with_host_data(s0, cq, NULL, h, NULL, NULL, NULL, NULL, 16, 8, &err), "both outputs and kth_out NULL, host");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ki, NULL, NULL, 16, 8, &err), "in place");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko_on_ki, NULL, NULL, 16, 8, &err), "keys_out sharing keys_in's last element");
	REFUSED_DEV(clo_topk_with_device_data(s4, cq, NULL, ki, vi, ko, vo_in_ko, NULL, 16, 8, &err), "values_out on keys_out's row m - 1");
	REFUSED_DEV(clo_topk_with_device_data(s4, cq, NULL, ki, vi, ko, vi, NULL, 16, 8, &err), "values_out on values_in");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko, NULL, kth_in_ko, 16, 8, &err), "kth_out inside keys_out");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko, NULL, kth_in_ki, 16, 8, &err), "kth_out inside keys_in");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko, NULL, kth_odd, 16, 8, &err), "kth_out misaligned");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko, NULL, kth_small, 16, 8, &err), "kth_out below one key");
	REFUSED_HOST(clo_topk_with_host_data(s0, cq, NULL, h, NULL, ho, NULL, (char*) &hk + 1, 16, 8, &err), "kth_out misaligned, host");
	REFUSED_HOST(clo_topk_with_host_data(s4, cq, NULL, h, hv, ho, ho + 7, NULL, 16, 8, &err), "values_out on keys_out's last row, host");
	REFUSED_HOST(clo_topk_with_host_data(s0, cq, NULL, ho + 4, NULL, ho, NULL, NULL, 16, 8, &err), "keys_in inside keys_out, host");
	REFUSED_HOST(clo_topk_with_host_data(s0, cq, NULL, h, NULL, ho, NULL, ho + 7, 16, 8, &err), "kth_out inside keys_out, host");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko, NULL, NULL, 17, 8, &err), "numel beyond keys_in");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko_short, NULL, NULL, 16, 8, &err), "keys_out of m - 1 rows");
	REFUSED_DEV(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ko, NULL, NULL, 16, 9, &err), "k one above keys_out's rows");
	REFUSED_DEV(clo_topk_with_device_data(so, cq, NULL, large_in, NULL, large_out, NULL, NULL, 5000, cap + 1, &err), "sorted above the cap");
	REFUSED_HOST(clo_topk_with_host_data(so, cq, NULL, h, NULL, ho, NULL, NULL, 5000, 5000, &err), "sorted above the cap, host");
	/* err == NULL */
	CHECK(clo_topk_with_device_data(s0, cq, NULL, ki, NULL, ki, NULL, NULL, 16, 8, NULL) == NULL, "in place, err NULL");
	CHECK(clo_topk_with_device_data(so, cq, NULL, large_in, NULL, large_out, NULL, NULL, 5000, cap + 1, NULL) == NULL, "sorted above the cap, err NULL");
	CHECK(!clo_topk_with_host_data(s4, NULL, NULL, h, hv, ho, hvo, NULL, (size_t) 1 << 32, 8, NULL), "numel 2^32, host, err NULL");
	CHECK(!clo_topk_with_host_data(s0, NULL, NULL, h, NULL, NULL, NULL, NULL, 16, 8, NULL), "everything NULL, host, err NULL");
	for (int i = 0; i < 24; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	CHECK(hk == 777, "a refused call wrote kth_out");
	/* accepted: adjacent, disjoint views of one allocation; an output of exactly m rows; the cap itself; k above numel
	 * with outputs of numel rows */
	CHECK(clo_topk_with_device_data(s4, cq, NULL, ki, vi, ko, vo, kth, 16, 8, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_topk_with_device_data(so, cq, NULL, large_in, NULL, large_out, NULL, NULL, 5000, cap, &err) != NULL, "sorted at the cap");
	expect(&err, 0, "sorted at the cap");
	CHECK(clo_topk_with_device_data(s0, cq, NULL, ko, NULL, ki, NULL, NULL, 8, 1000, &err) != NULL, "k above numel");
	expect(&err, 0, "k above numel");
	/* numel 0 and k 0: success, nothing written, no queue needed in the host form, inputs may be NULL */
	CHECK(clo_topk_with_host_data(s4, NULL, NULL, NULL, NULL, ho, hvo, &hk, 0, 5, &err), "empty, host");
	expect(&err, 0, "empty, host");
	CHECK(clo_topk_with_host_data(s4, NULL, NULL, h, hv, ho, hvo, &hk, 16, 0, &err), "k 0, host");
	expect(&err, 0, "k 0, host");
	CHECK(clo_topk_with_device_data(s4, cq, NULL, NULL, NULL, ko, vo, kth, 0, 5, &err) != NULL, "empty, device");
	expect(&err, 0, "empty, device");
	CHECK(clo_topk_with_device_data(s4, cq, NULL, ki, vi, ko, vo, kth, 16, 0, &err) != NULL, "k 0, device");
	expect(&err, 0, "k 0, device");
	for (int i = 0; i < 24; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "an empty call wrote an output at %d", i);
	CHECK(hk == 777, "an empty call wrote kth_out");

	clo_topk_destroy(s0); clo_topk_destroy(s4); clo_topk_destroy(s8); clo_topk_destroy(so);
	CCLBuffer* all[] = { ki, vi, ko, vo, vo8, kth, ko_on_ki, vo_in_ko, kth_in_ko, kth_in_ki, kth_odd, kth_small, ko_short, large_in, large_out, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType types[] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };
	/* large -> small -> large on one object per direction, order, type and mode, with numel 0 in between */
	static const size_t sizes[] = { 3001, 37, 0, 1, 5000 };
	for (int which = 0; which < 2; ++which) {
		for (int order = 0; order < 2; ++order) {
			for (size_t t = 0; t < sizeof(types) / sizeof(types[0]); ++t) {
				for (int mode = KEYS_ONLY; mode <= KTH_ONLY; ++mode) {
					CloTopK* topk = clo_topk_new(which_names[which], order_names[order], NULL, ctx, types[t],
						mode == KEYS_ONLY || mode == KTH_ONLY ? 0 : mode == VAL8 ? 8 : 4, &err);
					expect(&err, 0, "clo_topk_new");
					if (!topk) continue;
					for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z) {
						const size_t n = sizes[z];
						const size_t ks[] = { 0, 1, n / 3, n, n + 1, 10 * n + 7 };
						const size_t k = ks[(z + t + (size_t) mode) % 6];
						const size_t cap = clo_hip_topk_sorted_max((int) clo_type_sizeof(types[t]), 0);
						for (int host_form = 0; host_form < 2; ++host_form)
							run_topk(ctx, cq, topk, which, order, types[t], mode, n, order == 1 && k > cap ? cap : k, host_form);
					}
					clo_topk_destroy(topk);
				}
			}
		}
	}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("topk host ok\n");
	return failures ? 1 : 0;
}
