/*
 * bucket_host_test.c — CloBucket (include/clo_bucket.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_bucket_cpu.py). Every integer key type; keys
 * only, 4- and 8-byte values, the arg form with and without keys_out; both count types; bin counts on both sides of 256;
 * lower NULL, positive, and negative for signed keys; numel 0; the host-data form; one object used large -> small ->
 * large (its workspace grows once and is reused); every refusal the driver makes (err == NULL included), with the
 * outputs left alone; a clean destroy. The expected rows are computed here over 128-bit integers from the definition
 * (d = key - lower, in range iff d >= 0 and (d >> shift) < num_bins), not taken from the stub.
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

static int is_signed(CloType t) { return t == CLO_CHAR || t == CLO_SHORT || t == CLO_INT || t == CLO_LONG; }

/* the value of the key with these bits, as a 128-bit integer */
static __int128 value_of(uint64_t bits, size_t ks, int sg) {
	const unsigned b = 8 * (unsigned) ks;
	if (ks < 8) bits &= (1ull << b) - 1ull;
	if (sg && (bits >> (b - 1)) & 1u) return (__int128) bits - ((__int128) 1 << b);
	return (__int128) bits;
}

/* the bin from the definition, num_bins for the rest */
static size_t bin_of(uint64_t bits, uint64_t lower_bits, size_t ks, int sg, unsigned shift, size_t num_bins) {
	const __int128 d = value_of(bits, ks, sg) - value_of(lower_bits, ks, sg);
	if (d < 0) return num_bins;
	const __int128 b = d >> shift;
	return b < (__int128) num_bins ? (size_t) b : num_bins;
}

enum { KEYS_ONLY, VAL4, VAL8, ARG, ARG_ONLY };

static void run_bucket(CCLContext* ctx, CCLQueue* cq, CloBucket* bkt, CloType kt, CloType ct, int mode, size_t n, size_t num_bins,
	int lower_mode, unsigned shift, int host_form) {
	GError* err = NULL;
	const size_t ks = clo_type_sizeof(kt), vs = mode == KEYS_ONLY ? 0 : mode == VAL8 ? 8 : 4, cs = clo_type_sizeof(ct);
	const int sg = is_signed(kt), vals = mode == VAL4 || mode == VAL8, keys_out = mode != ARG_ONLY;
	/* lower: NULL (0), a small positive value, a negative one (signed keys) */
	int64_t lower_value = lower_mode == 0 ? 0 : lower_mode == 1 ? 7 : sg ? -9 : 3;
	uint64_t lower_bits = 0;
	memcpy(&lower_bits, &lower_value, ks);
	const void* lower = lower_mode == 0 ? NULL : (const void*) &lower_bits;   /* little-endian: the key's bytes come first */
	unsigned char* hk = (unsigned char*) malloc(n * ks + 8);
	unsigned char* hv = (unsigned char*) malloc(n * 8 + 8);
	uint64_t* bits = (uint64_t*) malloc((n + 1) * sizeof(uint64_t));
	/* keys around lower: some below it, most in range, some beyond the last bin; and the type's two ends */
	uint64_t span = ((uint64_t) num_bins << shift) + ((uint64_t) 40 << shift);
	if (span == 0) span = ~0ull;   /* shift 63 */
	for (size_t i = 0; i < n; ++i) {
		uint64_t b = (uint64_t) lower_value + (((uint64_t) rnd() << 16 ^ rnd()) % span) - ((uint64_t) 10 << shift);
		if (rnd() % 50 == 0) b = rnd() & 1 ? ~0ull : 1ull << (8 * ks - 1);
		bits[i] = ks == 8 ? b : b & ((1ull << (8 * ks)) - 1ull);
		const uint64_t v = ((uint64_t) rnd() << 32) | rnd();
		memcpy(hk + i * ks, &bits[i], ks);
		memcpy(hv + i * vs, &v, vs);
	}
	/* the expected rows: bin by bin, the rest last, each in input order */
	uint32_t* want_p = (uint32_t*) malloc((n + 1) * sizeof(uint32_t));
	uint64_t* want_off = (uint64_t*) calloc(num_bins + 2, sizeof(uint64_t));
	for (size_t i = 0; i < n; ++i) ++want_off[bin_of(bits[i], lower_bits, ks, sg, shift, num_bins) + 1];
	for (size_t b = 0; b <= num_bins; ++b) want_off[b + 1] += want_off[b];
	uint64_t* at = (uint64_t*) malloc((num_bins + 1) * sizeof(uint64_t));
	memcpy(at, want_off, (num_bins + 1) * sizeof(uint64_t));
	for (size_t i = 0; i < n; ++i) want_p[at[bin_of(bits[i], lower_bits, ks, sg, shift, num_bins)]++] = (uint32_t) i;
	unsigned char* got_k = (unsigned char*) malloc(n * ks + 8);
	unsigned char* got_v = (unsigned char*) malloc(n * 8 + 8);
	unsigned char* got_o = (unsigned char*) malloc((num_bins + 1) * cs + 8);
	memset(got_k, 0xEE, n * ks + 8);
	memset(got_v, 0xEE, n * 8 + 8);
	memset(got_o, 0xEE, (num_bins + 1) * cs + 8);
	if (host_form) {
		CHECK(clo_bucket_with_host_data(bkt, (n & 1) ? cq : NULL, NULL, hk, vals ? hv : NULL, keys_out ? got_k : NULL, vs ? got_v : NULL, got_o,
			n, lower, shift, num_bins, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[5];   /* keys, values, keys out, values out, the offsets */
		const size_t bytes[5] = { n * ks, n * vs, n * ks, n * vs, (num_bins + 1) * cs };
		for (int i = 0; i < 5; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], hk, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, bytes[1], hv, NULL, &err);
		ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2] + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_write(b[3], cq, CL_TRUE, 0, bytes[3] + 8, got_v, NULL, &err);
		ccl_buffer_enqueue_write(b[4], cq, CL_TRUE, 0, bytes[4] + 8, got_o, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_bucket_with_device_data(bkt, cq, NULL, b[0], vals ? b[1] : NULL, keys_out ? b[2] : NULL, vs ? b[3] : NULL, b[4],
			n, lower, shift, num_bins, &err);
		expect(&err, 0, "bucket");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[2], cq, CL_TRUE, 0, bytes[2] + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_read(b[3], cq, CL_TRUE, 0, bytes[3] + 8, got_v, NULL, &err);
		ccl_buffer_enqueue_read(b[4], cq, CL_TRUE, 0, bytes[4] + 8, got_o, NULL, &err);
		expect(&err, 0, "read");
		for (int i = 0; i < 5; ++i) ccl_buffer_destroy(b[i]);
	}
#define WHERE "key type %d count type %d mode %d n %zu bins %zu lower %d shift %u host %d"
#define WHERE_ARGS (int) kt, (int) ct, mode, n, num_bins, lower_mode, shift, host_form
	for (size_t b = 0; b <= num_bins; ++b) {
		uint64_t o = 0;
		memcpy(&o, got_o + b * cs, cs);
		CHECK(o == want_off[b], WHERE ": offsets_out[%zu] = %llu, expected %llu", WHERE_ARGS, b, (unsigned long long) o, (unsigned long long) want_off[b]);
	}
	for (size_t j = 0; j < n; ++j) {
		const size_t i = want_p[j];
		if (keys_out) CHECK(memcmp(got_k + j * ks, hk + i * ks, ks) == 0, WHERE ": wrong key in row %zu", WHERE_ARGS, j);
		if (vals) CHECK(memcmp(got_v + j * vs, hv + i * vs, vs) == 0, WHERE ": wrong value in row %zu", WHERE_ARGS, j);
		else if (vs) CHECK(memcmp(got_v + j * 4, &want_p[j], 4) == 0, WHERE ": wrong index in row %zu", WHERE_ARGS, j);
	}
	for (size_t i = keys_out ? n * ks : 0; i < n * ks + 8; ++i) CHECK(got_k[i] == 0xEE, WHERE ": keys_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = n * vs; i < n * 8 + 8; ++i) CHECK(got_v[i] == 0xEE, WHERE ": values_out written at byte %zu", WHERE_ARGS, i);
	for (size_t i = (num_bins + 1) * cs; i < (num_bins + 1) * cs + 8; ++i) CHECK(got_o[i] == 0xEE, WHERE ": offsets_out written at byte %zu", WHERE_ARGS, i);
	free(hk); free(hv); free(bits); free(want_p); free(want_off); free(at); free(got_k); free(got_v); free(got_o);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_bucket_new(NULL, ctx, CLO_UINT, 2, CLO_UINT, &err), "value_size 2");
	REFUSED_NEW(clo_bucket_new(NULL, ctx, CLO_UINT, 16, CLO_UINT, &err), "value_size 16");
	REFUSED_NEW(clo_bucket_new("drop_rest", ctx, CLO_UINT, 0, CLO_UINT, &err), "options");
	REFUSED_NEW(clo_bucket_new(NULL, ctx, CLO_FLOAT, 0, CLO_UINT, &err), "float keys");
	REFUSED_NEW(clo_bucket_new(NULL, ctx, CLO_HALF, 0, CLO_UINT, &err), "half keys");
	REFUSED_NEW(clo_bucket_new(NULL, ctx, CLO_DOUBLE, 0, CLO_UINT, &err), "double keys");
	REFUSED_NEW(clo_bucket_new(NULL, ctx, (CloType) 11, 0, CLO_UINT, &err), "an unknown key type");
	REFUSED_NEW(clo_bucket_new(NULL, ctx, CLO_UINT, 0, CLO_INT, &err), "count type int");
	REFUSED_NEW(clo_bucket_new(NULL, ctx, CLO_UINT, 0, CLO_LONG, &err), "count type long");
	REFUSED_NEW(clo_bucket_new(NULL, ctx, CLO_UINT, 0, CLO_USHORT, &err), "count type ushort");
	REFUSED_NEW(clo_bucket_new(NULL, NULL, CLO_UINT, 0, CLO_UINT, &err), "no context");
	CHECK(clo_bucket_new(NULL, ctx, CLO_UINT, 3, CLO_UINT, NULL) == NULL, "value_size 3, err NULL");
	CHECK(clo_bucket_new(NULL, ctx, CLO_FLOAT, 4, CLO_UINT, NULL) == NULL, "float keys, err NULL");
	CHECK(clo_bucket_new(NULL, ctx, CLO_UINT, 4, CLO_FLOAT, NULL) == NULL, "count type float, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* ki = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);
	CCLBuffer* vi = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);          /* adjacent to ki */
	CCLBuffer* ko = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* vo = ccl_buffer_new_from_device_ptr(ctx, base + 576, 64, &err);         /* adjacent to ko */
	CCLBuffer* of = ccl_buffer_new_from_device_ptr(ctx, base + 640, 36, &err);         /* 8 bins + 1, adjacent to vo */
	CCLBuffer* ko_on_ki = ccl_buffer_new_from_device_ptr(ctx, base + 60, 64, &err);    /* one shared element with ki */
	CCLBuffer* vo_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 572, 64, &err);   /* starts on ko's last row */
	CCLBuffer* of_in_ko = ccl_buffer_new_from_device_ptr(ctx, base + 544, 36, &err);
	CCLBuffer* of_on_ki = ccl_buffer_new_from_device_ptr(ctx, base + 60, 36, &err);
	CCLBuffer* of_on_vo = ccl_buffer_new_from_device_ptr(ctx, base + 636, 36, &err);   /* its first entry is vo's last row */
	CCLBuffer* of_short = ccl_buffer_new_from_device_ptr(ctx, base + 1024, 32, &err);  /* 8 entries: one short of 8 bins + 1 */
	CCLBuffer* ko_short = ccl_buffer_new_from_device_ptr(ctx, base + 2048, 60, &err);  /* 15 rows */
	expect(&err, 0, "buffers");
	uint32_t h[16] = { 0 }, hv[16] = { 0 }, ho[24], hvo[24], hof[24], lo = 1;
	for (int i = 0; i < 24; ++i) { ho[i] = 0xABCD0000u + (uint32_t) i; hvo[i] = 0x12340000u + (uint32_t) i; hof[i] = 0x77770000u + (uint32_t) i; }
	CloBucket* b0 = clo_bucket_new(NULL, ctx, CLO_UINT, 0, CLO_UINT, &err);
	CloBucket* b4 = clo_bucket_new("", ctx, CLO_UINT, 4, CLO_UINT, &err);
	CloBucket* b8 = clo_bucket_new(NULL, ctx, CLO_UINT, 8, CLO_ULONG, &err);
	CloBucket* c1 = clo_bucket_new(NULL, ctx, CLO_CHAR, 0, CLO_UINT, &err);
	expect(&err, 0, "objects");
	if (!b0 || !b4 || !b8 || !c1) return;
	CHECK(clo_bucket_get_context(b4) == ctx && clo_bucket_get_key_type(b4) == CLO_UINT && clo_bucket_get_key_size(b4) == 4
		&& clo_bucket_get_value_size(b4) == 4 && clo_bucket_get_value_size(b0) == 0 && clo_bucket_get_value_size(b8) == 8
		&& clo_bucket_get_count_type(b4) == CLO_UINT && clo_bucket_get_count_size(b4) == 4 && clo_bucket_get_count_type(b8) == CLO_ULONG
		&& clo_bucket_get_count_size(b8) == 8 && clo_bucket_get_key_size(c1) == 1, "getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of, (size_t) 1 << 32, &lo, 0, 8, &err), "numel 2^32");
	REFUSED_HOST(clo_bucket_with_host_data(b4, cq, NULL, h, hv, ho, hvo, hof, (size_t) 1 << 32, &lo, 0, 8, &err), "numel 2^32, host");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of, 16, &lo, 0, 0, &err), "num_bins 0");
	REFUSED_HOST(clo_bucket_with_host_data(b0, cq, NULL, h, NULL, ho, NULL, hof, 16, NULL, 0, 0, &err), "num_bins 0, host");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of, 16, &lo, 0, 65536, &err), "num_bins 65536");
	REFUSED_HOST(clo_bucket_with_host_data(b0, cq, NULL, h, NULL, ho, NULL, hof, 16, NULL, 0, (size_t) 1 << 40, &err), "num_bins 2^40, host");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of, 16, &lo, 32, 8, &err), "shift 32 of uint keys");
	REFUSED_HOST(clo_bucket_with_host_data(c1, cq, NULL, h, NULL, ho, NULL, hof, 16, NULL, 8, 8, &err), "shift 8 of char keys, host");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, NULL, NULL, ko, NULL, of, 16, &lo, 0, 8, &err), "keys_in NULL");
	REFUSED_HOST(clo_bucket_with_host_data(b4, cq, NULL, NULL, NULL, NULL, hvo, hof, 16, NULL, 0, 8, &err), "keys_in NULL in the arg form, host");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, NULL, 16, &lo, 0, 8, &err), "offsets_out NULL");
	REFUSED_HOST(clo_bucket_with_host_data(b0, cq, NULL, h, NULL, ho, NULL, NULL, 16, NULL, 0, 8, &err), "offsets_out NULL, host");
	REFUSED_HOST(clo_bucket_with_host_data(b0, cq, NULL, NULL, NULL, ho, NULL, NULL, 0, NULL, 0, 8, &err), "offsets_out NULL with numel 0, host");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, vi, ko, NULL, of, 16, &lo, 0, 8, &err), "values with value_size 0");
	REFUSED_HOST(clo_bucket_with_host_data(b0, cq, NULL, h, NULL, ho, hvo, hof, 16, NULL, 0, 8, &err), "values_out with value_size 0, host");
	REFUSED_DEV(clo_bucket_with_device_data(b4, cq, NULL, ki, vi, ko, NULL, of, 16, &lo, 0, 8, &err), "values_out NULL");
	REFUSED_HOST(clo_bucket_with_host_data(b8, cq, NULL, h, NULL, ho, hvo, hof, 8, NULL, 0, 3, &err), "NULL values with value_size 8, host");
	REFUSED_DEV(clo_bucket_with_device_data(b8, cq, NULL, ki, NULL, ko, vo, of, 8, &lo, 0, 3, &err), "NULL values with value_size 8");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, NULL, NULL, of, 16, &lo, 0, 8, &err), "keys_out NULL without values");
	REFUSED_DEV(clo_bucket_with_device_data(b4, cq, NULL, ki, vi, NULL, vo, of, 16, &lo, 0, 8, &err), "keys_out NULL outside the arg form");
	REFUSED_HOST(clo_bucket_with_host_data(b4, cq, NULL, h, hv, NULL, hvo, hof, 16, NULL, 0, 8, &err), "keys_out NULL outside the arg form, host");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ki, NULL, of, 16, &lo, 0, 8, &err), "in place");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko_on_ki, NULL, of, 16, &lo, 0, 8, &err), "keys_out sharing keys_in's last element");
	REFUSED_DEV(clo_bucket_with_device_data(b4, cq, NULL, ki, vi, ko, vo_in_ko, of, 16, &lo, 0, 8, &err), "values_out on keys_out's last row");
	REFUSED_DEV(clo_bucket_with_device_data(b4, cq, NULL, ki, vi, ko, vi, of, 16, &lo, 0, 8, &err), "values_out on values_in");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of_in_ko, 16, &lo, 0, 8, &err), "offsets_out inside keys_out");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of_on_ki, 16, &lo, 0, 8, &err), "offsets_out on keys_in's last element");
	REFUSED_DEV(clo_bucket_with_device_data(b4, cq, NULL, ki, vi, ko, vo, of_on_vo, 16, &lo, 0, 8, &err), "offsets_out on values_out's last row");
	REFUSED_HOST(clo_bucket_with_host_data(b4, cq, NULL, h, hv, ho, ho + 15, hof, 16, NULL, 0, 8, &err), "values_out on keys_out's last row, host");
	REFUSED_HOST(clo_bucket_with_host_data(b0, cq, NULL, ho + 8, NULL, ho, NULL, hof, 16, NULL, 0, 8, &err), "keys_in inside keys_out, host");
	REFUSED_HOST(clo_bucket_with_host_data(b0, cq, NULL, h, NULL, ho, NULL, ho + 15, 16, NULL, 0, 8, &err), "offsets_out on keys_out's last row, host");
	REFUSED_HOST(clo_bucket_with_host_data(b0, cq, NULL, h, NULL, ho, NULL, h + 15, 16, NULL, 0, 8, &err), "offsets_out on keys_in's last row, host");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of, 17, &lo, 0, 8, &err), "numel beyond the buffers");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko_short, NULL, of, 16, &lo, 0, 8, &err), "keys_out below numel rows");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of_short, 16, &lo, 0, 8, &err), "offsets_out below num_bins + 1 entries");
	REFUSED_DEV(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, of, 16, &lo, 0, 9, &err), "num_bins beyond offsets_out");
	/* err == NULL */
	CHECK(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ki, NULL, of, 16, &lo, 0, 8, NULL) == NULL, "in place, err NULL");
	CHECK(clo_bucket_with_device_data(b0, cq, NULL, ki, NULL, ko, NULL, NULL, 16, &lo, 0, 8, NULL) == NULL, "offsets_out NULL, err NULL");
	CHECK(!clo_bucket_with_host_data(b4, NULL, NULL, h, hv, ho, hvo, hof, (size_t) 1 << 32, NULL, 0, 8, NULL), "numel 2^32, host, err NULL");
	CHECK(!clo_bucket_with_host_data(b0, NULL, NULL, h, NULL, ho, NULL, hof, 16, NULL, 0, 0, NULL), "num_bins 0, host, err NULL");
	for (int i = 0; i < 24; ++i)
		CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i && hof[i] == 0x77770000u + (uint32_t) i, "a refused call wrote an output at %d", i);
	/* adjacent, disjoint views of one allocation are accepted */
	CHECK(clo_bucket_with_device_data(b4, cq, NULL, ki, vi, ko, vo, of, 16, &lo, 0, 8, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_bucket_with_device_data(b4, cq, NULL, ki, NULL, NULL, vo, of, 16, NULL, 0, 8, &err) != NULL, "indices alone");
	expect(&err, 0, "indices alone");
	/* numel 0: success, num_bins + 1 zeros, nothing else written, no queue needed in the host form, inputs may be NULL */
	CHECK(clo_bucket_with_host_data(b4, NULL, NULL, NULL, NULL, ho, hvo, hof, 0, NULL, 0, 8, &err), "empty, host");
	expect(&err, 0, "empty, host");
	for (int i = 0; i < 24; ++i) CHECK(hof[i] == (i < 9 ? 0u : 0x77770000u + (uint32_t) i), "empty, host: offsets_out[%d] = %#x", i, hof[i]);
	uint32_t dof[9];
	memset(dof, 0x55, sizeof dof);
	ccl_buffer_enqueue_write(of, cq, CL_TRUE, 0, 36, dof, NULL, &err);
	CHECK(clo_bucket_with_device_data(b4, cq, NULL, NULL, NULL, ko, vo, of, 0, &lo, 0, 8, &err) != NULL, "empty, device");
	expect(&err, 0, "empty, device");
	ccl_buffer_enqueue_read(of, cq, CL_TRUE, 0, 36, dof, NULL, &err);
	expect(&err, 0, "read");
	for (int i = 0; i < 9; ++i) CHECK(dof[i] == 0, "empty, device: offsets_out[%d] = %#x", i, dof[i]);
	for (int i = 0; i < 24; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i && hvo[i] == 0x12340000u + (uint32_t) i, "an empty call wrote a row at %d", i);

	clo_bucket_destroy(b0); clo_bucket_destroy(b4); clo_bucket_destroy(b8); clo_bucket_destroy(c1);
	CCLBuffer* all[] = { ki, vi, ko, vo, of, ko_on_ki, vo_in_ko, of_in_ko, of_on_ki, of_on_vo, of_short, ko_short, big };
	for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) ccl_buffer_destroy(all[i]);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType types[] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG };
	/* large -> small -> large on one object per type, count type and mode, with numel 0 in between */
	static const size_t sizes[] = { 9001, 37, 0, 1, 12000 };
	static const size_t bins[] = { 1, 3, 255, 256, 1000 };
	int turn = 0;
	for (size_t t = 0; t < sizeof(types) / sizeof(types[0]); ++t) {
		for (int c = 0; c < 2; ++c) {
			for (int mode = KEYS_ONLY; mode <= ARG_ONLY; ++mode) {
				const CloType ct = c ? CLO_ULONG : CLO_UINT;
				CloBucket* bkt = clo_bucket_new(NULL, ctx, types[t], mode == KEYS_ONLY ? 0 : mode == VAL8 ? 8 : 4, ct, &err);
				expect(&err, 0, "clo_bucket_new");
				if (!bkt) continue;
				for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z) {
					for (int host_form = 0; host_form < 2; ++host_form) {
						size_t nb = bins[turn % 5];
						const unsigned bits = 8 * (unsigned) clo_type_sizeof(types[t]);
						unsigned shift = (unsigned) (turn % 3);
						if (bits == 8) { shift = 0; if (nb > 100) nb = 50 + (size_t) (turn % 7); }   /* a range the 1-byte types can leave on both sides */
						run_bucket(ctx, cq, bkt, types[t], ct, mode, sizes[z], nb, turn % 3, shift, host_form);
						++turn;
					}
				}
				clo_bucket_destroy(bkt);
			}
		}
	}
	/* shift B - 1 and bin counts the type's range cannot fill */
	for (size_t t = 0; t < sizeof(types) / sizeof(types[0]); ++t) {
		CloBucket* bkt = clo_bucket_new(NULL, ctx, types[t], 4, CLO_UINT, &err);
		expect(&err, 0, "clo_bucket_new");
		if (!bkt) continue;
		run_bucket(ctx, cq, bkt, types[t], CLO_UINT, ARG, 3000, 2, 0, 8 * (unsigned) clo_type_sizeof(types[t]) - 1, 0);
		run_bucket(ctx, cq, bkt, types[t], CLO_UINT, VAL4, 3000, 65535, 2, 0, 1);
		clo_bucket_destroy(bkt);
	}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("bucket host ok\n");
	return failures ? 1 : 0;
}
