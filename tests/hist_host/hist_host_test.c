/*
 * hist_host_test.c — CloHistogram (include/clo_histogram.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_histogram_cpu.py). Every key type, values
 * given and NULL, every value -> sum pair, both modes, lower NULL / negative / at the type's ends, the host-data
 * form, numel 0, several calls of different sizes on one object, and every refusal the driver makes (err == NULL
 * included). The expected histograms are computed here with __int128 differences, not taken from the stub.
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

typedef struct { CloType key, value, sum; } tcase;

static int key_signed(CloType t) { return t == CLO_CHAR || t == CLO_SHORT || t == CLO_INT || t == CLO_LONG; }

/* element i of an array of integers of type t, as an integer */
static __int128 int_at(const unsigned char* p, size_t i, CloType t) {
	const size_t es = clo_type_sizeof(t);
	uint64_t bits = 0;
	memcpy(&bits, p + i * es, es);
	if (!key_signed(t)) return (__int128) bits;
	const int sh = 64 - 8 * (int) es;
	return (__int128) ((int64_t) (bits << sh) >> sh);
}

static void model(const tcase* c, const unsigned char* keys, const unsigned char* values, size_t n, const void* lower,
	unsigned shift, size_t num_bins, unsigned char* hist) {
	const size_t ss = clo_type_sizeof(c->sum);
	const __int128 lo = lower ? int_at((const unsigned char*) lower, 0, c->key) : 0;
	for (size_t i = 0; i < n; ++i) {
		const __int128 d = int_at(keys, i, c->key) - lo;
		if (d < 0 || (d >> shift) >= (__int128) num_bins) continue;
		const size_t b = (size_t) (d >> shift);
		const uint64_t x = values ? (uint64_t) (int64_t) int_at(values, i, c->value) : 1u;
		uint64_t h = 0;
		memcpy(&h, hist + b * ss, ss);
		h += x;
		memcpy(hist + b * ss, &h, ss);
	}
}

typedef struct { int64_t lower; int lower_null; unsigned shift; size_t num_bins; } binning;

static void run_case(CCLContext* ctx, CCLQueue* cq, const tcase* c, int vals, int accumulate, const size_t* sizes, int nsizes, const binning* bn) {
	GError* err = NULL;
	CloHistogram* h = clo_histogram_new(accumulate ? "accumulate" : NULL, ctx, c->key, c->value, c->sum, &err);
	expect(&err, 0, "clo_histogram_new");
	if (!h) return;
	CHECK(clo_histogram_get_key_type(h) == c->key && clo_histogram_get_value_type(h) == c->value
		&& clo_histogram_get_sum_type(h) == c->sum && clo_histogram_get_context(h) == ctx
		&& clo_histogram_get_key_size(h) == clo_type_sizeof(c->key) && clo_histogram_get_value_size(h) == clo_type_sizeof(c->value)
		&& clo_histogram_get_sum_size(h) == clo_type_sizeof(c->sum) && (clo_histogram_get_accumulate(h) != 0) == (accumulate != 0), "getters");
	const size_t ks = clo_type_sizeof(c->key), vs = clo_type_sizeof(c->value), ss = clo_type_sizeof(c->sum);
	const size_t nb = bn->num_bins;
	unsigned char lower[8];
	memcpy(lower, &bn->lower, 8);   /* (little-endian: the low bytes are the value in the key type) */
	const void* lo = bn->lower_null ? NULL : lower;
	for (int z = 0; z < nsizes; ++z) {
		const size_t n = sizes[z];
		unsigned char* keys = (unsigned char*) malloc(n * ks + 8);
		unsigned char* values = (unsigned char*) malloc(n * vs + 8);
		unsigned char* want = (unsigned char*) malloc(nb * ss + 8);
		unsigned char* got = (unsigned char*) malloc(nb * ss + 8);
		for (size_t i = 0; i < n; ++i) {
			/* a third of the keys near the lower bound (both sides), the others anywhere */
			uint64_t k = ((uint64_t) rnd() << 32) | rnd();
			if (rnd() % 3 != 0) k = (uint64_t) bn->lower + (uint64_t) (rnd() % (4 * (nb << bn->shift) + 8)) - (uint64_t) (nb << bn->shift);
			memcpy(keys + i * ks, &k, ks);
			uint64_t v = ((uint64_t) rnd() << 32) | rnd();
			memcpy(values + i * vs, &v, vs);
		}
		for (size_t i = 0; i < nb * ss + 8; ++i) got[i] = (unsigned char) (i * 7 + 3);   /* what hist_out holds before */
		memcpy(want, got, nb * ss + 8);
		if (!accumulate) memset(want, 0, nb * ss);
		model(c, keys, vals ? values : NULL, n, lo, bn->shift, nb, want);

		CCLBuffer* kin = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * ks + 8, NULL, &err);
		CCLBuffer* vin = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * vs + 8, NULL, &err);
		CCLBuffer* out = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, nb * ss + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(kin, cq, CL_TRUE, 0, n * ks + 8, keys, NULL, &err);
		ccl_buffer_enqueue_write(vin, cq, CL_TRUE, 0, n * vs + 8, values, NULL, &err);
		ccl_buffer_enqueue_write(out, cq, CL_TRUE, 0, nb * ss + 8, got, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_histogram_with_device_data(h, cq, NULL, kin, vals ? vin : NULL, out, n, lo, bn->shift, nb, &err);
		expect(&err, 0, "histogram");
		CHECK(evt != NULL, "no event");
		unsigned char* back = (unsigned char*) malloc(nb * ss + 8);
		ccl_buffer_enqueue_read(out, cq, CL_TRUE, 0, nb * ss + 8, back, NULL, &err);
		expect(&err, 0, "read");
		CHECK(memcmp(back, want, nb * ss + 8) == 0, "key %d value %d sum %d vals %d acc %d n %zu bins %zu shift %u: wrong histogram or written past it",
			(int) c->key, (int) c->value, (int) c->sum, vals, accumulate, n, nb, bn->shift);

		/* the host-data form gives the same, from the same starting contents */
		CHECK(clo_histogram_with_host_data(h, (z & 1) ? cq : NULL, NULL, keys, vals ? values : NULL, got, n, lo, bn->shift, nb, &err), "host data");
		expect(&err, 0, "host data");
		CHECK(memcmp(got, want, nb * ss + 8) == 0, "host data, key %d value %d sum %d vals %d acc %d n %zu bins %zu", (int) c->key, (int) c->value,
			(int) c->sum, vals, accumulate, n, nb);

		ccl_buffer_destroy(kin); ccl_buffer_destroy(vin); ccl_buffer_destroy(out);
		free(keys); free(values); free(want); free(got); free(back);
	}
	clo_histogram_destroy(h);
}

static void refuse_new(CCLContext* ctx, const char* options, CloType k, CloType v, CloType s, const char* what) {
	GError* err = NULL;
	CHECK(clo_histogram_new(options, ctx, k, v, s, &err) == NULL, "%s: an object came back", what);
	expect(&err, CLO_ERROR_ARGS, what);
	CHECK(clo_histogram_new(options, ctx, k, v, s, NULL) == NULL, "%s, err NULL: an object came back", what);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	refuse_new(ctx, NULL, CLO_FLOAT, CLO_UINT, CLO_UINT, "float keys");
	refuse_new(ctx, NULL, CLO_DOUBLE, CLO_UINT, CLO_UINT, "double keys");
	refuse_new(ctx, NULL, CLO_HALF, CLO_UINT, CLO_UINT, "half keys");
	refuse_new(ctx, NULL, (CloType) 11, CLO_UINT, CLO_UINT, "an unknown key type");
	refuse_new(ctx, NULL, CLO_UINT, CLO_FLOAT, CLO_FLOAT, "float values");
	refuse_new(ctx, NULL, CLO_UINT, CLO_UINT, CLO_DOUBLE, "double sums");
	refuse_new(ctx, NULL, CLO_UINT, CLO_USHORT, CLO_UINT, "2-byte values");
	refuse_new(ctx, NULL, CLO_UINT, CLO_UINT, CLO_USHORT, "2-byte sums");
	refuse_new(ctx, NULL, CLO_UINT, CLO_ULONG, CLO_UINT, "a sum narrower than the values");
	refuse_new(ctx, "tile=4096", CLO_UINT, CLO_UINT, CLO_UINT, "options");
	refuse_new(ctx, "accumulate,x", CLO_UINT, CLO_UINT, CLO_UINT, "options with a tail");
	CloHistogram* e = clo_histogram_new("", ctx, CLO_CHAR, CLO_INT, CLO_LONG, &err);
	expect(&err, 0, "empty options");
	if (e) { CHECK(!clo_histogram_get_accumulate(e), "empty options accumulate"); clo_histogram_destroy(e); }

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* k = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);
	CCLBuffer* v = ccl_buffer_new_from_device_ptr(ctx, base + 256, 64, &err);
	CCLBuffer* out = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* k_tail = ccl_buffer_new_from_device_ptr(ctx, base + 60, 64, &err);     /* overlaps k's last word */
	CCLBuffer* v_head = ccl_buffer_new_from_device_ptr(ctx, base + 196, 64, &err);    /* ends inside v */
	expect(&err, 0, "buffers");
	uint32_t hk[16] = { 0 }, hv[16] = { 0 }, ho[16];
	for (int i = 0; i < 16; ++i) ho[i] = 0xABCD0000u + (uint32_t) i;
	CloHistogram* h = clo_histogram_new(NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err);
	expect(&err, 0, "object");
	if (!h) return;

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, out, (size_t) 1 << 32, NULL, 0, 16, &err), "numel 2^32");
	REFUSED_HOST(clo_histogram_with_host_data(h, cq, NULL, hk, hv, ho, (size_t) 1 << 32, NULL, 0, 16, &err), "numel 2^32, host");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, out, 16, NULL, 0, 0, &err), "no bins");
	REFUSED_HOST(clo_histogram_with_host_data(h, cq, NULL, hk, hv, ho, 16, NULL, 0, 0, &err), "no bins, host");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, out, 16, NULL, 0, (size_t) 1 << 32, &err), "2^32 bins");
	REFUSED_HOST(clo_histogram_with_host_data(h, cq, NULL, hk, hv, ho, 16, NULL, 0, (size_t) 1 << 32, &err), "2^32 bins, host");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, out, 16, NULL, 32, 16, &err), "shift 32 of uint keys");
	REFUSED_HOST(clo_histogram_with_host_data(h, cq, NULL, hk, hv, ho, 16, NULL, 32, 16, &err), "shift 32 of uint keys, host");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, NULL, v, out, 16, NULL, 0, 16, &err), "keys_in NULL");
	REFUSED_HOST(clo_histogram_with_host_data(h, cq, NULL, NULL, hv, ho, 16, NULL, 0, 16, &err), "keys_in NULL, host");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, NULL, 16, NULL, 0, 16, &err), "hist_out NULL");
	REFUSED_HOST(clo_histogram_with_host_data(h, cq, NULL, hk, hv, NULL, 16, NULL, 0, 16, &err), "hist_out NULL, host");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, k, 16, NULL, 0, 16, &err), "hist_out on the keys");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, v, 16, NULL, 0, 16, &err), "hist_out on the values");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, k_tail, 16, NULL, 0, 16, &err), "hist_out overlapping the end of keys_in");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, v_head, 16, NULL, 0, 16, &err), "hist_out ending inside values_in");
	REFUSED_HOST(clo_histogram_with_host_data(h, cq, NULL, hk, hv, hk, 16, NULL, 0, 16, &err), "hist_out on the keys, host");
	REFUSED_HOST(clo_histogram_with_host_data(h, cq, NULL, hk, hv, hv + 8, 16, NULL, 0, 8, &err), "hist_out inside the values, host");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, out, 17, NULL, 0, 16, &err), "numel beyond the buffers");
	REFUSED_DEV(clo_histogram_with_device_data(h, cq, NULL, k, v, out, 16, NULL, 0, 17, &err), "num_bins beyond the buffer");
	/* err == NULL */
	CHECK(clo_histogram_with_device_data(h, cq, NULL, k, v, k, 16, NULL, 0, 16, NULL) == NULL, "in place, err NULL");
	CHECK(clo_histogram_with_device_data(h, cq, NULL, k, v, out, 16, NULL, 0, 0, NULL) == NULL, "no bins, err NULL");
	CHECK(!clo_histogram_with_host_data(h, NULL, NULL, hk, hv, ho, (size_t) 1 << 32, NULL, 0, 16, NULL), "numel 2^32, host, err NULL");
	CHECK(!clo_histogram_with_host_data(h, NULL, NULL, hk, hv, ho, 16, NULL, 32, 16, NULL), "shift, host, err NULL");
	for (int i = 0; i < 16; ++i) CHECK(ho[i] == 0xABCD0000u + (uint32_t) i, "a refused call wrote hist_out[%d]", i);
	/* disjoint views of one allocation are accepted */
	CHECK(clo_histogram_with_device_data(h, cq, NULL, k, v, out, 16, NULL, 0, 16, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");

	/* numel 0: zeroes hist_out (keys NULL allowed), or leaves it alone under "accumulate"; the host form needs no queue */
	CHECK(clo_histogram_with_host_data(h, NULL, NULL, NULL, NULL, ho, 0, NULL, 0, 16, &err), "numel 0, host");
	expect(&err, 0, "numel 0, host");
	for (int i = 0; i < 16; ++i) CHECK(ho[i] == 0, "numel 0 left hist_out[%d]", i);
	CloHistogram* ha = clo_histogram_new("accumulate", ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err);
	expect(&err, 0, "accumulating object");
	if (ha) {
		for (int i = 0; i < 16; ++i) ho[i] = 5u + (uint32_t) i;
		CHECK(clo_histogram_with_host_data(ha, NULL, NULL, NULL, NULL, ho, 0, NULL, 0, 16, &err), "numel 0, host, accumulate");
		expect(&err, 0, "numel 0, host, accumulate");
		for (int i = 0; i < 16; ++i) CHECK(ho[i] == 5u + (uint32_t) i, "numel 0 under accumulate changed hist_out[%d]", i);
		clo_histogram_destroy(ha);
	}
	CCLEvent* e0 = clo_histogram_with_device_data(h, cq, NULL, NULL, NULL, out, 0, NULL, 0, 16, &err);
	expect(&err, 0, "numel 0, device");
	CHECK(e0 != NULL, "numel 0: no event");
	ccl_buffer_enqueue_read(out, cq, CL_TRUE, 0, 64, ho, NULL, &err);
	expect(&err, 0, "numel 0: read");
	for (int i = 0; i < 16; ++i) CHECK(ho[i] == 0, "numel 0, device, left hist_out[%d]", i);

	clo_histogram_destroy(h);
	ccl_buffer_destroy(k); ccl_buffer_destroy(v); ccl_buffer_destroy(out); ccl_buffer_destroy(k_tail); ccl_buffer_destroy(v_head);
	ccl_buffer_destroy(big);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	/* every key type, every value -> sum pair the library takes */
	static const tcase cases[] = {
		{ CLO_UCHAR, CLO_UINT, CLO_UINT }, { CLO_CHAR, CLO_INT, CLO_INT }, { CLO_USHORT, CLO_UINT, CLO_ULONG }, { CLO_SHORT, CLO_INT, CLO_LONG },
		{ CLO_UINT, CLO_UINT, CLO_UINT }, { CLO_INT, CLO_INT, CLO_ULONG }, { CLO_UINT, CLO_UINT, CLO_INT }, { CLO_INT, CLO_UINT, CLO_LONG },
		{ CLO_ULONG, CLO_ULONG, CLO_ULONG }, { CLO_LONG, CLO_LONG, CLO_LONG }, { CLO_LONG, CLO_LONG, CLO_ULONG }, { CLO_ULONG, CLO_ULONG, CLO_LONG },
	};
	static const size_t sizes[] = { 0, 1, 37, 9000, 300 };
	for (size_t c = 0; c < sizeof(cases) / sizeof(cases[0]); ++c) {
		const CloType kt = cases[c].key;
		const int bits = 8 * (int) clo_type_sizeof(kt);
		const int64_t tmin = key_signed(kt) ? -((int64_t) 1 << (bits - 2)) * 2 : 0;
		const int64_t tmax = key_signed(kt) ? (int64_t) (((uint64_t) 1 << (bits - 1)) - 1) : (bits == 64 ? -1 : (int64_t) (((uint64_t) 1 << bits) - 1));
		const binning bns[] = {
			{ 0, 1, 0, 7 },                                         /* lower NULL */
			{ key_signed(kt) ? -20 : 3, 0, 1, 40 },                 /* a negative lower for signed keys */
			{ tmin, 0, 0, 19 },                                     /* lower at the type's minimum */
			{ (int64_t) ((uint64_t) tmax - 9u), 0, 2, 64 },         /* the wrap trap: lower + (num_bins << shift) past the maximum */
			{ 1, 0, (unsigned) bits - 1u, 3 },                      /* the largest shift */
		};
		for (size_t b = 0; b < sizeof(bns) / sizeof(bns[0]); ++b)
			for (int vals = 0; vals < 2; ++vals)
				for (int acc = 0; acc < 2; ++acc)
					run_case(ctx, cq, &cases[c], vals, acc, sizes, (int) (sizeof(sizes) / sizeof(sizes[0])), &bns[b]);
	}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("hist host ok\n");
	return failures ? 1 : 0;
}
