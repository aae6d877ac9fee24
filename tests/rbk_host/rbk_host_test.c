/*
 * rbk_host_test.c — CloReduceByKey (include/clo_reduce.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_reduce_by_key_cpu.py). Every key size, values
 * given and NULL, each op, keys_out NULL and aggr_out NULL, the host-data form, numel 0 and 1, two calls of different
 * sizes on one object (growing, then smaller), and every refusal the driver makes (err == NULL included). The expected
 * rows are computed here, run by run, not taken from the stub.
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

static int64_t value_at(const unsigned char* values, size_t i, CloType vt) {
	if (!values) return 1;
	if (vt == CLO_INT) { int32_t v; memcpy(&v, values + i * 4, 4); return v; }
	if (vt == CLO_UINT) { uint32_t v; memcpy(&v, values + i * 4, 4); return (int64_t) v; }
	int64_t v;
	memcpy(&v, values + i * 8, 8);
	return v;
}

static int less_in(uint64_t a, uint64_t b, CloType st) {
	switch (st) {
		case CLO_INT: return (int32_t) (uint32_t) a < (int32_t) (uint32_t) b;
		case CLO_UINT: return (uint32_t) a < (uint32_t) b;
		case CLO_LONG: return (int64_t) a < (int64_t) b;
		default: return a < b;
	}
}

/* the rows of (keys, values): keys_out / aggr_out of numel entries; returns m */
static size_t model(const tcase* c, int op, const unsigned char* keys, const unsigned char* values, size_t n,
	unsigned char* keys_out, unsigned char* aggr_out) {
	const size_t ks = clo_type_sizeof(c->key), ss = clo_type_sizeof(c->sum);
	size_t m = 0, b = 0;
	while (b < n) {
		size_t e = b + 1;
		while (e < n && memcmp(keys + e * ks, keys + b * ks, ks) == 0) ++e;
		uint64_t acc = (uint64_t) value_at(values, b, c->value);
		if (ss == 4) acc &= 0xffffffffull;
		for (size_t i = b + 1; i < e; ++i) {
			uint64_t x = (uint64_t) value_at(values, i, c->value);
			if (ss == 4) x &= 0xffffffffull;
			if (op == 0) acc += x;
			else if (op == 1) acc = less_in(x, acc, c->sum) ? x : acc;
			else acc = less_in(acc, x, c->sum) ? x : acc;
		}
		memcpy(keys_out + m * ks, keys + b * ks, ks);
		memcpy(aggr_out + m * ss, &acc, ss);
		++m;
		b = e;
	}
	return m;
}

static const char* const ops[3] = { "sum", "min", "max" };

/* mode bit 0: values given, bit 1: keys_out given, bit 2: aggr_out given; one object, the sizes in turn */
static void run_case(CCLContext* ctx, CCLQueue* cq, const tcase* c, int op, int mode, const size_t* sizes, int nsizes, uint32_t key_range) {
	GError* err = NULL;
	const int vals = mode & 1, kout = (mode & 2) != 0, aout = (mode & 4) != 0;
	CloReduceByKey* r = clo_reduce_by_key_new(ops[op], NULL, ctx, c->key, c->value, c->sum, &err);
	expect(&err, 0, "clo_reduce_by_key_new");
	if (!r) return;
	CHECK(clo_reduce_by_key_get_key_type(r) == c->key && clo_reduce_by_key_get_value_type(r) == c->value
		&& clo_reduce_by_key_get_sum_type(r) == c->sum && clo_reduce_by_key_get_context(r) == ctx
		&& clo_reduce_by_key_get_key_size(r) == clo_type_sizeof(c->key) && clo_reduce_by_key_get_value_size(r) == clo_type_sizeof(c->value)
		&& clo_reduce_by_key_get_sum_size(r) == clo_type_sizeof(c->sum) && !strcmp(clo_reduce_by_key_get_op(r), ops[op]), "getters");
	const size_t ks = clo_type_sizeof(c->key), vs = clo_type_sizeof(c->value), ss = clo_type_sizeof(c->sum);
	for (int z = 0; z < nsizes; ++z) {
		const size_t n = sizes[z];
		unsigned char* keys = (unsigned char*) malloc(n * ks + 8);
		unsigned char* values = (unsigned char*) malloc(n * vs + 8);
		unsigned char* want_k = (unsigned char*) malloc(n * ks + 8);
		unsigned char* want_a = (unsigned char*) malloc(n * ss + 8);
		unsigned char* got_k = (unsigned char*) malloc(n * ks + 8);
		unsigned char* got_a = (unsigned char*) malloc(n * ss + 8);
		uint64_t cur = rnd();
		for (size_t i = 0; i < n; ++i) {   /* runs of random length; key_range 1: one run */
			if (rnd() % 3 == 0) cur = (uint64_t) (rnd() % key_range) * 0x0101010101010101ull;
			memcpy(keys + i * ks, &cur, ks);
			uint64_t v = ((uint64_t) rnd() << 32) | rnd();
			memcpy(values + i * vs, &v, vs);
		}
		const size_t m = model(c, op, keys, vals ? values : NULL, n, want_k, want_a);

		CCLBuffer* kin = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * ks + 8, NULL, &err);
		CCLBuffer* vin = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * vs + 8, NULL, &err);
		CCLBuffer* ko = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * ks + 8, NULL, &err);
		CCLBuffer* ao = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * ss + 8, NULL, &err);
		CCLBuffer* cnt = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 8, NULL, &err);
		expect(&err, 0, "buffers");
		memset(got_k, 0xCD, n * ks + 8);
		memset(got_a, 0xCD, n * ss + 8);
		ccl_buffer_enqueue_write(kin, cq, CL_TRUE, 0, n * ks + 8, keys, NULL, &err);
		ccl_buffer_enqueue_write(vin, cq, CL_TRUE, 0, n * vs + 8, values, NULL, &err);
		ccl_buffer_enqueue_write(ko, cq, CL_TRUE, 0, n * ks + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_write(ao, cq, CL_TRUE, 0, n * ss + 8, got_a, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_reduce_by_key_with_device_data(r, cq, NULL, kin, vals ? vin : NULL, kout ? ko : NULL, aout ? ao : NULL, cnt, n, &err);
		expect(&err, 0, "reduce by key");
		CHECK(evt != NULL, "no event");
		cl_ulong got_m = ~(cl_ulong) 0;
		ccl_buffer_enqueue_read(cnt, cq, CL_TRUE, 0, 8, &got_m, NULL, &err);
		ccl_buffer_enqueue_read(ko, cq, CL_TRUE, 0, n * ks + 8, got_k, NULL, &err);
		ccl_buffer_enqueue_read(ao, cq, CL_TRUE, 0, n * ss + 8, got_a, NULL, &err);
		expect(&err, 0, "read");
		CHECK(got_m == m, "key %d value %d sum %d op %s mode %d n %zu: %llu runs, expected %zu", (int) c->key, (int) c->value, (int) c->sum,
			ops[op], mode, n, (unsigned long long) got_m, m);
		int bad = 0;
		if (kout && memcmp(got_k, want_k, m * ks) != 0) bad = 1;
		if (aout && memcmp(got_a, want_a, m * ss) != 0) bad = 1;
		/* rows from m on, and an output that was not asked for, keep what was there */
		for (size_t i = kout ? m * ks : 0; i < n * ks + 8; ++i) if (got_k[i] != 0xCD) bad = 2;
		for (size_t i = aout ? m * ss : 0; i < n * ss + 8; ++i) if (got_a[i] != 0xCD) bad = 2;
		CHECK(!bad, "key %d value %d sum %d op %s mode %d n %zu: %s", (int) c->key, (int) c->value, (int) c->sum, ops[op], mode, n,
			bad == 1 ? "wrong rows" : "written past the rows");

		/* the host-data form gives the same, and copies out the m rows only */
		memset(got_k, 0xCD, n * ks + 8);
		memset(got_a, 0xCD, n * ss + 8);
		size_t hm = 12345;
		CHECK(clo_reduce_by_key_with_host_data(r, (z & 1) ? cq : NULL, NULL, keys, vals ? values : NULL, kout ? got_k : NULL, aout ? got_a : NULL, &hm, n, &err),
			"host data");
		expect(&err, 0, "host data");
		CHECK(hm == m, "host data: %zu runs, expected %zu", hm, m);
		bad = 0;
		if (kout && memcmp(got_k, want_k, m * ks) != 0) bad = 1;
		if (aout && memcmp(got_a, want_a, m * ss) != 0) bad = 1;
		for (size_t i = kout ? m * ks : 0; i < n * ks + 8; ++i) if (got_k[i] != 0xCD) bad = 2;
		for (size_t i = aout ? m * ss : 0; i < n * ss + 8; ++i) if (got_a[i] != 0xCD) bad = 2;
		CHECK(!bad, "host data, key %d value %d sum %d op %s mode %d n %zu: %s", (int) c->key, (int) c->value, (int) c->sum, ops[op], mode, n,
			bad == 1 ? "wrong rows" : "written past the rows");

		ccl_buffer_destroy(kin); ccl_buffer_destroy(vin); ccl_buffer_destroy(ko); ccl_buffer_destroy(ao); ccl_buffer_destroy(cnt);
		free(keys); free(values); free(want_k); free(want_a); free(got_k); free(got_a);
	}
	clo_reduce_by_key_destroy(r);
}

static void refuse_new(CCLContext* ctx, const char* op, const char* options, CloType k, CloType v, CloType s, const char* what) {
	GError* err = NULL;
	CHECK(clo_reduce_by_key_new(op, options, ctx, k, v, s, &err) == NULL, "%s: an object came back", what);
	expect(&err, CLO_ERROR_ARGS, what);
	CHECK(clo_reduce_by_key_new(op, options, ctx, k, v, s, NULL) == NULL, "%s, err NULL: an object came back", what);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	refuse_new(ctx, "sum", NULL, CLO_UINT, CLO_FLOAT, CLO_FLOAT, "float values");
	refuse_new(ctx, "sum", NULL, CLO_UINT, CLO_UINT, CLO_DOUBLE, "double sums");
	refuse_new(ctx, "sum", NULL, CLO_UINT, CLO_HALF, CLO_UINT, "half values");
	refuse_new(ctx, "sum", NULL, CLO_UINT, CLO_USHORT, CLO_UINT, "2-byte values");
	refuse_new(ctx, "sum", NULL, CLO_UINT, CLO_CHAR, CLO_LONG, "1-byte values");
	refuse_new(ctx, "sum", NULL, CLO_UINT, CLO_UINT, CLO_USHORT, "2-byte sums");
	refuse_new(ctx, "sum", NULL, CLO_UINT, CLO_ULONG, CLO_UINT, "a sum narrower than the values");
	refuse_new(ctx, "mean", NULL, CLO_UINT, CLO_UINT, CLO_UINT, "an unknown op");
	refuse_new(ctx, NULL, NULL, CLO_UINT, CLO_UINT, CLO_UINT, "op NULL");
	refuse_new(ctx, "sum", "tile=4096", CLO_UINT, CLO_UINT, CLO_UINT, "options");
	refuse_new(ctx, "sum", NULL, (CloType) 11, CLO_UINT, CLO_UINT, "an unknown key type");
	CloReduceByKey* e = clo_reduce_by_key_new("sum", "", ctx, CLO_HALF, CLO_INT, CLO_LONG, &err);   /* empty options, any key type */
	expect(&err, 0, "empty options");
	if (e) clo_reduce_by_key_destroy(e);

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	CCLBuffer* k = ccl_buffer_new_from_device_ptr(ctx, ccl_buffer_get_device_ptr(big), 64, &err);
	CCLBuffer* v = ccl_buffer_new_from_device_ptr(ctx, (char*) ccl_buffer_get_device_ptr(big) + 256, 64, &err);
	CCLBuffer* ko = ccl_buffer_new_from_device_ptr(ctx, (char*) ccl_buffer_get_device_ptr(big) + 512, 64, &err);
	CCLBuffer* ao = ccl_buffer_new_from_device_ptr(ctx, (char*) ccl_buffer_get_device_ptr(big) + 768, 64, &err);
	CCLBuffer* cnt = ccl_buffer_new_from_device_ptr(ctx, (char*) ccl_buffer_get_device_ptr(big) + 1024, 8, &err);
	CCLBuffer* cnt4 = ccl_buffer_new_from_device_ptr(ctx, (char*) ccl_buffer_get_device_ptr(big) + 1028, 8, &err);
	CCLBuffer* k_tail = ccl_buffer_new_from_device_ptr(ctx, (char*) ccl_buffer_get_device_ptr(big) + 60, 64, &err);   /* overlaps k's last word */
	CCLBuffer* v_head = ccl_buffer_new_from_device_ptr(ctx, (char*) ccl_buffer_get_device_ptr(big) + 196, 64, &err);   /* ends inside v */
	expect(&err, 0, "buffers");
	uint32_t hk[16] = { 0 }, hv[16] = { 0 }, hko[16], hao[16];
	size_t hm = 0;
	CloReduceByKey* r = clo_reduce_by_key_new("sum", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err);
	CloReduceByKey* rmin = clo_reduce_by_key_new("min", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err);
	expect(&err, 0, "objects");
	if (!r || !rmin) return;

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, ao, cnt, (size_t) 1 << 32, &err), "numel 2^32");
	REFUSED_HOST(clo_reduce_by_key_with_host_data(r, cq, NULL, hk, hv, hko, hao, &hm, (size_t) 1 << 32, &err), "numel 2^32, host");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, NULL, NULL, cnt, 16, &err), "both outputs NULL");
	REFUSED_HOST(clo_reduce_by_key_with_host_data(r, cq, NULL, hk, hv, NULL, NULL, &hm, 16, &err), "both outputs NULL, host");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, ao, NULL, 16, &err), "no run count");
	REFUSED_HOST(clo_reduce_by_key_with_host_data(r, cq, NULL, hk, hv, hko, hao, NULL, 16, &err), "no run count, host");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, ao, cnt4, 16, &err), "a misaligned run count");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, NULL, v, ko, ao, cnt, 16, &err), "keys_in NULL");
	REFUSED_HOST(clo_reduce_by_key_with_host_data(r, cq, NULL, NULL, hv, hko, hao, &hm, 16, &err), "keys_in NULL, host");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(rmin, cq, NULL, k, NULL, ko, ao, cnt, 16, &err), "min without values");
	REFUSED_HOST(clo_reduce_by_key_with_host_data(rmin, cq, NULL, hk, NULL, hko, hao, &hm, 16, &err), "min without values, host");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, k, ao, cnt, 16, &err), "keys in place");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, v, cnt, 16, &err), "aggregates over the values");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, v, ao, cnt, 16, &err), "keys_out over the values");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, k_tail, ao, cnt, 16, &err), "keys_out overlapping the end of keys_in");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, v_head, cnt, 16, &err), "aggr_out ending inside values_in");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, ao, k, 16, &err), "the run count inside keys_in");
	REFUSED_HOST(clo_reduce_by_key_with_host_data(r, cq, NULL, hk, hv, hk, hao, &hm, 16, &err), "keys in place, host");
	REFUSED_HOST(clo_reduce_by_key_with_host_data(r, cq, NULL, hk, hv, hko, hv + 8, &hm, 16, &err), "aggregates inside the values, host");
	REFUSED_DEV(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, ao, cnt, 17, &err), "numel beyond the buffers");
	/* err == NULL */
	CHECK(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, k, ao, cnt, 16, NULL) == NULL, "in place, err NULL");
	CHECK(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, NULL, NULL, cnt, 16, NULL) == NULL, "both outputs NULL, err NULL");
	CHECK(!clo_reduce_by_key_with_host_data(r, NULL, NULL, hk, hv, hko, hao, &hm, (size_t) 1 << 32, NULL), "numel 2^32, host, err NULL");
	CHECK(!clo_reduce_by_key_with_host_data(rmin, NULL, NULL, hk, NULL, hko, hao, &hm, 16, NULL), "min without values, host, err NULL");
	/* a partial overlap that is none: a non-overlapping neighbour is accepted, and keys_out alone with "min" and no values too */
	CHECK(clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, ao, cnt, 16, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_reduce_by_key_with_device_data(rmin, cq, NULL, k, NULL, ko, NULL, cnt, 16, &err) != NULL, "unique on a min object");
	expect(&err, 0, "unique on a min object");

	/* numel 0: an event, a count of 0, nothing else written */
	cl_ulong m = 99;
	ccl_buffer_enqueue_write(cnt, cq, CL_TRUE, 0, 8, &m, NULL, &err);
	CCLEvent* e0 = clo_reduce_by_key_with_device_data(r, cq, NULL, k, v, ko, ao, cnt, 0, &err);
	expect(&err, 0, "numel 0");
	CHECK(e0 != NULL, "numel 0: no event");
	ccl_buffer_enqueue_read(cnt, cq, CL_TRUE, 0, 8, &m, NULL, &err);
	expect(&err, 0, "numel 0: read");
	CHECK(m == 0, "numel 0: %llu runs", (unsigned long long) m);
	hm = 99;
	CHECK(clo_reduce_by_key_with_host_data(r, NULL, NULL, NULL, NULL, hko, hao, &hm, 0, &err) && hm == 0, "numel 0, host");
	expect(&err, 0, "numel 0, host");

	clo_reduce_by_key_destroy(r);
	clo_reduce_by_key_destroy(rmin);
	ccl_buffer_destroy(k); ccl_buffer_destroy(v); ccl_buffer_destroy(ko); ccl_buffer_destroy(ao); ccl_buffer_destroy(cnt);
	ccl_buffer_destroy(cnt4); ccl_buffer_destroy(k_tail); ccl_buffer_destroy(v_head);
	ccl_buffer_destroy(big);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	/* every key size, every value -> sum pair the library takes */
	static const tcase cases[] = {
		{ CLO_UCHAR, CLO_UINT, CLO_UINT }, { CLO_CHAR, CLO_INT, CLO_INT }, { CLO_USHORT, CLO_UINT, CLO_ULONG }, { CLO_HALF, CLO_INT, CLO_LONG },
		{ CLO_UINT, CLO_UINT, CLO_UINT }, { CLO_INT, CLO_INT, CLO_ULONG }, { CLO_FLOAT, CLO_UINT, CLO_INT }, { CLO_FLOAT, CLO_UINT, CLO_LONG },
		{ CLO_ULONG, CLO_ULONG, CLO_ULONG }, { CLO_LONG, CLO_LONG, CLO_LONG }, { CLO_DOUBLE, CLO_LONG, CLO_ULONG }, { CLO_DOUBLE, CLO_ULONG, CLO_LONG },
	};
	static const size_t sizes[] = { 0, 1, 2, 37, 9000, 300 };   /* one object: growing, then smaller */
	for (size_t c = 0; c < sizeof(cases) / sizeof(cases[0]); ++c)
		for (int op = 0; op < 3; ++op)
			for (int mode = 2; mode < 8; ++mode) {
				if (op != 0 && (mode & 4) && !(mode & 1)) continue;   /* min / max without values: refused (test_refusals) */
				run_case(ctx, cq, &cases[c], op, mode, sizes, (int) (sizeof(sizes) / sizeof(sizes[0])), (c + (size_t) mode) % 3 == 0 ? 1u : 5u);
			}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("rbk host ok\n");
	return failures ? 1 : 0;
}
