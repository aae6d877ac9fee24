/*
 * sbk_host_test.c — CloScanByKey (include/clo_scan_by_key.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_scan_by_key_cpu.py). Every key size, values
 * given and NULL, each op, both kinds, the host-data form, in place (device and host form), numel 0 and 1, several
 * calls of different sizes on one object (growing, then smaller), the option strings, and every refusal the driver
 * makes (err == NULL included). The expected results are computed here, run by run, not taken from the stub.
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

static uint64_t identity_of(int op, CloType st) {
	if (op == 0) return 0;
	switch (st) {
		case CLO_INT: return op == 1 ? (uint64_t) INT32_MAX : (uint64_t) (uint32_t) INT32_MIN;
		case CLO_UINT: return op == 1 ? (uint64_t) UINT32_MAX : 0;
		case CLO_LONG: return op == 1 ? (uint64_t) INT64_MAX : (uint64_t) INT64_MIN;
		default: return op == 1 ? UINT64_MAX : 0;
	}
}

/* the results of (keys, values), run by run: `want` of n entries of the sum type */
static void model(const tcase* c, int op, int inclusive, const unsigned char* keys, const unsigned char* values, size_t n, unsigned char* want) {
	const size_t ks = clo_type_sizeof(c->key), ss = clo_type_sizeof(c->sum);
	const uint64_t id = identity_of(op, c->sum);
	size_t b = 0;
	while (b < n) {
		size_t e = b + 1;
		while (e < n && memcmp(keys + e * ks, keys + b * ks, ks) == 0) ++e;
		uint64_t acc = id;
		for (size_t i = b; i < e; ++i) {
			uint64_t x = (uint64_t) value_at(values, i, c->value);
			if (ss == 4) x &= 0xffffffffull;
			if (!inclusive) memcpy(want + i * ss, &acc, ss);
			if (i == b) acc = x;
			else if (op == 0) acc += x;
			else if (op == 1) acc = less_in(x, acc, c->sum) ? x : acc;
			else acc = less_in(acc, x, c->sum) ? x : acc;
			if (ss == 4) acc &= 0xffffffffull;
			if (inclusive) memcpy(want + i * ss, &acc, ss);
		}
		b = e;
	}
}

static const char* const ops[3] = { "sum", "min", "max" };

/* one object, the sizes in turn; vals: values given; the device form, the host form, and where the widths allow it
 * both of them in place */
static void run_case(CCLContext* ctx, CCLQueue* cq, const tcase* c, int op, int inclusive, int vals, const size_t* sizes, int nsizes, uint32_t key_range) {
	GError* err = NULL;
	CloScanByKey* r = clo_scan_by_key_new(ops[op], inclusive ? "inclusive=1" : vals ? NULL : "inclusive=0", ctx, c->key, c->value, c->sum, &err);
	expect(&err, 0, "clo_scan_by_key_new");
	if (!r) return;
	CHECK(clo_scan_by_key_get_key_type(r) == c->key && clo_scan_by_key_get_value_type(r) == c->value
		&& clo_scan_by_key_get_sum_type(r) == c->sum && clo_scan_by_key_get_context(r) == ctx
		&& clo_scan_by_key_get_key_size(r) == clo_type_sizeof(c->key) && clo_scan_by_key_get_value_size(r) == clo_type_sizeof(c->value)
		&& clo_scan_by_key_get_sum_size(r) == clo_type_sizeof(c->sum) && !strcmp(clo_scan_by_key_get_op(r), ops[op])
		&& clo_scan_by_key_get_inclusive(r) == (inclusive ? CL_TRUE : CL_FALSE), "getters");
	const size_t ks = clo_type_sizeof(c->key), vs = clo_type_sizeof(c->value), ss = clo_type_sizeof(c->sum);
	for (int z = 0; z < nsizes; ++z) {
		const size_t n = sizes[z];
		unsigned char* keys = (unsigned char*) malloc(n * ks + 8);
		unsigned char* values = (unsigned char*) malloc(n * vs + 8);
		unsigned char* want = (unsigned char*) malloc(n * ss + 8);
		unsigned char* got = (unsigned char*) malloc(n * ss + 8);
		uint64_t cur = rnd();
		for (size_t i = 0; i < n; ++i) {   /* runs of random length; key_range 1: one run */
			if (rnd() % 3 == 0) cur = (uint64_t) (rnd() % key_range) * 0x0101010101010101ull;
			memcpy(keys + i * ks, &cur, ks);
			uint64_t v = ((uint64_t) rnd() << 32) | rnd();
			memcpy(values + i * vs, &v, vs);
		}
		memset(values + n * vs, 0xEE, 8);
		model(c, op, inclusive, keys, vals ? values : NULL, n, want);

		CCLBuffer* kin = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * ks + 8, NULL, &err);
		CCLBuffer* vin = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * vs + 8, NULL, &err);
		CCLBuffer* out = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, n * ss + 8, NULL, &err);
		expect(&err, 0, "buffers");
		memset(got, 0xCD, n * ss + 8);
		ccl_buffer_enqueue_write(kin, cq, CL_TRUE, 0, n * ks + 8, keys, NULL, &err);
		ccl_buffer_enqueue_write(vin, cq, CL_TRUE, 0, n * vs + 8, values, NULL, &err);
		ccl_buffer_enqueue_write(out, cq, CL_TRUE, 0, n * ss + 8, got, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_scan_by_key_with_device_data(r, cq, NULL, kin, vals ? vin : NULL, out, n, &err);
		expect(&err, 0, "scan by key");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(out, cq, CL_TRUE, 0, n * ss + 8, got, NULL, &err);
		expect(&err, 0, "read");
		int bad = memcmp(got, want, n * ss) != 0;
		for (size_t i = n * ss; i < n * ss + 8; ++i) if (got[i] != 0xCD) bad = 2;   /* nothing past the end */
		CHECK(!bad, "key %d value %d sum %d op %s incl %d vals %d n %zu: %s", (int) c->key, (int) c->value, (int) c->sum, ops[op], inclusive, vals, n,
			bad == 1 ? "wrong results" : "written past the end");

		/* the host-data form gives the same */
		memset(got, 0xCD, n * ss + 8);
		CHECK(clo_scan_by_key_with_host_data(r, (z & 1) ? cq : NULL, NULL, keys, vals ? values : NULL, got, n, &err), "host data");
		expect(&err, 0, "host data");
		bad = memcmp(got, want, n * ss) != 0;
		for (size_t i = n * ss; i < n * ss + 8; ++i) if (got[i] != 0xCD) bad = 2;
		CHECK(!bad, "host data, key %d value %d sum %d op %s incl %d vals %d n %zu: %s", (int) c->key, (int) c->value, (int) c->sum, ops[op], inclusive,
			vals, n, bad == 1 ? "wrong results" : "written past the end");

		/* in place: out == values_in, device form on the buffer that holds the values, then the host form */
		if (vals && vs == ss) {
			evt = clo_scan_by_key_with_device_data(r, cq, NULL, kin, vin, vin, n, &err);
			expect(&err, 0, "in place");
			CHECK(evt != NULL, "in place: no event");
			memset(got, 0, n * ss + 8);
			ccl_buffer_enqueue_read(vin, cq, CL_TRUE, 0, n * ss + 8, got, NULL, &err);
			expect(&err, 0, "in place: read");
			bad = memcmp(got, want, n * ss) != 0;
			for (size_t i = n * ss; i < n * ss + 8; ++i) if (got[i] != 0xEE) bad = 2;
			CHECK(!bad, "in place, key %d value %d sum %d op %s incl %d n %zu: %s", (int) c->key, (int) c->value, (int) c->sum, ops[op], inclusive, n,
				bad == 1 ? "wrong results" : "written past the end");
			CHECK(clo_scan_by_key_with_host_data(r, cq, NULL, keys, values, values, n, &err), "host data in place");
			expect(&err, 0, "host data in place");
			bad = memcmp(values, want, n * ss) != 0;
			for (size_t i = n * ss; i < n * ss + 8; ++i) if (values[i] != 0xEE) bad = 2;
			CHECK(!bad, "host data in place, key %d value %d sum %d op %s incl %d n %zu: %s", (int) c->key, (int) c->value, (int) c->sum, ops[op],
				inclusive, n, bad == 1 ? "wrong results" : "written past the end");
		}

		ccl_buffer_destroy(kin); ccl_buffer_destroy(vin); ccl_buffer_destroy(out);
		free(keys); free(values); free(want); free(got);
	}
	clo_scan_by_key_destroy(r);
}

static void refuse_new(CCLContext* ctx, const char* op, const char* options, CloType k, CloType v, CloType s, const char* what) {
	GError* err = NULL;
	CHECK(clo_scan_by_key_new(op, options, ctx, k, v, s, &err) == NULL, "%s: an object came back", what);
	expect(&err, CLO_ERROR_ARGS, what);
	CHECK(clo_scan_by_key_new(op, options, ctx, k, v, s, NULL) == NULL, "%s, err NULL: an object came back", what);
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
	refuse_new(ctx, "sum", "tile=4096", CLO_UINT, CLO_UINT, CLO_UINT, "an unknown option");
	refuse_new(ctx, "sum", "inclusive=2", CLO_UINT, CLO_UINT, CLO_UINT, "inclusive=2");
	refuse_new(ctx, "sum", "inclusive", CLO_UINT, CLO_UINT, CLO_UINT, "inclusive without a value");
	refuse_new(ctx, "sum", "inclusive=", CLO_UINT, CLO_UINT, CLO_UINT, "inclusive with an empty value");
	refuse_new(ctx, "sum", "inclusive=1,tile=1", CLO_UINT, CLO_UINT, CLO_UINT, "a second, unknown option");
	refuse_new(ctx, "sum", NULL, (CloType) 11, CLO_UINT, CLO_UINT, "an unknown key type");
	CloScanByKey* e = clo_scan_by_key_new("sum", "", ctx, CLO_HALF, CLO_INT, CLO_LONG, &err);   /* empty options, any key type */
	expect(&err, 0, "empty options");
	if (e) { CHECK(!clo_scan_by_key_get_inclusive(e), "empty options: inclusive"); clo_scan_by_key_destroy(e); }

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* k = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);
	CCLBuffer* v = ccl_buffer_new_from_device_ptr(ctx, base + 256, 64, &err);
	CCLBuffer* o = ccl_buffer_new_from_device_ptr(ctx, base + 512, 64, &err);
	CCLBuffer* o8 = ccl_buffer_new_from_device_ptr(ctx, base + 1024, 128, &err);
	CCLBuffer* v8 = ccl_buffer_new_from_device_ptr(ctx, base + 256, 128, &err);      /* at the values' address, twice their size */
	CCLBuffer* k_tail = ccl_buffer_new_from_device_ptr(ctx, base + 60, 64, &err);    /* overlaps k's last word */
	CCLBuffer* v_plus1 = ccl_buffer_new_from_device_ptr(ctx, base + 260, 64, &err);  /* the values shifted by one element */
	CCLBuffer* v_minus1 = ccl_buffer_new_from_device_ptr(ctx, base + 252, 64, &err);
	expect(&err, 0, "buffers");
	uint32_t hk[16] = { 0 }, hv[17] = { 0 }, ho[16];
	uint64_t ho8[16];
	CloScanByKey* r = clo_scan_by_key_new("sum", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err);
	CloScanByKey* rw = clo_scan_by_key_new("sum", NULL, ctx, CLO_UINT, CLO_UINT, CLO_ULONG, &err);
	CloScanByKey* rmin = clo_scan_by_key_new("min", NULL, ctx, CLO_UINT, CLO_UINT, CLO_UINT, &err);
	expect(&err, 0, "objects");
	if (!r || !rw || !rmin) return;

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, o, (size_t) 1 << 32, &err), "numel 2^32");
	REFUSED_HOST(clo_scan_by_key_with_host_data(r, cq, NULL, hk, hv, ho, (size_t) 1 << 32, &err), "numel 2^32, host");
	REFUSED_DEV(clo_scan_by_key_with_device_data(r, cq, NULL, NULL, v, o, 16, &err), "keys_in NULL");
	REFUSED_HOST(clo_scan_by_key_with_host_data(r, cq, NULL, NULL, hv, ho, 16, &err), "keys_in NULL, host");
	REFUSED_DEV(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, NULL, 16, &err), "data_out NULL");
	REFUSED_HOST(clo_scan_by_key_with_host_data(r, cq, NULL, hk, hv, NULL, 16, &err), "data_out NULL, host");
	REFUSED_DEV(clo_scan_by_key_with_device_data(rmin, cq, NULL, k, NULL, o, 16, &err), "min without values");
	REFUSED_HOST(clo_scan_by_key_with_host_data(rmin, cq, NULL, hk, NULL, ho, 16, &err), "min without values, host");
	REFUSED_DEV(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, k, 16, &err), "out on the keys");
	REFUSED_DEV(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, k_tail, 16, &err), "out overlapping the end of keys_in");
	REFUSED_DEV(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, v_plus1, 16, &err), "out one element above values_in");
	REFUSED_DEV(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, v_minus1, 16, &err), "out one element below values_in");
	REFUSED_DEV(clo_scan_by_key_with_device_data(rw, cq, NULL, k, v, v8, 16, &err), "out on values_in with a wider sum type");
	REFUSED_HOST(clo_scan_by_key_with_host_data(r, cq, NULL, hk, hv, hk, 16, &err), "out on the keys, host");
	REFUSED_HOST(clo_scan_by_key_with_host_data(r, cq, NULL, hk, hv, hv + 1, 16, &err), "out one element above values_in, host");
	REFUSED_HOST(clo_scan_by_key_with_host_data(rw, cq, NULL, hk, hv, (void*) hv, 8, &err), "out on values_in with a wider sum type, host");
	REFUSED_DEV(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, o, 17, &err), "numel beyond the buffers");
	/* err == NULL */
	CHECK(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, k, 16, NULL) == NULL, "out on the keys, err NULL");
	CHECK(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, v_plus1, 16, NULL) == NULL, "shifted, err NULL");
	CHECK(!clo_scan_by_key_with_host_data(r, NULL, NULL, hk, hv, ho, (size_t) 1 << 32, NULL), "numel 2^32, host, err NULL");
	CHECK(!clo_scan_by_key_with_host_data(rmin, NULL, NULL, hk, NULL, ho, 16, NULL), "min without values, host, err NULL");
	/* accepted: disjoint views of one allocation, exactly in place, a wider sum beside the values */
	CHECK(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, o, 16, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	CHECK(clo_scan_by_key_with_device_data(r, cq, NULL, k, v, v, 16, &err) != NULL, "in place");
	expect(&err, 0, "in place");
	CHECK(clo_scan_by_key_with_device_data(rw, cq, NULL, k, v, o8, 16, &err) != NULL, "a wider sum");
	expect(&err, 0, "a wider sum");
	CHECK(clo_scan_by_key_with_host_data(rw, cq, NULL, hk, hv, ho8, 16, &err), "a wider sum, host");
	expect(&err, 0, "a wider sum, host");

	/* numel 0: an event, nothing written, no pointer needed */
	uint32_t mark = 0xCDCDCDCDu, back = 0;
	ccl_buffer_enqueue_write(o, cq, CL_TRUE, 0, 4, &mark, NULL, &err);
	CCLEvent* e0 = clo_scan_by_key_with_device_data(r, cq, NULL, k, v, o, 0, &err);
	expect(&err, 0, "numel 0");
	CHECK(e0 != NULL, "numel 0: no event");
	ccl_buffer_enqueue_read(o, cq, CL_TRUE, 0, 4, &back, NULL, &err);
	expect(&err, 0, "numel 0: read");
	CHECK(back == mark, "numel 0: something was written");
	CHECK(clo_scan_by_key_with_device_data(r, cq, NULL, NULL, NULL, NULL, 0, &err) != NULL, "numel 0 without buffers");
	expect(&err, 0, "numel 0 without buffers");
	CHECK(clo_scan_by_key_with_host_data(r, NULL, NULL, NULL, NULL, NULL, 0, &err), "numel 0, host");
	expect(&err, 0, "numel 0, host");

	clo_scan_by_key_destroy(r);
	clo_scan_by_key_destroy(rw);
	clo_scan_by_key_destroy(rmin);
	ccl_buffer_destroy(k); ccl_buffer_destroy(v); ccl_buffer_destroy(o); ccl_buffer_destroy(o8); ccl_buffer_destroy(v8);
	ccl_buffer_destroy(k_tail); ccl_buffer_destroy(v_plus1); ccl_buffer_destroy(v_minus1);
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
			for (int inclusive = 0; inclusive < 2; ++inclusive)
				for (int vals = 0; vals < 2; ++vals) {
					if (op != 0 && !vals) continue;   /* min / max without values: refused (test_refusals) */
					run_case(ctx, cq, &cases[c], op, inclusive, vals, sizes, (int) (sizeof(sizes) / sizeof(sizes[0])),
						(c + (size_t) op + (size_t) vals) % 3 == 0 ? 1u : 5u);
				}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("sbk host ok\n");
	return failures ? 1 : 0;
}
