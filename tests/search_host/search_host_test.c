/*
 * search_host_test.c — CloSearch (include/clo_search.h) on the CPU, over the host stubs of the thin C-ABI
 * (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan (tests/test_search_cpu.py). Every key type; lower and
 * upper bounds; with and without the sorted-needles promise; an empty haystack, no needles; the device and the host
 * form; one object used large -> small -> large (its workspace grows once and is reused); every refusal the driver
 * makes (err == NULL included), with pos_out left alone; a clean destroy. The expected results are computed here by
 * a linear count over the haystack, not taken from the stub.
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

/* the bits of a key as an unsigned number in the library's order */
static uint64_t order_key(uint64_t bits, size_t ks, int kind) {
	const uint64_t sign = 1ull << (8 * ks - 1), all = ks == 8 ? ~0ull : ((1ull << (8 * ks)) - 1ull);
	bits &= all;
	if (kind == 1) return bits ^ sign;
	if (kind == 2) return (bits & sign) ? bits ^ all : bits ^ sign;
	return bits;
}

typedef struct { uint64_t ord, bits; } elem;

static int by_order(const void* x, const void* y) {
	const elem* a = (const elem*) x; const elem* b = (const elem*) y;
	return a->ord < b->ord ? -1 : a->ord > b->ord;
}

/* n keys drawn from few values (so that ties occur) around the type's sign change */
static void make_keys(elem* e, size_t n, size_t ks, int kind, int sorted) {
	for (size_t i = 0; i < n; ++i) {
		uint64_t bits = (uint64_t) (rnd() % 23) - 11u;   /* -11 .. 11 as two's complement */
		if (kind == 2) bits = (rnd() & 1 ? 1ull << (8 * ks - 1) : 0ull) | (rnd() % 7);   /* +-0 and small denormals */
		e[i].bits = ks == 8 ? bits : bits & ((1ull << (8 * ks)) - 1ull);
		e[i].ord = order_key(bits, ks, kind);
	}
	if (sorted) qsort(e, n, sizeof(elem), by_order);
}

static void run_search(CCLContext* ctx, CCLQueue* cq, CloSearch* s, CloType kt, unsigned flags, size_t nh, size_t nn, int host_form) {
	GError* err = NULL;
	const size_t ks = clo_type_sizeof(kt);
	const int kind = kind_of(kt), upper = (flags & CLO_SEARCH_UPPER) != 0;
	elem* h = (elem*) malloc((nh + 1) * sizeof(elem));
	elem* x = (elem*) malloc((nn + 1) * sizeof(elem));
	make_keys(h, nh, ks, kind, 1);
	make_keys(x, nn, ks, kind, (flags & CLO_SEARCH_NEEDLES_SORTED) != 0);
	unsigned char* hk = (unsigned char*) malloc(nh * ks + 8);
	unsigned char* xk = (unsigned char*) malloc(nn * ks + 8);
	for (size_t i = 0; i < nh; ++i) memcpy(hk + i * ks, &h[i].bits, ks);
	for (size_t i = 0; i < nn; ++i) memcpy(xk + i * ks, &x[i].bits, ks);
	uint32_t* want = (uint32_t*) malloc((nn + 2) * 4);
	for (size_t i = 0; i < nn; ++i) {   /* the definition: a linear count */
		uint32_t c = 0;
		for (size_t j = 0; j < nh; ++j) c += upper ? h[j].ord <= x[i].ord : h[j].ord < x[i].ord;
		want[i] = c;
	}
	unsigned char* got = (unsigned char*) malloc(nn * 4 + 8);
	memset(got, 0xEE, nn * 4 + 8);
	if (host_form) {
		CHECK(clo_search_with_host_data(s, (nn & 1) ? cq : NULL, NULL, nh ? hk : NULL, nh, xk, nn, flags, got, &err), "host data");
		expect(&err, 0, "host data");
	} else {
		CCLBuffer* b[3];   /* haystack, needles, positions */
		const size_t bytes[3] = { nh * ks, nn * ks, nn * 4 };
		for (int i = 0; i < 3; ++i) b[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i] + 8, NULL, &err);
		expect(&err, 0, "buffers");
		ccl_buffer_enqueue_write(b[0], cq, CL_TRUE, 0, bytes[0], hk, NULL, &err);
		ccl_buffer_enqueue_write(b[1], cq, CL_TRUE, 0, bytes[1], xk, NULL, &err);
		ccl_buffer_enqueue_write(b[2], cq, CL_TRUE, 0, bytes[2] + 8, got, NULL, &err);
		expect(&err, 0, "write");
		CCLEvent* evt = clo_search_with_device_data(s, cq, NULL, nh ? b[0] : NULL, nh, b[1], nn, flags, b[2], &err);
		expect(&err, 0, "search");
		CHECK(evt != NULL, "no event");
		ccl_buffer_enqueue_read(b[2], cq, CL_TRUE, 0, bytes[2] + 8, got, NULL, &err);
		expect(&err, 0, "read");
		for (int i = 0; i < 3; ++i) ccl_buffer_destroy(b[i]);
	}
	CHECK(memcmp(got, want, nn * 4) == 0, "key type %d flags %u, %zu needles in %zu keys, host %d: wrong positions", (int) kt, flags, nn, nh, host_form);
	for (size_t i = nn * 4; i < nn * 4 + 8; ++i) CHECK(got[i] == 0xEE, "pos_out written at byte %zu (flags %u, %zu in %zu)", i, flags, nn, nh);
	free(h); free(x); free(hk); free(xk); free(want); free(got);
}

static void test_refusals(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
#define REFUSED_NEW(call, what) do { CHECK((call) == NULL, "%s: an object came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_NEW(clo_search_new("descending", ctx, CLO_UINT, &err), "options");
	REFUSED_NEW(clo_search_new(" ", ctx, CLO_UINT, &err), "options, a blank");
	REFUSED_NEW(clo_search_new(NULL, ctx, (CloType) 11, &err), "an unknown key type");
	CHECK(clo_search_new("x", ctx, CLO_UINT, NULL) == NULL, "options, err NULL");

	CCLBuffer* big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 4096, NULL, &err);
	char* base = (char*) ccl_buffer_get_device_ptr(big);
	CCLBuffer* hay = ccl_buffer_new_from_device_ptr(ctx, base, 64, &err);
	CCLBuffer* ndl = ccl_buffer_new_from_device_ptr(ctx, base + 64, 64, &err);          /* adjacent to hay */
	CCLBuffer* pos = ccl_buffer_new_from_device_ptr(ctx, base + 128, 64, &err);         /* adjacent to ndl */
	CCLBuffer* pos_on_ndl = ccl_buffer_new_from_device_ptr(ctx, base + 124, 64, &err);  /* one shared element with ndl */
	CCLBuffer* pos_in_hay = ccl_buffer_new_from_device_ptr(ctx, base + 16, 64, &err);   /* starts inside hay, ends inside ndl */
	CCLBuffer* pos_small = ccl_buffer_new_from_device_ptr(ctx, base + 512, 32, &err);
	expect(&err, 0, "buffers");
	uint32_t h[48] = { 0 }, g[16] = { 0 }, out[32];
	for (int i = 0; i < 32; ++i) out[i] = 0xABCD0000u + (uint32_t) i;
	CloSearch* s = clo_search_new("", ctx, CLO_UINT, &err);
	expect(&err, 0, "object");
	if (!s) return;
	CHECK(clo_search_get_context(s) == ctx && clo_search_get_key_type(s) == CLO_UINT && clo_search_get_key_size(s) == 4, "getters");

#define REFUSED_DEV(call, what) do { CHECK((call) == NULL, "%s: an event came back", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
#define REFUSED_HOST(call, what) do { CHECK(!(call), "%s: success", what); expect(&err, CLO_ERROR_ARGS, what); } while (0)
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 4u, pos, &err), "flag 4");
	REFUSED_HOST(clo_search_with_host_data(s, cq, NULL, h, 16, g, 16, 0x80000001u, out, &err), "flag 2^31, host");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, (size_t) 1 << 32, ndl, 16, 0, pos, &err), "numel_h 2^32");
	REFUSED_HOST(clo_search_with_host_data(s, cq, NULL, h, 16, g, (size_t) 1 << 32, 0, out, &err), "numel_n 2^32, host");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, NULL, 16, ndl, 16, 0, pos, &err), "haystack NULL");
	REFUSED_HOST(clo_search_with_host_data(s, cq, NULL, NULL, 16, g, 16, 1u, out, &err), "haystack NULL, host");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 16, NULL, 16, 2u, pos, &err), "needles NULL");
	REFUSED_HOST(clo_search_with_host_data(s, cq, NULL, h, 16, NULL, 16, 0, out, &err), "needles NULL, host");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 0, NULL, &err), "pos_out NULL");
	REFUSED_HOST(clo_search_with_host_data(s, cq, NULL, h, 16, g, 16, 3u, NULL, &err), "pos_out NULL, host");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 0, hay, &err), "pos_out on the haystack");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 0, ndl, &err), "pos_out on the needles");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 0, pos_on_ndl, &err), "pos_out sharing the needles' last element");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 0, pos_in_hay, &err), "pos_out across the haystack's end");
	REFUSED_HOST(clo_search_with_host_data(s, cq, NULL, h, 48, g, 16, 0, h + 8, &err), "pos_out inside the haystack, host");
	REFUSED_HOST(clo_search_with_host_data(s, cq, NULL, h, 16, out + 15, 16, 0, out, &err), "pos_out sharing the needles' first element, host");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 17, ndl, 16, 0, pos, &err), "numel_h beyond the buffer");
	REFUSED_DEV(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 0, pos_small, &err), "pos_out too small");
	/* err == NULL */
	CHECK(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 0, ndl, NULL) == NULL, "in place, err NULL");
	CHECK(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 8u, pos, NULL) == NULL, "flag 8, err NULL");
	CHECK(!clo_search_with_host_data(s, NULL, NULL, h, (size_t) 1 << 32, g, 1, 0, out, NULL), "numel_h 2^32, host, err NULL");
	CHECK(!clo_search_with_host_data(s, NULL, NULL, h, 16, g, 16, 0, NULL, NULL), "pos_out NULL, host, err NULL");
	for (int i = 0; i < 32; ++i) CHECK(out[i] == 0xABCD0000u + (uint32_t) i, "a refused call wrote pos_out at %d", i);
	/* adjacent, disjoint views of one allocation are accepted */
	CHECK(clo_search_with_device_data(s, cq, NULL, hay, 16, ndl, 16, 3u, pos, &err) != NULL, "disjoint views of one allocation");
	expect(&err, 0, "disjoint views of one allocation");
	/* no needles: success, nothing written, no queue needed in the host form; the haystack may be anything */
	CHECK(clo_search_with_host_data(s, NULL, NULL, NULL, 0, NULL, 0, 0, out, &err), "no needles, host");
	expect(&err, 0, "no needles, host");
	CHECK(clo_search_with_host_data(s, NULL, NULL, h, 16, NULL, 0, 2u, NULL, &err), "no needles and no pos_out, host");
	expect(&err, 0, "no needles and no pos_out, host");
	CHECK(clo_search_with_device_data(s, cq, NULL, hay, 16, NULL, 0, 1u, pos, &err) != NULL, "no needles, device");
	expect(&err, 0, "no needles, device");
	for (int i = 0; i < 32; ++i) CHECK(out[i] == 0xABCD0000u + (uint32_t) i, "an empty search wrote pos_out at %d", i);
	/* an empty haystack: its pointer is not looked at, even one that would overlap pos_out */
	CHECK(clo_search_with_host_data(s, cq, NULL, out, 0, g, 16, 1u, out, &err), "empty haystack on pos_out, host");
	expect(&err, 0, "empty haystack on pos_out, host");
	for (int i = 0; i < 16; ++i) CHECK(out[i] == 0, "empty haystack: position %d is %u", i, out[i]);

	clo_search_destroy(s);
	ccl_buffer_destroy(hay); ccl_buffer_destroy(ndl); ccl_buffer_destroy(pos); ccl_buffer_destroy(pos_on_ndl);
	ccl_buffer_destroy(pos_in_hay); ccl_buffer_destroy(pos_small); ccl_buffer_destroy(big);
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	static const CloType types[] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };
	/* (haystack, needles): large -> small -> large on one object, an empty haystack, no needles, a last partial tile */
	static const size_t sizes[][2] = { { 1300, 2100 }, { 37, 5 }, { 0, 300 }, { 300, 0 }, { 1, 1 }, { 0, 0 }, { 5, 1025 }, { 4100, 3073 } };
	for (size_t t = 0; t < sizeof(types) / sizeof(types[0]); ++t) {
		CloSearch* s = clo_search_new(NULL, ctx, types[t], &err);
		expect(&err, 0, "clo_search_new");
		if (!s) continue;
		for (size_t z = 0; z < sizeof(sizes) / sizeof(sizes[0]); ++z)
			for (unsigned flags = 0; flags < 4; ++flags)
				for (int host_form = 0; host_form < 2; ++host_form)
					run_search(ctx, cq, s, types[t], flags, sizes[z][0], sizes[z][1], host_form);
		clo_search_destroy(s);
	}
	test_refusals(ctx, cq);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("search host ok\n");
	return failures ? 1 : 0;
}
