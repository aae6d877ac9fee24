/*
 * op_host_test.c — the host layer the operation drivers share (cl_ops_amd/csrc/clo_internal.h, clo_op_host.c) on the
 * CPU, over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c), under AddressSanitizer + UBSan
 * (tests/test_op_host_cpu.py): range overlap and the conflict helper's order, the key kind of all eleven types, the
 * value-type predicate, the name lookup, the object head, and the staging of a host-data call — a round trip with a
 * caller's queue and with the queue made inside, the same with named copies on a profiling queue, and the failure on a
 * context without a device, with err and with err == NULL, without and with names, after which nothing is left allocated.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cl_ops.h"
#include "clo_internal.h"

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); ++failures; } } while (0)

static void test_ranges(void) {
	static char mem[64];
	const clo_range a = { mem, 16 }, next = { mem + 16, 16 }, last_byte = { mem + 15, 16 }, inside = { mem + 4, 2 },
		null_range = { NULL, 16 }, empty = { mem + 4, 0 };
	CHECK(!clo_ranges_overlap(a, next) && !clo_ranges_overlap(next, a), "adjacent ranges overlap");
	CHECK(clo_ranges_overlap(a, last_byte) && clo_ranges_overlap(last_byte, a), "one shared byte does not overlap");
	CHECK(clo_ranges_overlap(a, inside) && clo_ranges_overlap(inside, a), "a range inside another does not overlap");
	CHECK(clo_ranges_overlap(a, a), "a range does not overlap itself");
	CHECK(!clo_ranges_overlap(a, null_range) && !clo_ranges_overlap(null_range, a) && !clo_ranges_overlap(null_range, null_range), "NULL overlaps");
	CHECK(!clo_ranges_overlap(a, empty) && !clo_ranges_overlap(empty, a), "an empty range overlaps");

	/* inputs at 0 and 16; outputs: the first clean, the second on the first output AND on an input */
	const clo_range in[2] = { { mem, 8 }, { mem + 16, 8 } };
	const clo_range both[2] = { { mem + 32, 8 }, { mem + 20, 16 } };
	CHECK(clo_ranges_conflict(in, 2, both, 2) == CLO_RANGES_OUT_IN, "output-vs-input is not reported first");
	const clo_range outs[3] = { { mem + 32, 8 }, { mem + 48, 8 }, { mem + 39, 4 } };
	CHECK(clo_ranges_conflict(in, 2, outs, 3) == CLO_RANGES_OUT_OUT, "two outputs that overlap are not reported");
	/* an earlier output's clash with another output wins over a later output's clash with an input: output by output */
	const clo_range order[3] = { { mem + 32, 8 }, { mem + 36, 8 }, { mem, 4 } };
	CHECK(clo_ranges_conflict(in, 2, order, 3) == CLO_RANGES_OUT_OUT, "the outputs are not taken in order");
	const clo_range clean[3] = { { mem + 8, 8 }, { mem + 24, 8 }, { NULL, 64 } };
	CHECK(clo_ranges_conflict(in, 2, clean, 3) == 0, "ranges that only touch conflict");
	CHECK(clo_ranges_conflict(NULL, 0, clean, 1) == 0 && clo_ranges_conflict(in, 2, NULL, 0) == 0, "nothing conflicts");
}

static void test_types_and_names(void) {
	static const CloType types[11] = { CLO_CHAR, CLO_UCHAR, CLO_SHORT, CLO_USHORT, CLO_INT, CLO_UINT, CLO_LONG, CLO_ULONG, CLO_HALF, CLO_FLOAT, CLO_DOUBLE };
	static const int kinds[11] = { 1, 0, 1, 0, 1, 0, 1, 0, 2, 2, 2 };
	static const int wide[11] = { 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0 };
	for (int i = 0; i < 11; ++i) {
		CHECK(clo_type_key_kind(types[i]) == kinds[i], "key kind of %s: %d", clo_type_get_name(types[i]), clo_type_key_kind(types[i]));
		CHECK(clo_type_is_int32_or_64(types[i]) == wide[i], "int32_or_64 of %s", clo_type_get_name(types[i]));
	}
	static const char* const names[3] = { "sum", "min", "max" };
	CHECK(clo_name_index("sum", names, 3) == 0 && clo_name_index("max", names, 3) == 2, "a known name");
	CHECK(clo_name_index(NULL, names, 3) == -1, "NULL");
	CHECK(clo_name_index("Sum", names, 3) == -1 && clo_name_index("", names, 3) == -1 && clo_name_index("mi", names, 3) == -1, "an unknown name");
	CHECK(clo_name_index("max", names, 2) == -1 && clo_name_index("sum", names, 0) == -1, "a name past the count");
}

typedef struct { clo_op_head head; int own; } test_op;

static void test_head(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	test_op* op = (test_op*) clo_op_new(sizeof(test_op), ctx, &err);
	CHECK(op != NULL && err == NULL && op->head.ctx == ctx && op->own == 0 && op->head.workspace.ptr == NULL, "clo_op_new");
	if (!op) return;
	CHECK(clo_op_reserve(&op->head, cq, 100, "hipMalloc(test workspace)", &err) && err == NULL, "reserve");
	CHECK(op->head.workspace.ptr != NULL && op->head.workspace.bytes >= 100 && op->head.guard.cq == cq, "the workspace after reserve");
	void* const first = op->head.workspace.ptr;
	CHECK(clo_op_reserve(&op->head, cq, 50, "hipMalloc(test workspace)", NULL) && op->head.workspace.ptr == first, "a smaller size reallocates");
	clo_op_destroy(op);   /* the workspace, the hold on cq, the reference to ctx: ASan's leak check sees what stays */
}

static void test_buffers(CCLContext* ctx, CCLQueue* cq) {
	GError* err = NULL;
	CCLBuffer* b = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, 32, NULL, &err);
	CHECK(b != NULL && err == NULL, "buffer");
	if (!b) return;
	CCLBuffer* const buf[3] = { b, NULL, b };
	void* p[3] = { &err, &err, &err };
	clo_buffers_device_ptrs(buf, p, 3);
	CHECK(p[0] == ccl_buffer_get_device_ptr(b) && p[1] == NULL && p[2] == p[0], "device pointers");
	const size_t fits[3] = { 32, 1000, 0 }, too_long[3] = { 8, 0, 33 };
	CHECK(clo_buffers_hold(buf, fits, 3) && !clo_buffers_hold(buf, too_long, 3), "clo_buffers_hold");
	/* a command whose thin-ABI call failed is taken back, and says which call it was */
	CCLEvent* evt = ccl_queue_begin_command(cq, "test", &err);
	CHECK(evt != NULL && clo_op_end_command(cq, evt, 1, "clo_hip_test", &err) == NULL && err != NULL && err->domain == CCL_HIP_ERROR
		&& strstr(err->message, "clo_hip_test") != NULL, "a failed call: %s", err ? err->message : "no error");
	clo_gerror_clear(&err);
	evt = ccl_queue_begin_command(cq, "test", &err);
	CHECK(evt != NULL && clo_op_end_command(cq, evt, 0, "clo_hip_test", &err) == evt && err == NULL, "a call that worked");
	ccl_buffer_destroy(b);
}

/* upload -> (no device call) -> read back, with the caller's queue or with the one the stage makes */
static void test_stage_round_trip(CCLContext* ctx, CCLQueue* cq_exec, CCLQueue* cq_comm) {
	GError* err = NULL;
	const unsigned char in[7] = { 3, 1, 4, 1, 5, 9, 2 };
	unsigned char out[7] = { 0 }, untouched[4] = { 7, 7, 7, 7 };
	clo_stage st;
	clo_stage_open(&st, ctx, cq_exec, cq_comm);
	CHECK(clo_stage_ok(&st) && st.cq_exec != NULL && st.cq_comm == (cq_comm ? cq_comm : st.cq_exec)
		&& (cq_exec ? st.cq_exec == cq_exec && st.own_queue == NULL : st.own_queue == st.cq_exec), "open");
	clo_stage_in(&st, 0, in, sizeof in);
	clo_stage_in(&st, 1, NULL, 16);          /* no host pointer: no slot */
	clo_stage_in(&st, 2, in, 0);             /* nothing to hold: no slot */
	clo_stage_out(&st, 3, untouched, sizeof untouched);
	clo_stage_out(&st, CLO_STAGE_SLOTS - 1, NULL, 4);
	CHECK(clo_stage_ok(&st) && st.dev[0] && !st.dev[1] && !st.dev[2] && st.dev[3] && !st.dev[CLO_STAGE_SLOTS - 1], "the slots");
	CHECK(st.dev[0] && ccl_buffer_get_size(st.dev[0]) == sizeof in, "the slot's size");
	clo_stage_read(&st, 0, out, 5);          /* the first bytes of the slot */
	clo_stage_read(&st, 1, untouched, 4);    /* no slot: nothing is read */
	clo_stage_read(&st, 3, untouched, 0);    /* no bytes: nothing is read */
	CHECK(clo_stage_close(&st, &err) == CL_TRUE && err == NULL, "close: %s", err ? err->message : "");
	CHECK(memcmp(out, in, 5) == 0 && out[5] == 0 && out[6] == 0, "the bytes read back");
	CHECK(untouched[0] == 7 && untouched[3] == 7, "a read that should not have happened");
}

/* The same round trip on a stage with names, over a profiling transfer queue: the two copies reach a CCLProf consumer
 * under those names and no other; and a named stage leaves nothing out — an empty array gets its buffer and its copies. */
static void test_stage_names(CCLContext* ctx, CCLQueue* cq_exec, size_t bytes) {
	GError* err = NULL;
	const unsigned char in[7] = { 3, 1, 4, 1, 5, 9, 2 };
	unsigned char out[7] = { 0 };
	CCLQueue* prof_q = ccl_queue_new(ctx, NULL, CL_QUEUE_PROFILING_ENABLE, &err);
	CHECK(prof_q != NULL && err == NULL, "a profiling queue");
	if (!prof_q) return;
	clo_stage st;
	clo_stage_open(&st, ctx, cq_exec, prof_q);
	CHECK(st.write_name == NULL && st.read_name == NULL, "a stage is opened without names");
	st.write_name = "test_write";
	st.read_name = "test_read";
	clo_stage_in(&st, 0, in, bytes);
	CHECK(clo_stage_ok(&st) && st.dev[0] != NULL && ccl_buffer_get_size(st.dev[0]) == bytes, "the named slot");
	clo_stage_read(&st, 0, out, bytes);
	CHECK(clo_stage_close(&st, &err) == CL_TRUE && err == NULL, "close: %s", err ? err->message : "");
	CHECK(memcmp(out, in, bytes) == 0 && (bytes == sizeof in || out[bytes] == 0), "the bytes read back under a name");
	CCLProf* prof = ccl_prof_new();
	ccl_prof_add_queue(prof, "comm", prof_q);
	CHECK(ccl_prof_calc(prof, &err) && err == NULL, "ccl_prof_calc");
	int seen = 0;
	ccl_prof_iter_agg_init(prof, 0);
	while (ccl_prof_iter_agg_next(prof) != NULL) ++seen;
	CHECK(seen == 2 && ccl_prof_get_agg(prof, "test_write") != NULL && ccl_prof_get_agg(prof, "test_read") != NULL,
		"%d names on the transfer queue of a named stage of %zu bytes", seen, bytes);
	ccl_prof_destroy(prof);
	ccl_queue_destroy(prof_q);
}

/* on a context without a device and without a queue: the first step fails, the later ones do nothing, the error arrives */
static void test_stage_failure(int with_err, int named) {
	GError* err = NULL;
	CCLContext* off = ccl_context_new_offline(&err);
	CHECK(off != NULL && err == NULL, "offline context");
	if (!off) return;
	unsigned char bytes[4] = { 1, 2, 3, 4 }, out[4] = { 9, 9, 9, 9 };
	clo_stage st;
	clo_stage_open(&st, off, NULL, NULL);
	CHECK(!clo_stage_ok(&st) && st.own_queue == NULL, "a queue on an offline context");
	if (named) { st.write_name = "test_write"; st.read_name = "test_read"; }
	clo_stage_in(&st, 0, bytes, 4);
	clo_stage_out(&st, 1, out, 4);
	clo_stage_read(&st, 1, out, 4);
	CHECK(st.dev[0] == NULL && st.dev[1] == NULL && out[0] == 9, "steps after a failure");
	CHECK(clo_stage_close(&st, with_err ? &err : NULL) == CL_FALSE, "close after a failure");
	if (with_err) {
		CHECK(err != NULL && err->domain == CCL_HIP_ERROR && err->message && err->message[0], "the caller's error");
		clo_gerror_clear(&err);
	}
	ccl_context_destroy(off);
}

/* a failure the driver itself finds after buffers and the queue were made (a count above its bound): they are
 * released all the same, and nothing more is read */
static void test_stage_late_failure(CCLContext* ctx, int with_err) {
	GError* err = NULL;
	unsigned char bytes[4] = { 1, 2, 3, 4 }, out[4] = { 9, 9, 9, 9 };
	clo_stage st;
	clo_stage_open(&st, ctx, NULL, NULL);
	clo_stage_in(&st, 0, bytes, 4);
	clo_stage_out(&st, 1, out, 4);
	CHECK(clo_stage_ok(&st) && st.dev[0] && st.dev[1] && st.own_queue, "before the failure");
	clo_gerror_set(&st.err, CLO_ERROR, CLO_ERROR_LIBRARY, "a failure of the driver's own, %d", 7);
	clo_stage_read(&st, 0, out, 4);
	CHECK(out[0] == 9, "a read after a failure");
	CHECK(clo_stage_close(&st, with_err ? &err : NULL) == CL_FALSE, "close after the driver's failure");
	if (with_err) {
		CHECK(err != NULL && err->domain == CLO_ERROR && err->code == CLO_ERROR_LIBRARY && strstr(err->message, "7") != NULL, "the driver's error");
		clo_gerror_clear(&err);
	}
}

int main(void) {
	GError* err = NULL;
	CCLContext* ctx = ccl_context_new_from_device_index(0, &err);
	if (!ctx) { fprintf(stderr, "context: %s\n", err ? err->message : "?"); return 2; }
	CCLQueue* cq = ccl_queue_new(ctx, NULL, 0, &err);
	CCLQueue* cq2 = ccl_queue_new(ctx, NULL, 0, &err);
	if (!cq || !cq2) { fprintf(stderr, "queue: %s\n", err ? err->message : "?"); return 2; }
	test_ranges();
	test_types_and_names();
	test_head(ctx, cq);
	test_buffers(ctx, cq);
	test_stage_round_trip(ctx, cq, NULL);
	test_stage_round_trip(ctx, cq, cq2);
	test_stage_round_trip(ctx, NULL, NULL);    /* the queue made inside, destroyed by close */
	test_stage_round_trip(ctx, NULL, cq2);
	test_stage_names(ctx, cq, 7);
	test_stage_names(ctx, NULL, 5);
	test_stage_names(ctx, cq, 0);
	test_stage_failure(1, 0);
	test_stage_failure(0, 0);
	test_stage_failure(1, 1);
	test_stage_failure(0, 1);
	test_stage_late_failure(ctx, 1);
	test_stage_late_failure(ctx, 0);
	ccl_queue_destroy(cq2);
	ccl_queue_destroy(cq);
	ccl_context_destroy(ctx);
	if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
	else printf("op host ok\n");
	return failures ? 1 : 0;
}
