/* clo_op_host.c — the host layer the operation drivers share: see clo_internal.h. */
#include "clo_internal.h"

#include <stdint.h>
#include <string.h>

int clo_type_key_kind(CloType t) {
	return clo_type_is_float(t) ? 2 : (clo_type_is_signed(t) ? 1 : 0);
}

int clo_type_is_int32_or_64(CloType t) {
	return t == CLO_INT || t == CLO_UINT || t == CLO_LONG || t == CLO_ULONG;
}

int clo_name_index(const char* name, const char* const* names, int count) {
	for (int i = 0; name && i < count; ++i)
		if (!strcmp(name, names[i])) return i;
	return -1;
}

int clo_ranges_overlap(clo_range a, clo_range b) {
	if (!a.p || !b.p || !a.bytes || !b.bytes) return 0;
	const uintptr_t a0 = (uintptr_t) a.p, b0 = (uintptr_t) b.p;
	return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

int clo_ranges_conflict(const clo_range* in, int nin, const clo_range* out, int nout) {
	for (int o = 0; o < nout; ++o) {
		for (int i = 0; i < nin; ++i)
			if (clo_ranges_overlap(out[o], in[i])) return CLO_RANGES_OUT_IN;
		for (int p = 0; p < o; ++p)
			if (clo_ranges_overlap(out[o], out[p])) return CLO_RANGES_OUT_OUT;
	}
	return 0;
}

void* clo_op_new(size_t size, CCLContext* ctx, GError** err) {
	clo_op_head* op = (clo_op_head*) calloc(1, size);
	if (!op) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	ccl_context_ref(ctx);
	op->ctx = ctx;
	return op;
}

void clo_op_destroy(void* op) {
	clo_op_head* head = (clo_op_head*) op;
	clo_devbuf_release(&head->workspace);
	clo_stream_guard_release(&head->guard);
	ccl_context_unref(head->ctx);
	free(op);
}

int clo_op_reserve(clo_op_head* op, CCLQueue* cq, size_t ws, const char* what, GError** err) {
	return !clo_hip_failed(clo_stream_guard_enter(&op->guard, cq), err, "hipStreamWaitEvent")
		&& !clo_hip_failed(clo_devbuf_reserve(&op->workspace, ws), err, what);
}

void clo_buffers_device_ptrs(CCLBuffer* const* buf, void** p, int n) {
	for (int i = 0; i < n; ++i) p[i] = buf[i] ? ccl_buffer_get_device_ptr(buf[i]) : NULL;
}

int clo_buffers_hold(CCLBuffer* const* buf, const size_t* need, int n) {
	for (int i = 0; i < n; ++i)
		if (buf[i] && need[i] > ccl_buffer_get_size(buf[i])) return 0;
	return 1;
}

CCLEvent* clo_op_end_command(CCLQueue* cq, CCLEvent* evt, int st, const char* what, GError** err) {
	if (clo_hip_failed(st, err, what) || !ccl_queue_end_command(cq, evt, err)) {
		ccl_queue_abort_command(cq, evt);
		return NULL;
	}
	return evt;
}

void clo_stage_open(clo_stage* st, CCLContext* ctx, CCLQueue* cq_exec, CCLQueue* cq_comm) {
	memset(st, 0, sizeof(*st));
	st->ctx = ctx;
	if (cq_exec == NULL) {
		CCLDevice* d = ccl_context_get_device(ctx, 0, &st->err);
		if (!st->err) st->own_queue = ccl_queue_new(ctx, d, 0, &st->err);
		cq_exec = st->own_queue;
	}
	st->cq_exec = cq_exec;
	st->cq_comm = cq_comm ? cq_comm : cq_exec;
}

/* One transfer of a slot on cq_comm: blocking, or — under a name — enqueued, named and waited for with ccl_event_wait. */
static void stage_copy(clo_stage* st, int slot, int read, const char* name, size_t bytes, void* host, CCLEventWaitList* after) {
	CCLEvent* e = (read ? ccl_buffer_enqueue_read : ccl_buffer_enqueue_write)(st->dev[slot], st->cq_comm, name ? CL_FALSE : CL_TRUE,
		0, bytes, host, after, &st->err);
	if (!name || st->err) return;
	ccl_event_set_name(e, name);
	ccl_event_wait(ccl_ewl(&st->ewl, e, NULL), &st->err);
}

/* (a named transfer is never left out: an empty array still gets its buffer and its named copy, as upstream's path does) */
void clo_stage_out(clo_stage* st, int slot, const void* host, size_t bytes) {
	if (st->err || (!st->read_name && (!host || bytes == 0))) return;
	st->dev[slot] = ccl_buffer_new(st->ctx, CL_MEM_READ_WRITE, bytes, NULL, &st->err);
}

void clo_stage_in(clo_stage* st, int slot, const void* host, size_t bytes) {
	if (st->err || (!st->write_name && (!host || bytes == 0))) return;
	st->dev[slot] = ccl_buffer_new(st->ctx, CL_MEM_READ_WRITE, bytes, NULL, &st->err);
	if (!st->err && st->dev[slot]) stage_copy(st, slot, 0, st->write_name, bytes, (void*) host, NULL);
}

void clo_stage_read(clo_stage* st, int slot, void* host, size_t bytes) {
	if (st->err || !st->dev[slot] || (bytes == 0 && !st->read_name)) return;
	/* the first read waits for the device call and blocks; the later ones find it done */
	stage_copy(st, slot, 1, st->read_name, bytes, host, st->evt ? ccl_ewl(&st->ewl, st->evt, NULL) : NULL);
	st->evt = NULL;
}

cl_bool clo_stage_close(clo_stage* st, GError** err) {
	const cl_bool status = st->err ? CL_FALSE : CL_TRUE;
	if (st->err) clo_gerror_propagate(err, st->err);
	st->err = NULL;
	ccl_event_wait_list_clear(&st->ewl);
	for (int i = 0; i < CLO_STAGE_SLOTS; ++i) if (st->dev[i]) ccl_buffer_destroy(st->dev[i]);
	if (st->own_queue) ccl_queue_destroy(st->own_queue);
	return status;
}
