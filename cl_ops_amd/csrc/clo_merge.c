/*
 * clo_merge.c — CloMerge (include/clo_merge.h; not upstream): the stable merge of two sorted arrays, with values
 * or as argmerge. The kernels are reached through the thin C-ABI (clo_hip_merge, include/clo_hip.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_merge.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_MERGE_EVENT "clo_merge"

struct clo_merge {
	CCLContext* ctx;
	CloType key_type;
	size_t value_size;
	clo_devbuf workspace;    /* the tiles' split points (clo_hip_merge_workspace_bytes); grows, never shrinks */
	clo_stream_guard guard;  /* the workspace belongs to one queue at a time */
};

/* 0 unsigned, 1 signed, 2 IEEE total order: the key kinds of clo_sort_by_key_* */
static int merge_key_kind(CloType t) {
	if (t == CLO_CHAR || t == CLO_SHORT || t == CLO_INT || t == CLO_LONG) return 1;
	if (t == CLO_HALF || t == CLO_FLOAT || t == CLO_DOUBLE) return 2;
	return 0;
}

CloMerge* clo_merge_new(const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for merge (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_merge_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for merge.", (int) key_type);
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Merge carries values of 0 (none), 4 or 8 bytes, not a value_size of %zu.", value_size);
		return NULL;
	}
	CloMerge* m = (CloMerge*) calloc(1, sizeof(CloMerge));
	if (!m) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	ccl_context_ref(ctx);
	m->ctx = ctx;
	m->key_type = key_type;
	m->value_size = value_size;
	return m;
}

void clo_merge_destroy(CloMerge* m) {
	clo_return_if_fail(m != NULL);
	clo_devbuf_release(&m->workspace);
	clo_stream_guard_release(&m->guard);
	ccl_context_unref(m->ctx);
	free(m);
}

typedef struct { const void* p; size_t bytes; } merge_range;

static int merge_overlap(merge_range a, merge_range b) {
	if (!a.p || !b.p || !a.bytes || !b.bytes) return 0;
	const uintptr_t a0 = (uintptr_t) a.p, b0 = (uintptr_t) b.p;
	return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced. */
static const char* merge_refusal(CloMerge* m, const void* keys_a, const void* values_a, size_t numel_a,
	const void* keys_b, const void* values_b, size_t numel_b, const void* keys_out, const void* values_out) {
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull)
		return "numel_a + numel_b must be below 2^32";
	if (numel_a > 0 && !keys_a) return "keys_a is required";
	if (numel_b > 0 && !keys_b) return "keys_b is required";
	if (!keys_out && !values_out) return "keys_out and values_out are both NULL";
	if (m->value_size == 0 && (values_a || values_b || values_out)) return "values passed to a merge made with value_size 0";
	if (m->value_size > 0 && !values_out) return "values_out is required with a value_size above 0";
	if (numel_a > 0 && numel_b > 0 && (values_a == NULL) != (values_b == NULL))
		return "values_a and values_b must both be given, or both be NULL (argmerge)";
	if (m->value_size == 8 && ((numel_a > 0 && !values_a) || (numel_b > 0 && !values_b)))
		return "NULL values (argmerge) need a value_size of 4: the permutation is written as uint";
	const size_t ks = clo_type_sizeof(m->key_type), vs = m->value_size, n = numel_a + numel_b;
	const merge_range in[4] = { { keys_a, numel_a * ks }, { keys_b, numel_b * ks }, { values_a, numel_a * vs }, { values_b, numel_b * vs } };
	const merge_range out[2] = { { keys_out, n * ks }, { values_out, n * vs } };
	for (int o = 0; o < 2; ++o)
		for (int i = 0; i < 4; ++i)
			if (merge_overlap(out[o], in[i])) return "an output range overlaps an input range (there is no in-place merge)";
	if (merge_overlap(out[0], out[1])) return "keys_out overlaps values_out";
	return NULL;
}

CCLEvent* clo_merge_with_device_data(CloMerge* m, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_a, CCLBuffer* values_a, size_t numel_a, CCLBuffer* keys_b, CCLBuffer* values_b, size_t numel_b,
	CCLBuffer* keys_out, CCLBuffer* values_out, GError** err) {
	clo_return_val_if_fail(m != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[6] = { keys_a, values_a, keys_b, values_b, keys_out, values_out };
	void* p[6];
	for (int i = 0; i < 6; ++i) p[i] = buf[i] ? ccl_buffer_get_device_ptr(buf[i]) : NULL;
	const char* why = merge_refusal(m, p[0], p[1], numel_a, p[2], p[3], numel_b, p[4], p[5]);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(m->key_type), vs = m->value_size, n = numel_a + numel_b;
	const size_t need[6] = { numel_a * ks, numel_a * vs, numel_b * ks, numel_b * vs, n * ks, n * vs };
	for (int i = 0; i < 6; ++i) {
		if (buf[i] && need[i] > ccl_buffer_get_size(buf[i])) {
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_a (%zu) and numel_b (%zu) exceed the size of the device buffers", numel_a, numel_b);
			return NULL;
		}
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("MERGE: %zu + %zu keys of type %s, %s", numel_a, numel_b, clo_type_get_name(m->key_type),
		vs == 0 ? "no values" : ((numel_a > 0 && !p[1]) || (numel_b > 0 && !p[3])) ? "argmerge" : vs == 4 ? "4-byte values" : "8-byte values");

	const size_t ws = clo_hip_merge_workspace_bytes(numel_a, numel_b);
	if (ws > 0) {
		if (clo_hip_failed(clo_stream_guard_enter(&m->guard, cq_exec), err, "hipStreamWaitEvent")) return NULL;
		if (clo_hip_failed(clo_devbuf_reserve(&m->workspace, ws), err, "hipMalloc(merge workspace)")) return NULL;
	}
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_MERGE_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_merge(p[0], p[1], numel_a, p[2], p[3], numel_b, p[4], p[5], (int) ks, merge_key_kind(m->key_type), (int) vs,
		m->workspace.ptr, m->workspace.bytes, ccl_queue_get_stream(cq_exec));
	if (clo_hip_failed(st, err, "clo_hip_merge")) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	if (!ccl_queue_end_command(cq_exec, evt, err)) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	return evt;
}

cl_bool clo_merge_with_host_data(CloMerge* m, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_a, const void* values_a, size_t numel_a, const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, GError** err) {
	clo_return_val_if_fail(m != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = merge_refusal(m, keys_a, values_a, numel_a, keys_b, values_b, numel_b, keys_out, values_out);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const size_t n = numel_a + numel_b;
	if (n == 0) return CL_TRUE;   /* no device needed */

	cl_bool status = CL_FALSE;
	const size_t ks = clo_type_sizeof(m->key_type), vs = m->value_size;
	/* keys a, values a, keys b, values b, keys out, values out */
	const void* const host[6] = { keys_a, values_a, keys_b, values_b, keys_out, values_out };
	const size_t bytes[6] = { numel_a * ks, numel_a * vs, numel_b * ks, numel_b * vs, n * ks, n * vs };
	CCLBuffer* dev[6] = { NULL, NULL, NULL, NULL, NULL, NULL };
	CCLQueue* intern_queue = NULL;
	CCLEvent* evt = NULL;
	CCLEventWaitList ewl = NULL;
	GError* err_internal = NULL;
	CCLContext* ctx = m->ctx;

	if (cq_exec == NULL) {
		CCLDevice* d = ccl_context_get_device(ctx, 0, &err_internal);
		if (err_internal) goto error_handler;
		intern_queue = ccl_queue_new(ctx, d, 0, &err_internal);
		if (err_internal) goto error_handler;
		cq_exec = intern_queue;
	}
	if (cq_comm == NULL) cq_comm = cq_exec;
	for (int i = 0; i < 6; ++i) {
		if (!host[i] || bytes[i] == 0) continue;
		dev[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i], NULL, &err_internal);
		if (err_internal) goto error_handler;
		if (i < 4) {
			ccl_buffer_enqueue_write(dev[i], cq_comm, CL_TRUE, 0, bytes[i], (void*) host[i], NULL, &err_internal);
			if (err_internal) goto error_handler;
		}
	}
	evt = clo_merge_with_device_data(m, cq_exec, cq_comm, dev[0], dev[1], numel_a, dev[2], dev[3], numel_b, dev[4], dev[5], &err_internal);
	if (err_internal) goto error_handler;
	for (int i = 4; i < 6; ++i) {
		if (!dev[i]) continue;
		/* the first read waits for the merge and blocks; the second finds it done */
		ccl_buffer_enqueue_read(dev[i], cq_comm, CL_TRUE, 0, bytes[i], (void*) host[i], evt ? ccl_ewl(&ewl, evt, NULL) : NULL, &err_internal);
		if (err_internal) goto error_handler;
		evt = NULL;
	}
	status = CL_TRUE;
	goto finish;

error_handler:
	clo_gerror_propagate(err, err_internal);
	status = CL_FALSE;

finish:
	ccl_event_wait_list_clear(&ewl);
	for (int i = 0; i < 6; ++i) if (dev[i]) ccl_buffer_destroy(dev[i]);
	if (intern_queue) ccl_queue_destroy(intern_queue);
	return status;
}

CCLContext* clo_merge_get_context(CloMerge* m) {
	clo_return_val_if_fail(m != NULL, NULL);
	return m->ctx;
}

CloType clo_merge_get_key_type(CloMerge* m) {
	clo_return_val_if_fail(m != NULL, (CloType) -1);
	return m->key_type;
}

size_t clo_merge_get_key_size(CloMerge* m) {
	clo_return_val_if_fail(m != NULL, 0);
	return clo_type_sizeof(m->key_type);
}

size_t clo_merge_get_value_size(CloMerge* m) {
	clo_return_val_if_fail(m != NULL, 0);
	return m->value_size;
}
