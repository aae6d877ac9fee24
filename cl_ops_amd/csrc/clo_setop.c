/*
 * clo_setop.c — CloSetOp (include/clo_setop.h; not upstream): union, intersection, difference and symmetric
 * difference of two sorted arrays as multisets, with values or as indices. The kernels are reached through the thin
 * C-ABI (clo_hip_setop, include/clo_hip.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_setop.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SETOP_EVENT "clo_setop"

struct clo_setop {
	CCLContext* ctx;
	int op;                  /* index in setop_ops: what clo_hip_setop takes */
	CloType key_type;
	size_t value_size;
	clo_devbuf workspace;    /* split points and kept counts (clo_hip_setop_workspace_bytes); grows, never shrinks */
	clo_stream_guard guard;  /* the workspace belongs to one queue at a time */
};

static const char* const setop_ops[] = { "union", "intersection", "difference", "symmetric_difference" };

/* 0 unsigned, 1 signed, 2 IEEE total order: the key kinds of clo_sort_by_key_* */
static int setop_key_kind(CloType t) {
	if (t == CLO_CHAR || t == CLO_SHORT || t == CLO_INT || t == CLO_LONG) return 1;
	if (t == CLO_HALF || t == CLO_FLOAT || t == CLO_DOUBLE) return 2;
	return 0;
}

/* union and symmetric difference keep elements of B; the other two never look at values_b */
static int setop_keeps_b(int op) { return op == CLO_HIP_SETOP_UNION || op == CLO_HIP_SETOP_SYMMETRIC_DIFFERENCE; }

static size_t setop_capacity(int op, size_t numel_a, size_t numel_b) {
	if (setop_keeps_b(op)) return numel_a + numel_b;
	if (op == CLO_HIP_SETOP_DIFFERENCE) return numel_a;
	return numel_a < numel_b ? numel_a : numel_b;
}

CloSetOp* clo_setop_new(const char* op, const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	int opi = -1;
	for (int i = 0; op && i < 4; ++i)
		if (!strcmp(op, setop_ops[i])) opi = i;
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown set operation '%s' (one of: " CLO_SETOP_OPS ").", op ? op : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a set operation (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_setop_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for a set operation.", (int) key_type);
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A set operation carries values of 0 (none), 4 or 8 bytes, not a value_size of %zu.", value_size);
		return NULL;
	}
	CloSetOp* so = (CloSetOp*) calloc(1, sizeof(CloSetOp));
	if (!so) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	ccl_context_ref(ctx);
	so->ctx = ctx;
	so->op = opi;
	so->key_type = key_type;
	so->value_size = value_size;
	return so;
}

void clo_setop_destroy(CloSetOp* so) {
	clo_return_if_fail(so != NULL);
	clo_devbuf_release(&so->workspace);
	clo_stream_guard_release(&so->guard);
	ccl_context_unref(so->ctx);
	free(so);
}

typedef struct { const void* p; size_t bytes; } setop_range;

static int setop_overlap(setop_range a, setop_range b) {
	if (!a.p || !b.p || !a.bytes || !b.bytes) return 0;
	const uintptr_t a0 = (uintptr_t) a.p, b0 = (uintptr_t) b.p;
	return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * count_bytes: the size of what num_out points to (a cl_ulong of the device, a size_t of the host). */
static const char* setop_refusal(CloSetOp* so, const void* keys_a, const void* values_a, size_t numel_a,
	const void* keys_b, const void* values_b, size_t numel_b, const void* keys_out, const void* values_out,
	const void* num_out, size_t count_bytes) {
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull)
		return "numel_a + numel_b must be below 2^32";
	if (numel_a > 0 && !keys_a) return "keys_a is required";
	if (numel_b > 0 && !keys_b) return "keys_b is required";
	if (!num_out) return "num_out is required";
	if (!keys_out && !values_out) return "keys_out and values_out are both NULL";
	if (so->value_size == 0 && (values_a || values_b || values_out)) return "values passed to a set operation made with value_size 0";
	if (so->value_size > 0 && !values_out) return "values_out is required with a value_size above 0";
	const int keeps_b = setop_keeps_b(so->op);
	if (keeps_b && numel_a > 0 && numel_b > 0 && (values_a == NULL) != (values_b == NULL))
		return "values_a and values_b must both be given, or both be NULL (the arg form)";
	if (so->value_size == 8 && ((numel_a > 0 && !values_a) || (keeps_b && numel_b > 0 && !values_b)))
		return "NULL values (the arg form) need a value_size of 4: the indices are written as uint";
	const size_t ks = clo_type_sizeof(so->key_type), vs = so->value_size, cap = setop_capacity(so->op, numel_a, numel_b);
	const setop_range in[4] = { { keys_a, numel_a * ks }, { keys_b, numel_b * ks }, { values_a, numel_a * vs },
		{ keeps_b ? values_b : NULL, numel_b * vs } };
	const setop_range out[3] = { { keys_out, cap * ks }, { values_out, cap * vs }, { num_out, count_bytes } };
	for (int o = 0; o < 3; ++o) {
		for (int i = 0; i < 4; ++i)
			if (setop_overlap(out[o], in[i])) return "an output range overlaps an input range (there is no in-place set operation)";
		for (int p = 0; p < o; ++p)
			if (setop_overlap(out[o], out[p])) return "two output ranges overlap";
	}
	return NULL;
}

CCLEvent* clo_setop_with_device_data(CloSetOp* so, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_a, CCLBuffer* values_a, size_t numel_a, CCLBuffer* keys_b, CCLBuffer* values_b, size_t numel_b,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* num_out, GError** err) {
	clo_return_val_if_fail(so != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[7] = { keys_a, values_a, keys_b, values_b, keys_out, values_out, num_out };
	void* p[7];
	for (int i = 0; i < 7; ++i) p[i] = buf[i] ? ccl_buffer_get_device_ptr(buf[i]) : NULL;
	const char* why = setop_refusal(so, p[0], p[1], numel_a, p[2], p[3], numel_b, p[4], p[5], p[6], sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[6] & 7u)) why = "num_out must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const int keeps_b = setop_keeps_b(so->op);
	const size_t ks = clo_type_sizeof(so->key_type), vs = so->value_size, cap = setop_capacity(so->op, numel_a, numel_b);
	const size_t need[7] = { numel_a * ks, numel_a * vs, numel_b * ks, keeps_b ? numel_b * vs : 0, cap * ks, cap * vs, sizeof(cl_ulong) };
	for (int i = 0; i < 7; ++i) {
		if (buf[i] && need[i] > ccl_buffer_get_size(buf[i])) {
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_a (%zu) and numel_b (%zu) exceed the size of the device buffers "
				"(the outputs hold %zu elements, num_out 8 bytes)", numel_a, numel_b, cap);
			return NULL;
		}
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SETOP: %s of %zu + %zu keys of type %s, %s", setop_ops[so->op], numel_a, numel_b, clo_type_get_name(so->key_type),
		vs == 0 ? "no values" : ((numel_a > 0 && !p[1]) || (keeps_b && numel_b > 0 && !p[3])) ? "indices" : vs == 4 ? "4-byte values" : "8-byte values");

	const size_t ws = clo_hip_setop_workspace_bytes(numel_a, numel_b);
	if (ws > 0) {
		if (clo_hip_failed(clo_stream_guard_enter(&so->guard, cq_exec), err, "hipStreamWaitEvent")) return NULL;
		if (clo_hip_failed(clo_devbuf_reserve(&so->workspace, ws), err, "hipMalloc(setop workspace)")) return NULL;
	}
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SETOP_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_setop(so->op, p[0], p[1], numel_a, p[2], keeps_b ? p[3] : NULL, numel_b, p[4], p[5], (uint64_t*) p[6],
		(int) ks, setop_key_kind(so->key_type), (int) vs, so->workspace.ptr, so->workspace.bytes, ccl_queue_get_stream(cq_exec));
	if (clo_hip_failed(st, err, "clo_hip_setop")) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	if (!ccl_queue_end_command(cq_exec, evt, err)) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	return evt;
}

cl_bool clo_setop_with_host_data(CloSetOp* so, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_a, const void* values_a, size_t numel_a, const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, size_t* num_out, GError** err) {
	clo_return_val_if_fail(so != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = setop_refusal(so, keys_a, values_a, numel_a, keys_b, values_b, numel_b, keys_out, values_out, num_out, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	*num_out = 0;
	const size_t cap = setop_capacity(so->op, numel_a, numel_b);
	if (cap == 0) return CL_TRUE;   /* nothing can be kept: no device needed */

	cl_bool status = CL_FALSE;
	const size_t ks = clo_type_sizeof(so->key_type), vs = so->value_size;
	const int keeps_b = setop_keeps_b(so->op);
	/* keys a, values a, keys b, values b, keys out, values out, the count */
	const void* const host[7] = { keys_a, values_a, keys_b, keeps_b ? values_b : NULL, keys_out, values_out, num_out };
	const size_t bytes[7] = { numel_a * ks, numel_a * vs, numel_b * ks, numel_b * vs, cap * ks, cap * vs, sizeof(cl_ulong) };
	CCLBuffer* dev[7] = { NULL, NULL, NULL, NULL, NULL, NULL, NULL };
	CCLQueue* intern_queue = NULL;
	CCLEvent* evt = NULL;
	CCLEventWaitList ewl = NULL;
	GError* err_internal = NULL;
	cl_ulong k = 0;
	CCLContext* ctx = so->ctx;

	if (cq_exec == NULL) {
		CCLDevice* d = ccl_context_get_device(ctx, 0, &err_internal);
		if (err_internal) goto error_handler;
		intern_queue = ccl_queue_new(ctx, d, 0, &err_internal);
		if (err_internal) goto error_handler;
		cq_exec = intern_queue;
	}
	if (cq_comm == NULL) cq_comm = cq_exec;
	for (int i = 0; i < 7; ++i) {
		if (!host[i] || bytes[i] == 0) continue;
		dev[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i], NULL, &err_internal);
		if (err_internal) goto error_handler;
		if (i < 4) {
			ccl_buffer_enqueue_write(dev[i], cq_comm, CL_TRUE, 0, bytes[i], (void*) host[i], NULL, &err_internal);
			if (err_internal) goto error_handler;
		}
	}
	evt = clo_setop_with_device_data(so, cq_exec, cq_comm, dev[0], dev[1], numel_a, dev[2], dev[3], numel_b, dev[4], dev[5], dev[6], &err_internal);
	if (err_internal) goto error_handler;
	/* the count first (blocking): it says how many rows there are to copy */
	ccl_buffer_enqueue_read(dev[6], cq_comm, CL_TRUE, 0, sizeof(cl_ulong), &k, evt ? ccl_ewl(&ewl, evt, NULL) : NULL, &err_internal);
	if (err_internal) goto error_handler;
	if (k > cap) {
		clo_gerror_set(&err_internal, CLO_ERROR, CLO_ERROR_LIBRARY, "set operation: %llu rows in outputs of %zu", (unsigned long long) k, cap);
		goto error_handler;
	}
	for (int i = 4; i < 6; ++i) {
		if (!dev[i] || k == 0) continue;
		ccl_buffer_enqueue_read(dev[i], cq_comm, CL_TRUE, 0, (size_t) k * (i == 4 ? ks : vs), (void*) host[i], NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	*num_out = (size_t) k;
	status = CL_TRUE;
	goto finish;

error_handler:
	clo_gerror_propagate(err, err_internal);
	status = CL_FALSE;

finish:
	ccl_event_wait_list_clear(&ewl);
	for (int i = 0; i < 7; ++i) if (dev[i]) ccl_buffer_destroy(dev[i]);
	if (intern_queue) ccl_queue_destroy(intern_queue);
	return status;
}

CCLContext* clo_setop_get_context(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, NULL);
	return so->ctx;
}

CloType clo_setop_get_key_type(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, (CloType) -1);
	return so->key_type;
}

size_t clo_setop_get_key_size(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, 0);
	return clo_type_sizeof(so->key_type);
}

size_t clo_setop_get_value_size(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, 0);
	return so->value_size;
}

const char* clo_setop_get_op(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, NULL);
	return setop_ops[so->op];
}

size_t clo_setop_get_max_numel_out(CloSetOp* so, size_t numel_a, size_t numel_b) {
	clo_return_val_if_fail(so != NULL, 0);
	return setop_capacity(so->op, numel_a, numel_b);
}
