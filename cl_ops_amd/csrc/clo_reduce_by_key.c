/*
 * clo_reduce_by_key.c — CloReduceByKey (include/clo_reduce.h; not upstream): every run of equal keys collapsed
 * into one row. The kernels are reached through the thin C-ABI (clo_hip_reduce_by_key, include/clo_hip.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_reduce.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_REDUCE_BY_KEY_EVENT "clo_reduce_by_key"

struct clo_reduce_by_key {
	CCLContext* ctx;
	CloType key_type, value_type, sum_type;
	int op;                  /* index in rbk_ops: what clo_hip_reduce_by_key takes */
	clo_devbuf workspace;    /* the tile states; grows, never shrinks */
	clo_stream_guard guard;  /* the workspace belongs to one queue at a time */
};

static const char* const rbk_ops[] = { "sum", "min", "max" };

static int rbk_value_type_ok(CloType t) { return t == CLO_INT || t == CLO_UINT || t == CLO_LONG || t == CLO_ULONG; }

CloReduceByKey* clo_reduce_by_key_new(const char* op, const char* options, CCLContext* ctx,
	CloType key_type, CloType value_type, CloType sum_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	int opi = -1;
	for (int i = 0; op && i < 3; ++i)
		if (!strcmp(op, rbk_ops[i])) opi = i;
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown reduce-by-key operation '%s' (one of: " CLO_REDUCE_BY_KEY_OPS ").",
			op ? op : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for reduce by key.");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_reduce_by_key_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d.", (int) key_type);
		return NULL;
	}
	if (!rbk_value_type_ok(value_type) || !rbk_value_type_ok(sum_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Reduce by key takes values and sums of type int, uint, long or ulong "
			"(floating-point aggregates depend on the order of addition; narrower values are not built), not '%s' into '%s'.",
			clo_type_get_name(value_type) ? clo_type_get_name(value_type) : "?", clo_type_get_name(sum_type) ? clo_type_get_name(sum_type) : "?");
		return NULL;
	}
	if (clo_type_sizeof(sum_type) < clo_type_sizeof(value_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The sum type '%s' is narrower than the value type '%s'.",
			clo_type_get_name(sum_type), clo_type_get_name(value_type));
		return NULL;
	}
	CloReduceByKey* rbk = (CloReduceByKey*) calloc(1, sizeof(CloReduceByKey));
	if (!rbk) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	ccl_context_ref(ctx);
	rbk->ctx = ctx;
	rbk->key_type = key_type;
	rbk->value_type = value_type;
	rbk->sum_type = sum_type;
	rbk->op = opi;
	return rbk;
}

void clo_reduce_by_key_destroy(CloReduceByKey* rbk) {
	clo_return_if_fail(rbk != NULL);
	clo_devbuf_release(&rbk->workspace);
	clo_stream_guard_release(&rbk->guard);
	ccl_context_unref(rbk->ctx);
	free(rbk);
}

static int rbk_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
	if (!a || !b || !abytes || !bbytes) return 0;
	const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
	return a0 < b0 + bbytes && b0 < a0 + abytes;
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * count: the address of the run count (8 bytes), an output like the other two. */
static const char* rbk_refusal(CloReduceByKey* rbk, const void* keys_in, const void* values_in, const void* keys_out,
	const void* aggr_out, const void* count, size_t numel) {
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!count) return "the run count is required";
	if (!keys_out && !aggr_out) return "keys_out and aggr_out cannot both be NULL";
	if (aggr_out && !values_in && rbk->op != 0) return "min / max need values (without values every value is 1: only the sum, the run length, is offered)";
	if (numel > 0 && !keys_in) return "keys_in is required";
	const size_t kb = numel * clo_type_sizeof(rbk->key_type), vb = numel * clo_type_sizeof(rbk->value_type),
		sb = numel * clo_type_sizeof(rbk->sum_type);
	const void* in[2] = { keys_in, values_in };
	const size_t inb[2] = { kb, vb };
	const void* out[3] = { keys_out, aggr_out, count };
	const size_t outb[3] = { kb, sb, sizeof(cl_ulong) };
	for (int o = 0; o < 3; ++o) {
		for (int i = 0; i < 2; ++i)
			if (rbk_overlap(out[o], outb[o], in[i], inb[i]))
				return "an output range overlaps an input range (rows land below the elements they come from, in tiles that "
					"may not have been read yet: reduce by key does not work in place)";
		for (int p = 0; p < o; ++p)
			if (rbk_overlap(out[o], outb[o], out[p], outb[p])) return "two output ranges overlap";
	}
	return NULL;
}

CCLEvent* clo_reduce_by_key_with_device_data(CloReduceByKey* rbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out, CCLBuffer* aggr_out,
	CCLBuffer* num_runs_out, size_t numel, GError** err) {
	clo_return_val_if_fail(rbk != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	void* kin = keys_in ? ccl_buffer_get_device_ptr(keys_in) : NULL;
	void* vin = values_in ? ccl_buffer_get_device_ptr(values_in) : NULL;
	void* kout = keys_out ? ccl_buffer_get_device_ptr(keys_out) : NULL;
	void* aout = aggr_out ? ccl_buffer_get_device_ptr(aggr_out) : NULL;
	void* count = num_runs_out ? ccl_buffer_get_device_ptr(num_runs_out) : NULL;
	const char* why = rbk_refusal(rbk, kin, vin, kout, aout, count, numel);
	if (!why && ((uintptr_t) count & 7u)) why = "the run count must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t kb = numel * clo_type_sizeof(rbk->key_type), vb = numel * clo_type_sizeof(rbk->value_type),
		sb = numel * clo_type_sizeof(rbk->sum_type);
	if ((keys_in && kb > ccl_buffer_get_size(keys_in)) || (values_in && vb > ccl_buffer_get_size(values_in))
		|| (keys_out && kb > ccl_buffer_get_size(keys_out)) || (aggr_out && sb > ccl_buffer_get_size(aggr_out))
		|| ccl_buffer_get_size(num_runs_out) < sizeof(cl_ulong)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) exceeds the size of the device buffers", numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("REDUCE BY KEY: %s, numel=%zu, key %s, values %s, sum %s, keys out %s", rbk_ops[rbk->op], numel,
		clo_type_get_name(rbk->key_type), values_in ? clo_type_get_name(rbk->value_type) : "absent",
		aggr_out ? clo_type_get_name(rbk->sum_type) : "not written", keys_out ? "written" : "not written");

	if (numel > 0) {
		if (clo_hip_failed(clo_stream_guard_enter(&rbk->guard, cq_exec), err, "hipStreamWaitEvent")) return NULL;
		if (clo_hip_failed(clo_devbuf_reserve(&rbk->workspace, clo_hip_reduce_by_key_workspace_bytes(numel)), err,
			"hipMalloc(reduce-by-key workspace)")) return NULL;
	}
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_REDUCE_BY_KEY_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_reduce_by_key(kin, vin, kout, aout, (uint64_t*) count, numel, (int) clo_type_sizeof(rbk->key_type),
		(int) rbk->value_type, (int) rbk->sum_type, rbk->op, rbk->workspace.ptr, rbk->workspace.bytes, ccl_queue_get_stream(cq_exec));
	if (clo_hip_failed(st, err, "clo_hip_reduce_by_key")) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	if (!ccl_queue_end_command(cq_exec, evt, err)) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	return evt;
}

cl_bool clo_reduce_by_key_with_host_data(CloReduceByKey* rbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* keys_out, void* aggr_out,
	size_t* num_runs, size_t numel, GError** err) {
	clo_return_val_if_fail(rbk != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = rbk_refusal(rbk, keys_in, values_in, keys_out, aggr_out, num_runs, numel);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	*num_runs = 0;
	if (numel == 0) return CL_TRUE;

	cl_bool status = CL_FALSE;
	CCLBuffer* dev[5] = { NULL, NULL, NULL, NULL, NULL };   /* keys in, values in, keys out, aggregates out, run count */
	CCLQueue* intern_queue = NULL;
	CCLEvent* evt = NULL;
	CCLEventWaitList ewl = NULL;
	GError* err_internal = NULL;
	const size_t ks = clo_type_sizeof(rbk->key_type), vs = clo_type_sizeof(rbk->value_type), ss = clo_type_sizeof(rbk->sum_type);
	const size_t bytes[5] = { numel * ks, numel * vs, numel * ks, numel * ss, sizeof(cl_ulong) };
	const int used[5] = { 1, values_in != NULL, keys_out != NULL, aggr_out != NULL, 1 };
	cl_ulong m = 0;
	CCLContext* ctx = rbk->ctx;

	if (cq_exec == NULL) {
		CCLDevice* d = ccl_context_get_device(ctx, 0, &err_internal);
		if (err_internal) goto error_handler;
		intern_queue = ccl_queue_new(ctx, d, 0, &err_internal);
		if (err_internal) goto error_handler;
		cq_exec = intern_queue;
	}
	if (cq_comm == NULL) cq_comm = cq_exec;
	for (int i = 0; i < 5; ++i) {
		if (!used[i]) continue;
		dev[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i], NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	ccl_buffer_enqueue_write(dev[0], cq_comm, CL_TRUE, 0, bytes[0], (void*) keys_in, NULL, &err_internal);
	if (err_internal) goto error_handler;
	if (values_in) {
		ccl_buffer_enqueue_write(dev[1], cq_comm, CL_TRUE, 0, bytes[1], (void*) values_in, NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	evt = clo_reduce_by_key_with_device_data(rbk, cq_exec, cq_comm, dev[0], dev[1], dev[2], dev[3], dev[4], numel, &err_internal);
	if (err_internal) goto error_handler;
	/* the run count first (blocking): it says how many rows there are to copy */
	ccl_buffer_enqueue_read(dev[4], cq_comm, CL_TRUE, 0, sizeof(cl_ulong), &m, evt ? ccl_ewl(&ewl, evt, NULL) : NULL, &err_internal);
	if (err_internal) goto error_handler;
	if (m > numel) {
		clo_gerror_set(&err_internal, CLO_ERROR, CLO_ERROR_LIBRARY, "reduce by key: %llu runs of %zu elements", (unsigned long long) m, numel);
		goto error_handler;
	}
	if (keys_out) {
		ccl_buffer_enqueue_read(dev[2], cq_comm, CL_TRUE, 0, (size_t) m * ks, keys_out, NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	if (aggr_out) {
		ccl_buffer_enqueue_read(dev[3], cq_comm, CL_TRUE, 0, (size_t) m * ss, aggr_out, NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	*num_runs = (size_t) m;
	status = CL_TRUE;
	goto finish;

error_handler:
	clo_gerror_propagate(err, err_internal);
	status = CL_FALSE;

finish:
	ccl_event_wait_list_clear(&ewl);
	for (int i = 0; i < 5; ++i) if (dev[i]) ccl_buffer_destroy(dev[i]);
	if (intern_queue) ccl_queue_destroy(intern_queue);
	return status;
}

CCLContext* clo_reduce_by_key_get_context(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, NULL);
	return rbk->ctx;
}

CloType clo_reduce_by_key_get_key_type(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, (CloType) -1);
	return rbk->key_type;
}

size_t clo_reduce_by_key_get_key_size(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, 0);
	return clo_type_sizeof(rbk->key_type);
}

CloType clo_reduce_by_key_get_value_type(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, (CloType) -1);
	return rbk->value_type;
}

size_t clo_reduce_by_key_get_value_size(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, 0);
	return clo_type_sizeof(rbk->value_type);
}

CloType clo_reduce_by_key_get_sum_type(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, (CloType) -1);
	return rbk->sum_type;
}

size_t clo_reduce_by_key_get_sum_size(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, 0);
	return clo_type_sizeof(rbk->sum_type);
}

const char* clo_reduce_by_key_get_op(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, NULL);
	return rbk_ops[rbk->op];
}
