/*
 * clo_scan_by_key.c — CloScanByKey (include/clo_scan_by_key.h; not upstream): the running sum / min / max of every
 * element within its run of equal keys. The kernels are reached through the thin C-ABI (clo_hip_scan_by_key,
 * include/clo_hip.h). Follows clo_reduce_by_key.c point for point.
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_scan_by_key.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SCAN_BY_KEY_EVENT "clo_scan_by_key"

struct clo_scan_by_key {
	CCLContext* ctx;
	CloType key_type, value_type, sum_type;
	int op;                  /* index in sbk_ops: what clo_hip_scan_by_key takes */
	int inclusive;           /* 0 or 1 */
	clo_devbuf workspace;    /* the tile states; grows, never shrinks */
	clo_stream_guard guard;  /* the workspace belongs to one queue at a time */
};

static const char* const sbk_ops[] = { "sum", "min", "max" };

static int sbk_value_type_ok(CloType t) { return t == CLO_INT || t == CLO_UINT || t == CLO_LONG || t == CLO_ULONG; }

/* the one option there is: inclusive=0 | inclusive=1 */
static int sbk_option(const char* key, const char* value, const char* token, void* user, GError** err) {
	if (strcmp(key, "inclusive") == 0 && (strcmp(value, "0") == 0 || strcmp(value, "1") == 0)) {
		*(int*) user = value[0] == '1';
		return 1;
	}
	clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for scan by key: '%s' (inclusive=0 or inclusive=1).", token);
	return 0;
}

CloScanByKey* clo_scan_by_key_new(const char* op, const char* options, CCLContext* ctx,
	CloType key_type, CloType value_type, CloType sum_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	int opi = -1;
	for (int i = 0; op && i < 3; ++i)
		if (!strcmp(op, sbk_ops[i])) opi = i;
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown scan-by-key operation '%s' (one of: " CLO_SCAN_BY_KEY_OPS ").",
			op ? op : "(null)");
		return NULL;
	}
	int inclusive = 0;
	GError* err_opt = NULL;
	if (!clo_parse_options(options, sbk_option, &inclusive, "scan-by-key", &err_opt)) {
		/* (an option without '=' comes back with the parser's own wording, which names a sort) */
		if (err_opt) clo_gerror_free(err_opt);
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for scan by key: '%s' (inclusive=0 or inclusive=1).", options);
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_scan_by_key_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d.", (int) key_type);
		return NULL;
	}
	if (!sbk_value_type_ok(value_type) || !sbk_value_type_ok(sum_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Scan by key takes values and sums of type int, uint, long or ulong "
			"(floating-point aggregates depend on the order of addition; narrower values are not built), not '%s' into '%s'.",
			clo_type_get_name(value_type) ? clo_type_get_name(value_type) : "?", clo_type_get_name(sum_type) ? clo_type_get_name(sum_type) : "?");
		return NULL;
	}
	if (clo_type_sizeof(sum_type) < clo_type_sizeof(value_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The sum type '%s' is narrower than the value type '%s'.",
			clo_type_get_name(sum_type), clo_type_get_name(value_type));
		return NULL;
	}
	CloScanByKey* sbk = (CloScanByKey*) calloc(1, sizeof(CloScanByKey));
	if (!sbk) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	ccl_context_ref(ctx);
	sbk->ctx = ctx;
	sbk->key_type = key_type;
	sbk->value_type = value_type;
	sbk->sum_type = sum_type;
	sbk->op = opi;
	sbk->inclusive = inclusive;
	return sbk;
}

void clo_scan_by_key_destroy(CloScanByKey* sbk) {
	clo_return_if_fail(sbk != NULL);
	clo_devbuf_release(&sbk->workspace);
	clo_stream_guard_release(&sbk->guard);
	ccl_context_unref(sbk->ctx);
	free(sbk);
}

static int sbk_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
	if (!a || !b || !abytes || !bbytes) return 0;
	const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
	return a0 < b0 + bbytes && b0 < a0 + abytes;
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced. */
static const char* sbk_refusal(CloScanByKey* sbk, const void* keys_in, const void* values_in, const void* data_out, size_t numel) {
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!values_in && sbk->op != 0) return "min / max need values (without values every value is 1: only the sum, the rank in the run, is offered)";
	if (numel == 0) return NULL;
	if (!keys_in) return "keys_in is required";
	if (!data_out) return "data_out is required";
	const size_t kb = numel * clo_type_sizeof(sbk->key_type), vb = numel * clo_type_sizeof(sbk->value_type),
		sb = numel * clo_type_sizeof(sbk->sum_type);
	if (sbk_overlap(data_out, sb, keys_in, kb))
		return "data_out overlaps keys_in (the apply sweep reads the key to the left of its tile, which another work-group "
			"must not have overwritten)";
	if (sbk_overlap(data_out, sb, values_in, vb) && !(data_out == values_in && sb == vb))
		return "data_out overlaps values_in without being exactly it with a sum type as wide as the value type (in place "
			"works only where element i's result lands on element i's value)";
	return NULL;
}

CCLEvent* clo_scan_by_key_with_device_data(CloScanByKey* sbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* data_out, size_t numel, GError** err) {
	clo_return_val_if_fail(sbk != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	void* kin = keys_in ? ccl_buffer_get_device_ptr(keys_in) : NULL;
	void* vin = values_in ? ccl_buffer_get_device_ptr(values_in) : NULL;
	void* out = data_out ? ccl_buffer_get_device_ptr(data_out) : NULL;
	const char* why = sbk_refusal(sbk, kin, vin, out, numel);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t kb = numel * clo_type_sizeof(sbk->key_type), vb = numel * clo_type_sizeof(sbk->value_type),
		sb = numel * clo_type_sizeof(sbk->sum_type);
	if ((keys_in && kb > ccl_buffer_get_size(keys_in)) || (values_in && vb > ccl_buffer_get_size(values_in))
		|| (data_out && sb > ccl_buffer_get_size(data_out))) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) exceeds the size of the device buffers", numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SCAN BY KEY: %s %s, numel=%zu, key %s, values %s, sum %s%s", sbk->inclusive ? "inclusive" : "exclusive", sbk_ops[sbk->op], numel,
		clo_type_get_name(sbk->key_type), values_in ? clo_type_get_name(sbk->value_type) : "absent",
		clo_type_get_name(sbk->sum_type), (out && out == vin) ? ", in place" : "");

	if (numel > 0) {
		if (clo_hip_failed(clo_stream_guard_enter(&sbk->guard, cq_exec), err, "hipStreamWaitEvent")) return NULL;
		if (clo_hip_failed(clo_devbuf_reserve(&sbk->workspace, clo_hip_scan_by_key_workspace_bytes(numel)), err,
			"hipMalloc(scan-by-key workspace)")) return NULL;
	}
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SCAN_BY_KEY_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_scan_by_key(kin, vin, out, numel, (int) clo_type_sizeof(sbk->key_type),
		(int) sbk->value_type, (int) sbk->sum_type, sbk->op, sbk->inclusive, sbk->workspace.ptr, sbk->workspace.bytes,
		ccl_queue_get_stream(cq_exec));
	if (clo_hip_failed(st, err, "clo_hip_scan_by_key")) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	if (!ccl_queue_end_command(cq_exec, evt, err)) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	return evt;
}

cl_bool clo_scan_by_key_with_host_data(CloScanByKey* sbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* data_out, size_t numel, GError** err) {
	clo_return_val_if_fail(sbk != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = sbk_refusal(sbk, keys_in, values_in, data_out, numel);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	if (numel == 0) return CL_TRUE;

	cl_bool status = CL_FALSE;
	CCLBuffer* dev[3] = { NULL, NULL, NULL };   /* keys in, values in, out (the values' buffer itself when in place) */
	CCLQueue* intern_queue = NULL;
	CCLEvent* evt = NULL;
	CCLEventWaitList ewl = NULL;
	GError* err_internal = NULL;
	const size_t ks = clo_type_sizeof(sbk->key_type), vs = clo_type_sizeof(sbk->value_type), ss = clo_type_sizeof(sbk->sum_type);
	const int in_place = values_in != NULL && (const void*) data_out == values_in;
	const size_t bytes[3] = { numel * ks, numel * vs, numel * ss };
	const int used[3] = { 1, values_in != NULL, !in_place };
	CCLContext* ctx = sbk->ctx;

	if (cq_exec == NULL) {
		CCLDevice* d = ccl_context_get_device(ctx, 0, &err_internal);
		if (err_internal) goto error_handler;
		intern_queue = ccl_queue_new(ctx, d, 0, &err_internal);
		if (err_internal) goto error_handler;
		cq_exec = intern_queue;
	}
	if (cq_comm == NULL) cq_comm = cq_exec;
	for (int i = 0; i < 3; ++i) {
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
	evt = clo_scan_by_key_with_device_data(sbk, cq_exec, cq_comm, dev[0], dev[1], in_place ? dev[1] : dev[2], numel, &err_internal);
	if (err_internal) goto error_handler;
	ccl_buffer_enqueue_read(in_place ? dev[1] : dev[2], cq_comm, CL_TRUE, 0, bytes[2], data_out, evt ? ccl_ewl(&ewl, evt, NULL) : NULL, &err_internal);
	if (err_internal) goto error_handler;
	status = CL_TRUE;
	goto finish;

error_handler:
	clo_gerror_propagate(err, err_internal);
	status = CL_FALSE;

finish:
	ccl_event_wait_list_clear(&ewl);
	for (int i = 0; i < 3; ++i) if (dev[i]) ccl_buffer_destroy(dev[i]);
	if (intern_queue) ccl_queue_destroy(intern_queue);
	return status;
}

CCLContext* clo_scan_by_key_get_context(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, NULL);
	return sbk->ctx;
}

CloType clo_scan_by_key_get_key_type(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, (CloType) -1);
	return sbk->key_type;
}

size_t clo_scan_by_key_get_key_size(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, 0);
	return clo_type_sizeof(sbk->key_type);
}

CloType clo_scan_by_key_get_value_type(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, (CloType) -1);
	return sbk->value_type;
}

size_t clo_scan_by_key_get_value_size(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, 0);
	return clo_type_sizeof(sbk->value_type);
}

CloType clo_scan_by_key_get_sum_type(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, (CloType) -1);
	return sbk->sum_type;
}

size_t clo_scan_by_key_get_sum_size(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, 0);
	return clo_type_sizeof(sbk->sum_type);
}

const char* clo_scan_by_key_get_op(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, NULL);
	return sbk_ops[sbk->op];
}

cl_bool clo_scan_by_key_get_inclusive(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, CL_FALSE);
	return sbk->inclusive ? CL_TRUE : CL_FALSE;
}
