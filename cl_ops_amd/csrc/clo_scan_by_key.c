/*
 * clo_scan_by_key.c — CloScanByKey (include/clo_scan_by_key.h; not upstream): the running sum / min / max of every
 * element within its run of equal keys. The kernels are reached through the thin C-ABI (clo_hip_scan_by_key,
 * include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_scan_by_key.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SCAN_BY_KEY_EVENT "clo_scan_by_key"

struct clo_scan_by_key {
	clo_op_head head;        /* the workspace: the tile states */
	CloType key_type, value_type, sum_type;
	int op;                  /* index in sbk_ops: what clo_hip_scan_by_key takes */
	int inclusive;           /* 0 or 1 */
};

static const char* const sbk_ops[] = { "sum", "min", "max" };

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
	const int opi = clo_name_index(op, sbk_ops, 3);
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
	if (!clo_type_is_int32_or_64(value_type) || !clo_type_is_int32_or_64(sum_type)) {
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
	CloScanByKey* sbk = (CloScanByKey*) clo_op_new(sizeof(CloScanByKey), ctx, err);
	if (!sbk) return NULL;
	sbk->key_type = key_type;
	sbk->value_type = value_type;
	sbk->sum_type = sum_type;
	sbk->op = opi;
	sbk->inclusive = inclusive;
	return sbk;
}

void clo_scan_by_key_destroy(CloScanByKey* sbk) {
	clo_return_if_fail(sbk != NULL);
	clo_op_destroy(sbk);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced. */
static const char* sbk_refusal(CloScanByKey* sbk, const void* keys_in, const void* values_in, const void* data_out, size_t numel) {
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!values_in && sbk->op != 0) return "min / max need values (without values every value is 1: only the sum, the rank in the run, is offered)";
	if (numel == 0) return NULL;
	if (!keys_in) return "keys_in is required";
	if (!data_out) return "data_out is required";
	const clo_range keys = { keys_in, numel * clo_type_sizeof(sbk->key_type) }, values = { values_in, numel * clo_type_sizeof(sbk->value_type) },
		out = { data_out, numel * clo_type_sizeof(sbk->sum_type) };
	if (clo_ranges_overlap(out, keys))
		return "data_out overlaps keys_in (the apply sweep reads the key to the left of its tile, which another work-group "
			"must not have overwritten)";
	if (clo_ranges_overlap(out, values) && !(data_out == values_in && out.bytes == values.bytes))
		return "data_out overlaps values_in without being exactly it with a sum type as wide as the value type (in place "
			"works only where element i's result lands on element i's value)";
	return NULL;
}

CCLEvent* clo_scan_by_key_with_device_data(CloScanByKey* sbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* data_out, size_t numel, GError** err) {
	clo_return_val_if_fail(sbk != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[3] = { keys_in, values_in, data_out };
	void* p[3];
	clo_buffers_device_ptrs(buf, p, 3);
	const char* why = sbk_refusal(sbk, p[0], p[1], p[2], numel);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t need[3] = { numel * clo_type_sizeof(sbk->key_type), numel * clo_type_sizeof(sbk->value_type), numel * clo_type_sizeof(sbk->sum_type) };
	if (!clo_buffers_hold(buf, need, 3)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) exceeds the size of the device buffers", numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SCAN BY KEY: %s %s, numel=%zu, key %s, values %s, sum %s%s", sbk->inclusive ? "inclusive" : "exclusive", sbk_ops[sbk->op], numel,
		clo_type_get_name(sbk->key_type), values_in ? clo_type_get_name(sbk->value_type) : "absent",
		clo_type_get_name(sbk->sum_type), (p[2] && p[2] == p[1]) ? ", in place" : "");

	if (numel > 0 && !clo_op_reserve(&sbk->head, cq_exec, clo_hip_scan_by_key_workspace_bytes(numel), "hipMalloc(scan-by-key workspace)", err))
		return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SCAN_BY_KEY_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_scan_by_key(p[0], p[1], p[2], numel, (int) clo_type_sizeof(sbk->key_type),
		(int) sbk->value_type, (int) sbk->sum_type, sbk->op, sbk->inclusive, sbk->head.workspace.ptr, sbk->head.workspace.bytes,
		ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_scan_by_key", err);
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

	const size_t ks = clo_type_sizeof(sbk->key_type), vs = clo_type_sizeof(sbk->value_type), ss = clo_type_sizeof(sbk->sum_type);
	/* keys in, values in, out: in place the values' buffer itself, and no third one */
	const int out = values_in != NULL && (const void*) data_out == values_in ? 1 : 2;
	clo_stage st;
	clo_stage_open(&st, sbk->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, keys_in, numel * ks);
	clo_stage_in(&st, 1, values_in, numel * vs);
	if (out == 2) clo_stage_out(&st, 2, data_out, numel * ss);
	if (clo_stage_ok(&st))
		st.evt = clo_scan_by_key_with_device_data(sbk, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[out], numel, &st.err);
	clo_stage_read(&st, out, data_out, numel * ss);
	return clo_stage_close(&st, err);
}

CCLContext* clo_scan_by_key_get_context(CloScanByKey* sbk) {
	clo_return_val_if_fail(sbk != NULL, NULL);
	return sbk->head.ctx;
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
