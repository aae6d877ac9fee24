/*
 * clo_select.c — CloSelect (include/clo_select.h; not upstream): stable selection and partition by flags or by
 * comparison with a threshold, with values or as indices. The kernels are reached through the thin C-ABI
 * (clo_hip_select, include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_select.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SELECT_EVENT "clo_select"

struct clo_select {
	clo_op_head head;        /* the workspace: the tiles' kept counts (clo_hip_select_workspace_bytes) */
	int op;                  /* index in select_ops: what clo_hip_select takes */
	int pred;                /* index in select_preds, likewise */
	CloType key_type;
	size_t value_size;
};

static const char* const select_ops[] = { "select", "partition" };
static const char* const select_preds[] = { "flagged", "lt", "le", "gt", "ge", "eq", "ne" };

CloSelect* clo_select_new(const char* op, const char* pred, const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int opi = clo_name_index(op, select_ops, 2), predi = clo_name_index(pred, select_preds, 7);
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown selection op '%s' (one of: " CLO_SELECT_OPS ").", op ? op : "(null)");
		return NULL;
	}
	if (predi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown selection pred '%s' (one of: " CLO_SELECT_PREDS ").", pred ? pred : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a selection (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_select_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for a selection.", (int) key_type);
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A selection carries values of 0 (none), 4 or 8 bytes, not a value_size of %zu.", value_size);
		return NULL;
	}
	CloSelect* sel = (CloSelect*) clo_op_new(sizeof(CloSelect), ctx, err);
	if (!sel) return NULL;
	sel->op = opi;
	sel->pred = predi;
	sel->key_type = key_type;
	sel->value_size = value_size;
	return sel;
}

void clo_select_destroy(CloSelect* sel) {
	clo_return_if_fail(sel != NULL);
	clo_op_destroy(sel);
}

/* the bytes flags_or_threshold holds: numel flags, or one key */
static size_t select_fot_bytes(const CloSelect* sel, size_t numel) {
	return sel->pred == CLO_HIP_SELECT_FLAGGED ? numel : clo_type_sizeof(sel->key_type);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * count_bytes: the size of what num_out points to (a cl_ulong of the device, a size_t of the host). */
static const char* select_refusal(CloSelect* sel, const void* keys_in, const void* values_in, const void* fot,
	const void* keys_out, const void* values_out, const void* num_out, size_t numel, size_t count_bytes) {
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!num_out) return "num_out is required";
	if (!fot && (numel > 0 || sel->pred != CLO_HIP_SELECT_FLAGGED)) return sel->pred == CLO_HIP_SELECT_FLAGGED ? "flags_or_threshold is required: the flags" : "flags_or_threshold is required: the threshold";
	if (!keys_out && !values_out) return "keys_out and values_out are both NULL";
	if (sel->value_size == 0 && (values_in || values_out)) return "values passed to a selection made with value_size 0";
	if (sel->value_size > 0 && !values_out) return "values_out is required with a value_size above 0";
	if (sel->value_size == 8 && !values_in) return "NULL values_in (the arg form) needs a value_size of 4: the indices are written as uint";
	if (numel > 0 && !keys_in && (sel->pred != CLO_HIP_SELECT_FLAGGED || keys_out))
		return "keys_in is required (only a flagged selection that writes indices alone reads no keys)";
	const size_t ks = clo_type_sizeof(sel->key_type), vs = sel->value_size;
	const clo_range in[3] = { { keys_in, numel * ks }, { values_in, numel * vs }, { fot, select_fot_bytes(sel, numel) } };
	/* the outputs are sized by numel rows, whatever k turns out to be */
	const clo_range out[3] = { { keys_out, numel * ks }, { values_out, numel * vs }, { num_out, count_bytes } };
	switch (clo_ranges_conflict(in, 3, out, 3)) {
		case CLO_RANGES_OUT_IN: return "an output range overlaps an input range (there is no in-place selection)";
		case CLO_RANGES_OUT_OUT: return "two output ranges overlap";
	}
	return NULL;
}

CCLEvent* clo_select_with_device_data(CloSelect* sel, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* flags_or_threshold,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* num_out, size_t numel, GError** err) {
	clo_return_val_if_fail(sel != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[6] = { keys_in, values_in, flags_or_threshold, keys_out, values_out, num_out };
	void* p[6];
	clo_buffers_device_ptrs(buf, p, 6);
	const char* why = select_refusal(sel, p[0], p[1], p[2], p[3], p[4], p[5], numel, sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[5] & 7u)) why = "num_out must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(sel->key_type), vs = sel->value_size;
	const size_t need[6] = { numel * ks, numel * vs, select_fot_bytes(sel, numel), numel * ks, numel * vs, sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 6)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) exceeds the size of the device buffers (the inputs and the outputs "
			"hold numel rows, the flags numel bytes, the threshold one key, num_out 8 bytes)", numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SELECT: %s %s of %zu keys of type %s, %s", select_ops[sel->op], select_preds[sel->pred], numel, clo_type_get_name(sel->key_type),
		vs == 0 ? "no values" : !p[1] ? "indices" : vs == 4 ? "4-byte values" : "8-byte values");

	const size_t ws = clo_hip_select_workspace_bytes(numel, (int) ks, (int) vs);
	if (ws > 0 && !clo_op_reserve(&sel->head, cq_exec, ws, "hipMalloc(select workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SELECT_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_select(sel->op, sel->pred, p[0], p[1], p[2], p[3], p[4], (uint64_t*) p[5], numel,
		(int) ks, clo_type_key_kind(sel->key_type), (int) vs, sel->head.workspace.ptr, sel->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_select", err);
}

cl_bool clo_select_with_host_data(CloSelect* sel, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, const void* flags_or_threshold,
	void* keys_out, void* values_out, size_t numel, size_t* num_out, GError** err) {
	clo_return_val_if_fail(sel != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = select_refusal(sel, keys_in, values_in, flags_or_threshold, keys_out, values_out, num_out, numel, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	*num_out = 0;
	if (numel == 0) return CL_TRUE;   /* nothing can be kept: no device needed */

	const size_t ks = clo_type_sizeof(sel->key_type), vs = sel->value_size;
	/* keys, values, the flags or the threshold, keys out, values out, the count */
	const void* const host[6] = { keys_in, values_in, flags_or_threshold, keys_out, values_out, num_out };
	const size_t bytes[6] = { numel * ks, numel * vs, select_fot_bytes(sel, numel), numel * ks, numel * vs, sizeof(cl_ulong) };
	cl_ulong k = 0;
	clo_stage st;
	clo_stage_open(&st, sel->head.ctx, cq_exec, cq_comm);
	for (int i = 0; i < 3; ++i) clo_stage_in(&st, i, host[i], bytes[i]);
	for (int i = 3; i < 6; ++i) clo_stage_out(&st, i, host[i], bytes[i]);
	if (clo_stage_ok(&st))
		st.evt = clo_select_with_device_data(sel, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4], st.dev[5], numel, &st.err);
	/* the count first (blocking): it says how many rows of a select there are to copy */
	clo_stage_read(&st, 5, &k, sizeof(cl_ulong));
	if (clo_stage_ok(&st) && k > numel)
		clo_gerror_set(&st.err, CLO_ERROR, CLO_ERROR_LIBRARY, "selection: %llu rows kept of %zu", (unsigned long long) k, numel);
	const size_t rows = sel->op == CLO_HIP_SELECT_PARTITION ? numel : (size_t) k;
	clo_stage_read(&st, 3, keys_out, rows * ks);
	clo_stage_read(&st, 4, values_out, rows * vs);
	if (clo_stage_ok(&st)) *num_out = (size_t) k;
	return clo_stage_close(&st, err);
}

CCLContext* clo_select_get_context(CloSelect* sel) {
	clo_return_val_if_fail(sel != NULL, NULL);
	return sel->head.ctx;
}

CloType clo_select_get_key_type(CloSelect* sel) {
	clo_return_val_if_fail(sel != NULL, (CloType) -1);
	return sel->key_type;
}

size_t clo_select_get_key_size(CloSelect* sel) {
	clo_return_val_if_fail(sel != NULL, 0);
	return clo_type_sizeof(sel->key_type);
}

size_t clo_select_get_value_size(CloSelect* sel) {
	clo_return_val_if_fail(sel != NULL, 0);
	return sel->value_size;
}

const char* clo_select_get_op(CloSelect* sel) {
	clo_return_val_if_fail(sel != NULL, NULL);
	return select_ops[sel->op];
}

const char* clo_select_get_pred(CloSelect* sel) {
	clo_return_val_if_fail(sel != NULL, NULL);
	return select_preds[sel->pred];
}
