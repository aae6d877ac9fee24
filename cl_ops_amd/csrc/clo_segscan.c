/*
 * clo_segscan.c — CloSegScan (include/clo_segscan.h; not upstream): the running sum, minimum or maximum of every row
 * within its segment, the segments given by counts or by CSR offsets. The kernels are reached through the thin C-ABI
 * (clo_hip_segscan, include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_segscan.h"

#include <stdint.h>
#include <string.h>

#include "clo_scan_by_key.h"
#include "clo_internal.h"

#define CLO_SEGSCAN_EVENT "clo_segscan"

struct clo_segscan {
	clo_op_head head;        /* the workspace: the segment ends, the tiles' splits and states (clo_hip_segscan_workspace_bytes) */
	int op;                  /* index in segscan_ops: what clo_hip_segscan takes */
	int form;                /* index in segscan_forms: likewise */
	int inclusive;           /* 0 or 1 */
	CloType value_type, sum_type, count_type;
};

static const char* const segscan_ops[] = { "sum", "min", "max" };
static const char* const segscan_forms[] = { "counts", "offsets" };

/* the one option there is, scan by key's: inclusive=0 | inclusive=1 */
static int segscan_option(const char* key, const char* value, const char* token, void* user, GError** err) {
	if (strcmp(key, "inclusive") == 0 && (strcmp(value, "0") == 0 || strcmp(value, "1") == 0)) {
		*(int*) user = value[0] == '1';
		return 1;
	}
	clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a segmented scan: '%s' (inclusive=0 or inclusive=1).", token);
	return 0;
}

CloSegScan* clo_segscan_new(const char* op, const char* form, const char* options, CCLContext* ctx,
	CloType value_type, CloType sum_type, CloType count_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int opi = clo_name_index(op, segscan_ops, 3);
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segmented scan '%s' (one of: " CLO_SCAN_BY_KEY_OPS ").", op ? op : "(null)");
		return NULL;
	}
	const int formi = clo_name_index(form, segscan_forms, 2);
	if (formi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segment form '%s' (one of: " CLO_SEGSCAN_FORMS ").", form ? form : "(null)");
		return NULL;
	}
	int inclusive = 0;
	GError* err_opt = NULL;
	if (!clo_parse_options(options, segscan_option, &inclusive, "segmented-scan", &err_opt)) {
		/* (an option without '=' comes back with the parser's own wording, which names a sort) */
		if (err_opt) clo_gerror_free(err_opt);
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a segmented scan: '%s' (inclusive=0 or inclusive=1).", options);
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_segscan_new needs a context.");
		return NULL;
	}
	if (!clo_type_is_int32_or_64(value_type) || !clo_type_is_int32_or_64(sum_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A segmented scan takes values and sums of type int, uint, long or ulong "
			"(floating-point aggregates depend on the order of addition; narrower values are not built), not '%s' into '%s'.",
			clo_type_get_name(value_type) ? clo_type_get_name(value_type) : "?", clo_type_get_name(sum_type) ? clo_type_get_name(sum_type) : "?");
		return NULL;
	}
	if (clo_type_sizeof(sum_type) < clo_type_sizeof(value_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The sum type '%s' is narrower than the value type '%s'.",
			clo_type_get_name(sum_type), clo_type_get_name(value_type));
		return NULL;
	}
	if (count_type != CLO_UINT && count_type != CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The count_type of a segmented scan is uint or ulong, not type %d.", (int) count_type);
		return NULL;
	}
	CloSegScan* ss = (CloSegScan*) clo_op_new(sizeof(CloSegScan), ctx, err);
	if (!ss) return NULL;
	ss->op = opi;
	ss->form = formi;
	ss->inclusive = inclusive;
	ss->value_type = value_type;
	ss->sum_type = sum_type;
	ss->count_type = count_type;
	return ss;
}

void clo_segscan_destroy(CloSegScan* ss) {
	clo_return_if_fail(ss != NULL);
	clo_op_destroy(ss);
}

/* the bytes counts_or_offsets holds: numel_seg counts, or numel_seg + 1 offsets */
static size_t segscan_src_bytes(const CloSegScan* ss, size_t numel_seg) {
	return (numel_seg + (ss->form == CLO_HIP_SEGSCAN_OFFSETS ? 1 : 0)) * clo_type_sizeof(ss->count_type);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * word_bytes: the size of what num_in and num_out point to (a cl_ulong of the device, a size_t of the host). */
static const char* segscan_refusal(CloSegScan* ss, const void* src, const void* num_in, const void* values_in,
	const void* data_out, const void* num_out, size_t numel_seg, size_t numel, size_t word_bytes) {
	if (numel_seg > 0xffffffffull) return "numel_seg must be below 2^32";
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!num_out) return "num_out is required";
	if (!src && (numel_seg > 0 || ss->form == CLO_HIP_SEGSCAN_OFFSETS))
		return ss->form == CLO_HIP_SEGSCAN_OFFSETS ? "counts_or_offsets is required: the offsets" : "counts_or_offsets is required: the counts";
	if (!values_in && numel > 0) return "values_in is required (values absent as ones is not offered: clo_expand's rank_out is that result)";
	if (!data_out && numel > 0) return "data_out is required";
	const clo_range values = { values_in, numel * clo_type_sizeof(ss->value_type) }, data = { data_out, numel * clo_type_sizeof(ss->sum_type) };
	/* in place: element i's result lands on element i's value, which the group that writes it has read before */
	const int in_place = data_out != NULL && data_out == values_in && data.bytes == values.bytes;
	const clo_range in[3] = { { src, segscan_src_bytes(ss, numel_seg) }, { num_in, word_bytes }, { values_in, in_place ? 0 : values.bytes } };
	const clo_range out[2] = { data, { num_out, word_bytes } };
	switch (clo_ranges_conflict(in, 3, out, 2)) {
		case CLO_RANGES_OUT_IN: return "an output range (data_out or num_out) overlaps an input range (data_out may only be exactly values_in, with a "
			"sum type as wide as the value type)";
		case CLO_RANGES_OUT_OUT: return "data_out and num_out overlap";
	}
	return NULL;
}

CCLEvent* clo_segscan_with_device_data(CloSegScan* ss, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* data_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(ss != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[5] = { counts_or_offsets, num_in, values_in, data_out, num_out };
	void* p[5];
	clo_buffers_device_ptrs(buf, p, 5);
	const char* why = segscan_refusal(ss, p[0], p[1], p[2], p[3], p[4], numel_seg, numel, sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[4] & 7u)) why = "num_out must be 8-byte aligned";
	if (!why && ((uintptr_t) p[1] & 7u)) why = "num_in must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t cs = clo_type_sizeof(ss->count_type);
	const size_t need[5] = { segscan_src_bytes(ss, numel_seg), sizeof(cl_ulong), numel * clo_type_sizeof(ss->value_type),
		numel * clo_type_sizeof(ss->sum_type), sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 5)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_seg (%zu) or numel (%zu) exceeds the size of the device buffers (counts_or_offsets "
			"holds numel_seg counts or numel_seg + 1 offsets, values_in and data_out numel rows, num_in and num_out 8 bytes)",
			numel_seg, numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SEGSCAN: %s %s, %s, %zu segments of type %s, %zu rows of %s into %s%s", ss->inclusive ? "inclusive" : "exclusive", segscan_ops[ss->op],
		segscan_forms[ss->form], numel_seg, clo_type_get_name(ss->count_type), numel, clo_type_get_name(ss->value_type),
		clo_type_get_name(ss->sum_type), (p[3] && p[3] == p[2]) ? ", in place" : "");

	const size_t ws = clo_hip_segscan_workspace_bytes(numel_seg, numel);
	if (ws > 0 && !clo_op_reserve(&ss->head, cq_exec, ws, "hipMalloc(segscan workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SEGSCAN_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_segscan(ss->op, ss->inclusive, ss->form, p[0], (int) cs, (const uint64_t*) p[1], p[2], p[3], (uint64_t*) p[4], numel_seg, numel,
		(int) ss->value_type, (int) ss->sum_type, ss->head.workspace.ptr, ss->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_segscan", err);
}

cl_bool clo_segscan_with_host_data(CloSegScan* ss, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	void* data_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(ss != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = segscan_refusal(ss, counts_or_offsets, num_in, values_in, data_out, num_out, numel_seg, numel, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const cl_ulong m_in = num_in ? (cl_ulong) *num_in : 0;
	*num_out = 0;
	if (numel_seg == 0 || (num_in && m_in == 0)) return CL_TRUE;   /* m == 0: no segments, no device needed */

	const size_t vs = clo_type_sizeof(ss->value_type), sums = clo_type_sizeof(ss->sum_type);
	/* src, num_in, values in, out, num_out: in place the values' buffer itself, and no fourth one */
	const int out = values_in != NULL && (const void*) data_out == values_in ? 2 : 3;
	cl_ulong total = 0;
	clo_stage st;
	clo_stage_open(&st, ss->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, counts_or_offsets, segscan_src_bytes(ss, numel_seg));
	clo_stage_in(&st, 1, num_in ? &m_in : NULL, sizeof(cl_ulong));
	clo_stage_in(&st, 2, values_in, numel * vs);
	if (out == 3) clo_stage_out(&st, 3, data_out, numel * sums);
	clo_stage_out(&st, 4, num_out, sizeof(cl_ulong));
	if (clo_stage_ok(&st))
		st.evt = clo_segscan_with_device_data(ss, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[out], st.dev[4],
			numel_seg, numel, &st.err);
	clo_stage_read(&st, 4, &total, sizeof(cl_ulong));
	if (clo_stage_ok(&st)) {
		const size_t rows = total < numel ? (size_t) total : numel;   /* the rows of data_out that are written */
		if (rows > 0) clo_stage_read(&st, out, data_out, rows * sums);
	}
	if (clo_stage_ok(&st)) *num_out = (size_t) total;
	return clo_stage_close(&st, err);
}

CCLContext* clo_segscan_get_context(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, NULL);
	return ss->head.ctx;
}

const char* clo_segscan_get_op(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, NULL);
	return segscan_ops[ss->op];
}

const char* clo_segscan_get_form(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, NULL);
	return segscan_forms[ss->form];
}

cl_bool clo_segscan_get_inclusive(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, CL_FALSE);
	return ss->inclusive ? CL_TRUE : CL_FALSE;
}

CloType clo_segscan_get_value_type(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, (CloType) -1);
	return ss->value_type;
}

size_t clo_segscan_get_value_size(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, 0);
	return clo_type_sizeof(ss->value_type);
}

CloType clo_segscan_get_sum_type(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, (CloType) -1);
	return ss->sum_type;
}

size_t clo_segscan_get_sum_size(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, 0);
	return clo_type_sizeof(ss->sum_type);
}

CloType clo_segscan_get_count_type(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, (CloType) -1);
	return ss->count_type;
}

size_t clo_segscan_get_count_size(CloSegScan* ss) {
	clo_return_val_if_fail(ss != NULL, 0);
	return clo_type_sizeof(ss->count_type);
}
