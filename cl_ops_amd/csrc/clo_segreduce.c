/*
 * clo_segreduce.c — CloSegReduce (include/clo_segreduce.h; not upstream): the sum, minimum or maximum of every segment,
 * the segments given by counts or by CSR offsets. The kernels are reached through the thin C-ABI (clo_hip_segreduce,
 * include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_segreduce.h"

#include <stdint.h>
#include <string.h>

#include "clo_reduce.h"
#include "clo_internal.h"

#define CLO_SEGREDUCE_EVENT "clo_segreduce"

struct clo_segreduce {
	clo_op_head head;        /* the workspace: the segment ends, the tiles' splits and states (clo_hip_segreduce_workspace_bytes) */
	int op;                  /* index in segreduce_ops: what clo_hip_segreduce takes */
	int form;                /* index in segreduce_forms: likewise */
	CloType value_type, sum_type, count_type;
};

static const char* const segreduce_ops[] = { "sum", "min", "max" };
static const char* const segreduce_forms[] = { "counts", "offsets" };

CloSegReduce* clo_segreduce_new(const char* op, const char* form, const char* options, CCLContext* ctx,
	CloType value_type, CloType sum_type, CloType count_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int opi = clo_name_index(op, segreduce_ops, 3);
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segmented reduction '%s' (one of: " CLO_REDUCE_BY_KEY_OPS ").", op ? op : "(null)");
		return NULL;
	}
	const int formi = clo_name_index(form, segreduce_forms, 2);
	if (formi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segment form '%s' (one of: " CLO_SEGREDUCE_FORMS ").", form ? form : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a segmented reduction (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_segreduce_new needs a context.");
		return NULL;
	}
	if (!clo_type_is_int32_or_64(value_type) || !clo_type_is_int32_or_64(sum_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A segmented reduction takes values and sums of type int, uint, long or ulong "
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
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The count_type of a segmented reduction is uint or ulong, not type %d.", (int) count_type);
		return NULL;
	}
	CloSegReduce* sr = (CloSegReduce*) clo_op_new(sizeof(CloSegReduce), ctx, err);
	if (!sr) return NULL;
	sr->op = opi;
	sr->form = formi;
	sr->value_type = value_type;
	sr->sum_type = sum_type;
	sr->count_type = count_type;
	return sr;
}

void clo_segreduce_destroy(CloSegReduce* sr) {
	clo_return_if_fail(sr != NULL);
	clo_op_destroy(sr);
}

/* the bytes counts_or_offsets holds: numel_seg counts, or numel_seg + 1 offsets */
static size_t segreduce_src_bytes(const CloSegReduce* sr, size_t numel_seg) {
	return (numel_seg + (sr->form == CLO_HIP_SEGREDUCE_OFFSETS ? 1 : 0)) * clo_type_sizeof(sr->count_type);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * word_bytes: the size of what num_in and num_out point to (a cl_ulong of the device, a size_t of the host). */
static const char* segreduce_refusal(CloSegReduce* sr, const void* src, const void* num_in, const void* values_in,
	const void* aggr_out, const void* num_out, size_t numel_seg, size_t numel, size_t word_bytes) {
	if (numel_seg > 0xffffffffull) return "numel_seg must be below 2^32";
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!num_out) return "num_out is required";
	if (!src && (numel_seg > 0 || sr->form == CLO_HIP_SEGREDUCE_OFFSETS))
		return sr->form == CLO_HIP_SEGREDUCE_OFFSETS ? "counts_or_offsets is required: the offsets" : "counts_or_offsets is required: the counts";
	if (!values_in && numel > 0) return "values_in is required";
	if (!aggr_out && numel_seg > 0) return "aggr_out is required";
	const clo_range in[3] = { { src, segreduce_src_bytes(sr, numel_seg) }, { num_in, word_bytes }, { values_in, numel * clo_type_sizeof(sr->value_type) } };
	/* aggr_out is sized by numel_seg rows, however many segments *num_in leaves */
	const clo_range out[2] = { { aggr_out, numel_seg * clo_type_sizeof(sr->sum_type) }, { num_out, word_bytes } };
	switch (clo_ranges_conflict(in, 3, out, 2)) {
		case CLO_RANGES_OUT_IN: return "an output range (aggr_out or num_out) overlaps an input range";
		case CLO_RANGES_OUT_OUT: return "aggr_out and num_out overlap";
	}
	return NULL;
}

CCLEvent* clo_segreduce_with_device_data(CloSegReduce* sr, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* aggr_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(sr != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[5] = { counts_or_offsets, num_in, values_in, aggr_out, num_out };
	void* p[5];
	clo_buffers_device_ptrs(buf, p, 5);
	const char* why = segreduce_refusal(sr, p[0], p[1], p[2], p[3], p[4], numel_seg, numel, sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[4] & 7u)) why = "num_out must be 8-byte aligned";
	if (!why && ((uintptr_t) p[1] & 7u)) why = "num_in must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t cs = clo_type_sizeof(sr->count_type);
	const size_t need[5] = { segreduce_src_bytes(sr, numel_seg), sizeof(cl_ulong), numel * clo_type_sizeof(sr->value_type),
		numel_seg * clo_type_sizeof(sr->sum_type), sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 5)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_seg (%zu) or numel (%zu) exceeds the size of the device buffers (counts_or_offsets "
			"holds numel_seg counts or numel_seg + 1 offsets, values_in numel rows, aggr_out numel_seg rows, num_in and num_out 8 bytes)",
			numel_seg, numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SEGREDUCE: %s, %s, %zu segments of type %s, %zu rows of %s into %s", segreduce_ops[sr->op], segreduce_forms[sr->form], numel_seg,
		clo_type_get_name(sr->count_type), numel, clo_type_get_name(sr->value_type), clo_type_get_name(sr->sum_type));

	const size_t ws = clo_hip_segreduce_workspace_bytes(numel_seg, numel);
	if (ws > 0 && !clo_op_reserve(&sr->head, cq_exec, ws, "hipMalloc(segreduce workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SEGREDUCE_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_segreduce(sr->op, sr->form, p[0], (int) cs, (const uint64_t*) p[1], p[2], p[3], (uint64_t*) p[4], numel_seg, numel,
		(int) sr->value_type, (int) sr->sum_type, sr->head.workspace.ptr, sr->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_segreduce", err);
}

cl_bool clo_segreduce_with_host_data(CloSegReduce* sr, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	void* aggr_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(sr != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = segreduce_refusal(sr, counts_or_offsets, num_in, values_in, aggr_out, num_out, numel_seg, numel, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const cl_ulong m_in = num_in ? (cl_ulong) *num_in : 0;
	*num_out = 0;
	if (numel_seg == 0 || (num_in && m_in == 0)) return CL_TRUE;   /* m == 0: no segments, no device needed */

	const size_t m = num_in && m_in < numel_seg ? (size_t) m_in : numel_seg;   /* the rows of aggr_out that are written */
	const size_t ss = clo_type_sizeof(sr->sum_type);
	cl_ulong total = 0;
	clo_stage st;
	clo_stage_open(&st, sr->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, counts_or_offsets, segreduce_src_bytes(sr, numel_seg));
	clo_stage_in(&st, 1, num_in ? &m_in : NULL, sizeof(cl_ulong));
	clo_stage_in(&st, 2, values_in, numel * clo_type_sizeof(sr->value_type));
	clo_stage_out(&st, 3, aggr_out, numel_seg * ss);
	clo_stage_out(&st, 4, num_out, sizeof(cl_ulong));
	if (clo_stage_ok(&st))
		st.evt = clo_segreduce_with_device_data(sr, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4],
			numel_seg, numel, &st.err);
	clo_stage_read(&st, 4, &total, sizeof(cl_ulong));
	clo_stage_read(&st, 3, aggr_out, m * ss);
	if (clo_stage_ok(&st)) *num_out = (size_t) total;
	return clo_stage_close(&st, err);
}

CCLContext* clo_segreduce_get_context(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, NULL);
	return sr->head.ctx;
}

const char* clo_segreduce_get_op(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, NULL);
	return segreduce_ops[sr->op];
}

const char* clo_segreduce_get_form(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, NULL);
	return segreduce_forms[sr->form];
}

CloType clo_segreduce_get_value_type(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, (CloType) -1);
	return sr->value_type;
}

size_t clo_segreduce_get_value_size(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, 0);
	return clo_type_sizeof(sr->value_type);
}

CloType clo_segreduce_get_sum_type(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, (CloType) -1);
	return sr->sum_type;
}

size_t clo_segreduce_get_sum_size(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, 0);
	return clo_type_sizeof(sr->sum_type);
}

CloType clo_segreduce_get_count_type(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, (CloType) -1);
	return sr->count_type;
}

size_t clo_segreduce_get_count_size(CloSegReduce* sr) {
	clo_return_val_if_fail(sr != NULL, 0);
	return clo_type_sizeof(sr->count_type);
}
