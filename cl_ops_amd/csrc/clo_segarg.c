/*
 * clo_segarg.c — CloSegArg (include/clo_segarg.h; not upstream): where the minimum or maximum of every segment lies, and
 * its value, the segments given by counts or by CSR offsets. The kernels are reached through the thin C-ABI
 * (clo_hip_segarg, include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_segarg.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SEGARG_EVENT "clo_segarg"

struct clo_segarg {
	clo_op_head head;        /* the workspace: the segment ends, the tiles' splits and states (clo_hip_segarg_workspace_bytes) */
	int op;                  /* index in segarg_ops: what clo_hip_segarg takes */
	int tie;                 /* index in segarg_ties: likewise */
	int form;                /* index in segarg_forms: likewise */
	CloType value_type, count_type;
};

static const char* const segarg_ops[] = { "argmin", "argmax" };
static const char* const segarg_ties[] = { "first", "last" };
static const char* const segarg_forms[] = { "counts", "offsets" };

static int segarg_value_type_built(CloType t) {
	return t == CLO_INT || t == CLO_UINT || t == CLO_LONG || t == CLO_ULONG || t == CLO_FLOAT || t == CLO_DOUBLE;
}

CloSegArg* clo_segarg_new(const char* op, const char* tie, const char* form, const char* options, CCLContext* ctx,
	CloType value_type, CloType count_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int opi = clo_name_index(op, segarg_ops, 2);
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segmented arg operation '%s' (one of: " CLO_SEGARG_OPS ").", op ? op : "(null)");
		return NULL;
	}
	const int tiei = clo_name_index(tie, segarg_ties, 2);
	if (tiei < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown tie rule '%s' (one of: " CLO_SEGARG_TIES ").", tie ? tie : "(null)");
		return NULL;
	}
	const int formi = clo_name_index(form, segarg_forms, 2);
	if (formi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segment form '%s' (one of: " CLO_SEGREDUCE_FORMS ").", form ? form : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a segmented arg-min or arg-max (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_segarg_new needs a context.");
		return NULL;
	}
	if (!segarg_value_type_built(value_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A segmented arg-min or arg-max takes values of type int, uint, long, ulong, float or double "
			"(narrower values are not built), not '%s'.", clo_type_get_name(value_type) ? clo_type_get_name(value_type) : "?");
		return NULL;
	}
	if (count_type != CLO_UINT && count_type != CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The count_type of a segmented arg-min or arg-max is uint or ulong, not type %d.", (int) count_type);
		return NULL;
	}
	CloSegArg* sa = (CloSegArg*) clo_op_new(sizeof(CloSegArg), ctx, err);
	if (!sa) return NULL;
	sa->op = opi;
	sa->tie = tiei;
	sa->form = formi;
	sa->value_type = value_type;
	sa->count_type = count_type;
	return sa;
}

void clo_segarg_destroy(CloSegArg* sa) {
	clo_return_if_fail(sa != NULL);
	clo_op_destroy(sa);
}

/* the bytes counts_or_offsets holds: numel_seg counts, or numel_seg + 1 offsets */
static size_t segarg_src_bytes(const CloSegArg* sa, size_t numel_seg) {
	return (numel_seg + (sa->form == CLO_HIP_SEGARG_OFFSETS ? 1 : 0)) * clo_type_sizeof(sa->count_type);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * word_bytes: the size of what num_in and num_out point to (a cl_ulong of the device, a size_t of the host). */
static const char* segarg_refusal(CloSegArg* sa, const void* src, const void* num_in, const void* values_in,
	const void* idx_out, const void* val_out, const void* num_out, size_t numel_seg, size_t numel, size_t word_bytes) {
	if (numel_seg > 0xffffffffull) return "numel_seg must be below 2^32";
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!num_out) return "num_out is required";
	if (!src && (numel_seg > 0 || sa->form == CLO_HIP_SEGARG_OFFSETS))
		return sa->form == CLO_HIP_SEGARG_OFFSETS ? "counts_or_offsets is required: the offsets" : "counts_or_offsets is required: the counts";
	if (!values_in && numel > 0) return "values_in is required";
	if (!idx_out && numel_seg > 0) return "idx_out is required";
	const size_t vs = clo_type_sizeof(sa->value_type);
	const clo_range in[3] = { { src, segarg_src_bytes(sa, numel_seg) }, { num_in, word_bytes }, { values_in, numel * vs } };
	/* idx_out and val_out are sized by numel_seg rows, however many segments *num_in leaves */
	const clo_range out[3] = { { idx_out, numel_seg * sizeof(cl_uint) }, { val_out, numel_seg * vs }, { num_out, word_bytes } };
	switch (clo_ranges_conflict(in, 3, out, 3)) {
		case CLO_RANGES_OUT_IN: return "an output range (idx_out, val_out or num_out) overlaps an input range";
		case CLO_RANGES_OUT_OUT: return "two of idx_out, val_out and num_out overlap";
	}
	return NULL;
}

CCLEvent* clo_segarg_with_device_data(CloSegArg* sa, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* idx_out, CCLBuffer* val_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(sa != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[6] = { counts_or_offsets, num_in, values_in, idx_out, val_out, num_out };
	void* p[6];
	clo_buffers_device_ptrs(buf, p, 6);
	const char* why = segarg_refusal(sa, p[0], p[1], p[2], p[3], p[4], p[5], numel_seg, numel, sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[5] & 7u)) why = "num_out must be 8-byte aligned";
	if (!why && ((uintptr_t) p[1] & 7u)) why = "num_in must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t cs = clo_type_sizeof(sa->count_type), vs = clo_type_sizeof(sa->value_type);
	const size_t need[6] = { segarg_src_bytes(sa, numel_seg), sizeof(cl_ulong), numel * vs, numel_seg * sizeof(cl_uint), numel_seg * vs, sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 6)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_seg (%zu) or numel (%zu) exceeds the size of the device buffers (counts_or_offsets "
			"holds numel_seg counts or numel_seg + 1 offsets, values_in numel rows, idx_out numel_seg cl_uints, val_out numel_seg values, "
			"num_in and num_out 8 bytes)", numel_seg, numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SEGARG: %s, %s, %s, %zu segments of type %s, %zu rows of %s", segarg_ops[sa->op], segarg_ties[sa->tie], segarg_forms[sa->form], numel_seg,
		clo_type_get_name(sa->count_type), numel, clo_type_get_name(sa->value_type));

	const size_t ws = clo_hip_segarg_workspace_bytes(numel_seg, numel);
	if (ws > 0 && !clo_op_reserve(&sa->head, cq_exec, ws, "hipMalloc(segarg workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SEGARG_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_segarg(sa->op, sa->tie, sa->form, p[0], (int) cs, (const uint64_t*) p[1], p[2], (uint32_t*) p[3], p[4], (uint64_t*) p[5],
		numel_seg, numel, (int) sa->value_type, sa->head.workspace.ptr, sa->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_segarg", err);
}

cl_bool clo_segarg_with_host_data(CloSegArg* sa, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	cl_uint* idx_out, void* val_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(sa != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = segarg_refusal(sa, counts_or_offsets, num_in, values_in, idx_out, val_out, num_out, numel_seg, numel, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const cl_ulong m_in = num_in ? (cl_ulong) *num_in : 0;
	*num_out = 0;
	if (numel_seg == 0 || (num_in && m_in == 0)) return CL_TRUE;   /* m == 0: no segments, no device needed */

	const size_t m = num_in && m_in < numel_seg ? (size_t) m_in : numel_seg;   /* the rows of idx_out and val_out that are written */
	const size_t vs = clo_type_sizeof(sa->value_type);
	cl_ulong total = 0;
	clo_stage st;
	clo_stage_open(&st, sa->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, counts_or_offsets, segarg_src_bytes(sa, numel_seg));
	clo_stage_in(&st, 1, num_in ? &m_in : NULL, sizeof(cl_ulong));
	clo_stage_in(&st, 2, values_in, numel * vs);
	clo_stage_out(&st, 3, idx_out, numel_seg * sizeof(cl_uint));
	clo_stage_out(&st, 4, val_out, numel_seg * vs);   /* NULL: the slot stays NULL, indices only */
	clo_stage_out(&st, 5, num_out, sizeof(cl_ulong));
	if (clo_stage_ok(&st))
		st.evt = clo_segarg_with_device_data(sa, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4], st.dev[5],
			numel_seg, numel, &st.err);
	clo_stage_read(&st, 5, &total, sizeof(cl_ulong));
	clo_stage_read(&st, 3, idx_out, m * sizeof(cl_uint));
	clo_stage_read(&st, 4, val_out, m * vs);
	if (clo_stage_ok(&st)) *num_out = (size_t) total;
	return clo_stage_close(&st, err);
}

CCLContext* clo_segarg_get_context(CloSegArg* sa) {
	clo_return_val_if_fail(sa != NULL, NULL);
	return sa->head.ctx;
}

const char* clo_segarg_get_op(CloSegArg* sa) {
	clo_return_val_if_fail(sa != NULL, NULL);
	return segarg_ops[sa->op];
}

const char* clo_segarg_get_tie(CloSegArg* sa) {
	clo_return_val_if_fail(sa != NULL, NULL);
	return segarg_ties[sa->tie];
}

const char* clo_segarg_get_form(CloSegArg* sa) {
	clo_return_val_if_fail(sa != NULL, NULL);
	return segarg_forms[sa->form];
}

CloType clo_segarg_get_value_type(CloSegArg* sa) {
	clo_return_val_if_fail(sa != NULL, (CloType) -1);
	return sa->value_type;
}

size_t clo_segarg_get_value_size(CloSegArg* sa) {
	clo_return_val_if_fail(sa != NULL, 0);
	return clo_type_sizeof(sa->value_type);
}

CloType clo_segarg_get_count_type(CloSegArg* sa) {
	clo_return_val_if_fail(sa != NULL, (CloType) -1);
	return sa->count_type;
}

size_t clo_segarg_get_count_size(CloSegArg* sa) {
	clo_return_val_if_fail(sa != NULL, 0);
	return clo_type_sizeof(sa->count_type);
}
