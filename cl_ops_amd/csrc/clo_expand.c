/*
 * clo_expand.c — CloExpand (include/clo_expand.h; not upstream): run-length decode and segment ids from counts or from
 * CSR offsets. The kernels are reached through the thin C-ABI (clo_hip_expand, include/clo_hip.h); the host layer is
 * the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_expand.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_EXPAND_EVENT "clo_expand"

struct clo_expand {
	clo_op_head head;        /* the workspace: the segment ends, the tiles' first segments (clo_hip_expand_workspace_bytes) */
	int form;                /* index in expand_forms: what clo_hip_expand takes */
	CloType value_type;
	CloType count_type;
};

static const char* const expand_forms[] = { "counts", "offsets" };

CloExpand* clo_expand_new(const char* form, const char* options, CCLContext* ctx, CloType value_type, CloType count_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int formi = clo_name_index(form, expand_forms, 2);
	if (formi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown expansion form '%s' (one of: " CLO_EXPAND_FORMS ").", form ? form : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for an expansion (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_expand_new needs a context.");
		return NULL;
	}
	if ((int) value_type < (int) CLO_CHAR || (int) value_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown value_type %d for an expansion.", (int) value_type);
		return NULL;
	}
	if (count_type != CLO_UINT && count_type != CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The count_type of an expansion is uint or ulong, not type %d.", (int) count_type);
		return NULL;
	}
	CloExpand* ex = (CloExpand*) clo_op_new(sizeof(CloExpand), ctx, err);
	if (!ex) return NULL;
	ex->form = formi;
	ex->value_type = value_type;
	ex->count_type = count_type;
	return ex;
}

void clo_expand_destroy(CloExpand* ex) {
	clo_return_if_fail(ex != NULL);
	clo_op_destroy(ex);
}

/* the bytes counts_or_offsets holds: numel_in counts, or numel_in + 1 offsets */
static size_t expand_src_bytes(const CloExpand* ex, size_t numel_in) {
	return (numel_in + (ex->form == CLO_HIP_EXPAND_OFFSETS ? 1 : 0)) * clo_type_sizeof(ex->count_type);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * word_bytes: the size of what num_in and num_out point to (a cl_ulong of the device, a size_t of the host). */
static const char* expand_refusal(CloExpand* ex, const void* src, const void* num_in, const void* values_in,
	const void* values_out, const void* seg_out, const void* rank_out, const void* num_out, size_t numel_in, size_t capacity, size_t word_bytes) {
	if (numel_in > 0xffffffffull) return "numel_in must be below 2^32";
	if (capacity > 0xffffffffull) return "capacity must be below 2^32";
	if (!num_out) return "num_out is required";
	if (!src && (numel_in > 0 || (ex->form == CLO_HIP_EXPAND_OFFSETS && capacity > 0)))
		return ex->form == CLO_HIP_EXPAND_OFFSETS ? "counts_or_offsets is required: the offsets" : "counts_or_offsets is required: the counts";
	if (!values_out && !seg_out && !rank_out) return "values_out, seg_out and rank_out are all NULL";
	if (values_in && !values_out) return "values_in given without values_out";
	if (!values_in && values_out) return "values_out given without values_in";
	const size_t vs = clo_type_sizeof(ex->value_type);
	const clo_range in[3] = { { src, expand_src_bytes(ex, numel_in) }, { num_in, word_bytes }, { values_in, numel_in * vs } };
	/* the outputs are sized by capacity rows, whatever total turns out to be */
	const clo_range out[4] = { { values_out, capacity * vs }, { seg_out, capacity * sizeof(cl_uint) }, { rank_out, capacity * sizeof(cl_uint) },
		{ num_out, word_bytes } };
	switch (clo_ranges_conflict(in, 3, out, 4)) {
		case CLO_RANGES_OUT_IN: return "an output range (values_out, seg_out, rank_out or num_out) overlaps an input range";
		case CLO_RANGES_OUT_OUT: return "two output ranges (of values_out, seg_out, rank_out and num_out) overlap";
	}
	return NULL;
}

CCLEvent* clo_expand_with_device_data(CloExpand* ex, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* values_out, CCLBuffer* seg_out, CCLBuffer* rank_out, CCLBuffer* num_out,
	size_t numel_in, size_t capacity, GError** err) {
	clo_return_val_if_fail(ex != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[7] = { counts_or_offsets, num_in, values_in, values_out, seg_out, rank_out, num_out };
	void* p[7];
	clo_buffers_device_ptrs(buf, p, 7);
	const char* why = expand_refusal(ex, p[0], p[1], p[2], p[3], p[4], p[5], p[6], numel_in, capacity, sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[6] & 7u)) why = "num_out must be 8-byte aligned";
	if (!why && ((uintptr_t) p[1] & 7u)) why = "num_in must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t vs = clo_type_sizeof(ex->value_type), cs = clo_type_sizeof(ex->count_type);
	const size_t need[7] = { expand_src_bytes(ex, numel_in), sizeof(cl_ulong), numel_in * vs, capacity * vs, capacity * sizeof(cl_uint),
		capacity * sizeof(cl_uint), sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 7)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_in (%zu) or capacity (%zu) exceeds the size of the device buffers (counts_or_offsets "
			"holds numel_in counts or numel_in + 1 offsets, values_in numel_in rows, values_out, seg_out and rank_out capacity rows, num_in and "
			"num_out 8 bytes)", numel_in, capacity);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("EXPAND: %s, %zu segments of type %s, capacity %zu, %s", expand_forms[ex->form], numel_in, clo_type_get_name(ex->count_type), capacity,
		p[2] ? clo_type_get_name(ex->value_type) : "no values");

	const size_t ws = clo_hip_expand_workspace_bytes(numel_in, capacity);
	if (ws > 0 && !clo_op_reserve(&ex->head, cq_exec, ws, "hipMalloc(expand workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_EXPAND_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_expand(ex->form, p[0], (int) cs, (const uint64_t*) p[1], p[2], p[3], p[4], p[5], (uint64_t*) p[6], numel_in, capacity,
		(int) vs, ex->head.workspace.ptr, ex->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_expand", err);
}

cl_bool clo_expand_with_host_data(CloExpand* ex, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	void* values_out, void* seg_out, void* rank_out, size_t* num_out,
	size_t numel_in, size_t capacity, GError** err) {
	clo_return_val_if_fail(ex != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = expand_refusal(ex, counts_or_offsets, num_in, values_in, values_out, seg_out, rank_out, num_out, numel_in, capacity, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const cl_ulong m_in = num_in ? (cl_ulong) *num_in : 0;
	*num_out = 0;
	if (numel_in == 0 || (num_in && m_in == 0)) return CL_TRUE;   /* m == 0: no rows, no device needed */

	const size_t vs = clo_type_sizeof(ex->value_type);
	/* an output of a size query still needs a buffer to stand for it: one row */
	const size_t rows_held = capacity ? capacity : 1;
	cl_ulong total = 0;
	clo_stage st;
	clo_stage_open(&st, ex->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, counts_or_offsets, expand_src_bytes(ex, numel_in));
	clo_stage_in(&st, 1, num_in ? &m_in : NULL, sizeof(cl_ulong));
	clo_stage_in(&st, 2, values_in, numel_in * vs);
	clo_stage_out(&st, 3, values_out, rows_held * vs);
	clo_stage_out(&st, 4, seg_out, rows_held * sizeof(cl_uint));
	clo_stage_out(&st, 5, rank_out, rows_held * sizeof(cl_uint));
	clo_stage_out(&st, 6, num_out, sizeof(cl_ulong));
	if (clo_stage_ok(&st))
		st.evt = clo_expand_with_device_data(ex, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4], st.dev[5], st.dev[6],
			numel_in, capacity, &st.err);
	/* the total first (blocking): it says how many rows there are to copy */
	clo_stage_read(&st, 6, &total, sizeof(cl_ulong));
	const size_t rows = total < capacity ? (size_t) total : capacity;
	clo_stage_read(&st, 3, values_out, rows * vs);
	clo_stage_read(&st, 4, seg_out, rows * sizeof(cl_uint));
	clo_stage_read(&st, 5, rank_out, rows * sizeof(cl_uint));
	if (clo_stage_ok(&st)) *num_out = (size_t) total;
	return clo_stage_close(&st, err);
}

CCLContext* clo_expand_get_context(CloExpand* ex) {
	clo_return_val_if_fail(ex != NULL, NULL);
	return ex->head.ctx;
}

const char* clo_expand_get_form(CloExpand* ex) {
	clo_return_val_if_fail(ex != NULL, NULL);
	return expand_forms[ex->form];
}

CloType clo_expand_get_value_type(CloExpand* ex) {
	clo_return_val_if_fail(ex != NULL, (CloType) -1);
	return ex->value_type;
}

size_t clo_expand_get_value_size(CloExpand* ex) {
	clo_return_val_if_fail(ex != NULL, 0);
	return clo_type_sizeof(ex->value_type);
}

CloType clo_expand_get_count_type(CloExpand* ex) {
	clo_return_val_if_fail(ex != NULL, (CloType) -1);
	return ex->count_type;
}

size_t clo_expand_get_count_size(CloExpand* ex) {
	clo_return_val_if_fail(ex != NULL, 0);
	return clo_type_sizeof(ex->count_type);
}
