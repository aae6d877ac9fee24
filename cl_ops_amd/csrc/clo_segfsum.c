/*
 * clo_segfsum.c — CloSegFSum (include/clo_segfsum.h; not upstream): the floating-point sum of every segment in a fixed
 * order, the segments given by counts or by CSR offsets. The kernels are reached through the thin C-ABI
 * (clo_hip_segfsum, include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_segfsum.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SEGFSUM_EVENT "clo_segfsum"

struct clo_segfsum {
	clo_op_head head;        /* the workspace: the segment ends, the tiles' splits and states (clo_hip_segfsum_workspace_bytes) */
	int form;                /* index in segfsum_forms: what clo_hip_segfsum takes */
	CloType value_type, sum_type, count_type;
};

static const char* const segfsum_forms[] = { "counts", "offsets" };

static int segfsum_is_float(CloType t) { return t == CLO_HALF || t == CLO_FLOAT || t == CLO_DOUBLE; }

CloSegFSum* clo_segfsum_new(const char* form, const char* options, CCLContext* ctx,
	CloType value_type, CloType sum_type, CloType count_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int formi = clo_name_index(form, segfsum_forms, 2);
	if (formi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segment form '%s' (one of: " CLO_SEGREDUCE_FORMS ").", form ? form : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a floating-point segment sum (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_segfsum_new needs a context.");
		return NULL;
	}
	if (!segfsum_is_float(value_type) || !segfsum_is_float(sum_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A floating-point segment sum takes half, float or double values into float or double sums, "
			"not '%s' into '%s' (integer values and sums: CloSegReduce, clo_segreduce.h).",
			clo_type_get_name(value_type) ? clo_type_get_name(value_type) : "?", clo_type_get_name(sum_type) ? clo_type_get_name(sum_type) : "?");
		return NULL;
	}
	if (sum_type == CLO_HALF) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The sum type of a floating-point segment sum is float or double: half sums are not built.");
		return NULL;
	}
	if (clo_type_sizeof(sum_type) < clo_type_sizeof(value_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The sum type '%s' is narrower than the value type '%s'.",
			clo_type_get_name(sum_type), clo_type_get_name(value_type));
		return NULL;
	}
	if (value_type == CLO_HALF && sum_type == CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "half values into double sums are not built (half -> float, float -> float, float -> double, "
			"double -> double are).");
		return NULL;
	}
	if (count_type != CLO_UINT && count_type != CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The count_type of a floating-point segment sum is uint or ulong, not type %d.", (int) count_type);
		return NULL;
	}
	CloSegFSum* sf = (CloSegFSum*) clo_op_new(sizeof(CloSegFSum), ctx, err);
	if (!sf) return NULL;
	sf->form = formi;
	sf->value_type = value_type;
	sf->sum_type = sum_type;
	sf->count_type = count_type;
	return sf;
}

void clo_segfsum_destroy(CloSegFSum* sf) {
	clo_return_if_fail(sf != NULL);
	clo_op_destroy(sf);
}

/* the bytes counts_or_offsets holds: numel_seg counts, or numel_seg + 1 offsets */
static size_t segfsum_src_bytes(const CloSegFSum* sf, size_t numel_seg) {
	return (numel_seg + (sf->form == CLO_HIP_SEGFSUM_OFFSETS ? 1 : 0)) * clo_type_sizeof(sf->count_type);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * word_bytes: the size of what num_in and num_out point to (a cl_ulong of the device, a size_t of the host). */
static const char* segfsum_refusal(CloSegFSum* sf, const void* src, const void* num_in, const void* values_in,
	const void* sums_out, const void* num_out, size_t numel_seg, size_t numel, size_t word_bytes) {
	if (numel_seg > 0xffffffffull) return "numel_seg must be below 2^32";
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!num_out) return "num_out is required";
	if (!src && (numel_seg > 0 || sf->form == CLO_HIP_SEGFSUM_OFFSETS))
		return sf->form == CLO_HIP_SEGFSUM_OFFSETS ? "counts_or_offsets is required: the offsets" : "counts_or_offsets is required: the counts";
	if (!values_in && numel > 0) return "values_in is required";
	if (!sums_out && numel_seg > 0) return "sums_out is required";
	const clo_range in[3] = { { src, segfsum_src_bytes(sf, numel_seg) }, { num_in, word_bytes }, { values_in, numel * clo_type_sizeof(sf->value_type) } };
	/* sums_out is sized by numel_seg rows, however many segments *num_in leaves */
	const clo_range out[2] = { { sums_out, numel_seg * clo_type_sizeof(sf->sum_type) }, { num_out, word_bytes } };
	switch (clo_ranges_conflict(in, 3, out, 2)) {
		case CLO_RANGES_OUT_IN: return "an output range (sums_out or num_out) overlaps an input range";
		case CLO_RANGES_OUT_OUT: return "sums_out and num_out overlap";
	}
	return NULL;
}

CCLEvent* clo_segfsum_with_device_data(CloSegFSum* sf, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* sums_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(sf != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[5] = { counts_or_offsets, num_in, values_in, sums_out, num_out };
	void* p[5];
	clo_buffers_device_ptrs(buf, p, 5);
	const char* why = segfsum_refusal(sf, p[0], p[1], p[2], p[3], p[4], numel_seg, numel, sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[4] & 7u)) why = "num_out must be 8-byte aligned";
	if (!why && ((uintptr_t) p[1] & 7u)) why = "num_in must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t cs = clo_type_sizeof(sf->count_type);
	const size_t need[5] = { segfsum_src_bytes(sf, numel_seg), sizeof(cl_ulong), numel * clo_type_sizeof(sf->value_type),
		numel_seg * clo_type_sizeof(sf->sum_type), sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 5)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_seg (%zu) or numel (%zu) exceeds the size of the device buffers (counts_or_offsets "
			"holds numel_seg counts or numel_seg + 1 offsets, values_in numel rows, sums_out numel_seg rows, num_in and num_out 8 bytes)",
			numel_seg, numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SEGFSUM: %s, %zu segments of type %s, %zu rows of %s into %s", segfsum_forms[sf->form], numel_seg,
		clo_type_get_name(sf->count_type), numel, clo_type_get_name(sf->value_type), clo_type_get_name(sf->sum_type));

	const size_t ws = clo_hip_segfsum_workspace_bytes(numel_seg, numel);
	if (ws > 0 && !clo_op_reserve(&sf->head, cq_exec, ws, "hipMalloc(segfsum workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SEGFSUM_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_segfsum(sf->form, p[0], (int) cs, (const uint64_t*) p[1], p[2], p[3], (uint64_t*) p[4], numel_seg, numel,
		(int) sf->value_type, (int) sf->sum_type, sf->head.workspace.ptr, sf->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_segfsum", err);
}

cl_bool clo_segfsum_with_host_data(CloSegFSum* sf, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	void* sums_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(sf != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = segfsum_refusal(sf, counts_or_offsets, num_in, values_in, sums_out, num_out, numel_seg, numel, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const cl_ulong m_in = num_in ? (cl_ulong) *num_in : 0;
	*num_out = 0;
	if (numel_seg == 0 || (num_in && m_in == 0)) return CL_TRUE;   /* m == 0: no segments, no device needed */

	const size_t m = num_in && m_in < numel_seg ? (size_t) m_in : numel_seg;   /* the rows of sums_out that are written */
	const size_t ss = clo_type_sizeof(sf->sum_type);
	cl_ulong total = 0;
	clo_stage st;
	clo_stage_open(&st, sf->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, counts_or_offsets, segfsum_src_bytes(sf, numel_seg));
	clo_stage_in(&st, 1, num_in ? &m_in : NULL, sizeof(cl_ulong));
	clo_stage_in(&st, 2, values_in, numel * clo_type_sizeof(sf->value_type));
	clo_stage_out(&st, 3, sums_out, numel_seg * ss);
	clo_stage_out(&st, 4, num_out, sizeof(cl_ulong));
	if (clo_stage_ok(&st))
		st.evt = clo_segfsum_with_device_data(sf, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4],
			numel_seg, numel, &st.err);
	clo_stage_read(&st, 4, &total, sizeof(cl_ulong));
	clo_stage_read(&st, 3, sums_out, m * ss);
	if (clo_stage_ok(&st)) *num_out = (size_t) total;
	return clo_stage_close(&st, err);
}

CCLContext* clo_segfsum_get_context(CloSegFSum* sf) {
	clo_return_val_if_fail(sf != NULL, NULL);
	return sf->head.ctx;
}

const char* clo_segfsum_get_form(CloSegFSum* sf) {
	clo_return_val_if_fail(sf != NULL, NULL);
	return segfsum_forms[sf->form];
}

CloType clo_segfsum_get_value_type(CloSegFSum* sf) {
	clo_return_val_if_fail(sf != NULL, (CloType) -1);
	return sf->value_type;
}

size_t clo_segfsum_get_value_size(CloSegFSum* sf) {
	clo_return_val_if_fail(sf != NULL, 0);
	return clo_type_sizeof(sf->value_type);
}

CloType clo_segfsum_get_sum_type(CloSegFSum* sf) {
	clo_return_val_if_fail(sf != NULL, (CloType) -1);
	return sf->sum_type;
}

size_t clo_segfsum_get_sum_size(CloSegFSum* sf) {
	clo_return_val_if_fail(sf != NULL, 0);
	return clo_type_sizeof(sf->sum_type);
}

CloType clo_segfsum_get_count_type(CloSegFSum* sf) {
	clo_return_val_if_fail(sf != NULL, (CloType) -1);
	return sf->count_type;
}

size_t clo_segfsum_get_count_size(CloSegFSum* sf) {
	clo_return_val_if_fail(sf != NULL, 0);
	return clo_type_sizeof(sf->count_type);
}
