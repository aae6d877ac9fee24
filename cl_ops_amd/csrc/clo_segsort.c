/*
 * clo_segsort.c — CloSegSort (include/clo_segsort.h; not upstream): a stable sort of every segment on its own, the
 * segments given by counts or by CSR offsets. The kernels are reached through the thin C-ABI (clo_hip_segsort,
 * include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_segsort.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SEGSORT_EVENT "clo_segsort"

struct clo_segsort {
	clo_op_head head;        /* the workspace: a second copy of the rows, the heads, the segment ends (clo_hip_segsort_workspace_bytes) */
	int form;                /* index in segsort_forms: what clo_hip_segsort takes */
	CloType key_type, count_type;
	size_t value_size;
};

static const char* const segsort_forms[] = { "counts", "offsets" };

CloSegSort* clo_segsort_new(const char* form, const char* options, CCLContext* ctx,
	CloType key_type, size_t value_size, CloType count_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int formi = clo_name_index(form, segsort_forms, 2);
	if (formi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segment form '%s' (one of: " CLO_SEGSORT_FORMS ").", form ? form : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a segmented sort (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_segsort_new needs a context.");
		return NULL;
	}
	if (clo_type_sizeof(key_type) == 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for a segmented sort.", (int) key_type);
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The value_size of a segmented sort is 0, 4 or 8 bytes, not %zu.", value_size);
		return NULL;
	}
	if (count_type != CLO_UINT && count_type != CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The count_type of a segmented sort is uint or ulong, not type %d.", (int) count_type);
		return NULL;
	}
	CloSegSort* ss = (CloSegSort*) clo_op_new(sizeof(CloSegSort), ctx, err);
	if (!ss) return NULL;
	ss->form = formi;
	ss->key_type = key_type;
	ss->value_size = value_size;
	ss->count_type = count_type;
	return ss;
}

void clo_segsort_destroy(CloSegSort* ss) {
	clo_return_if_fail(ss != NULL);
	clo_op_destroy(ss);
}

/* the bytes counts_or_offsets holds: numel_seg counts, or numel_seg + 1 offsets */
static size_t segsort_src_bytes(const CloSegSort* ss, size_t numel_seg) {
	return (numel_seg + (ss->form == CLO_HIP_SEGSORT_OFFSETS ? 1 : 0)) * clo_type_sizeof(ss->count_type);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * word_bytes: the size of what num_in and num_out point to (a cl_ulong of the device, a size_t of the host). */
static const char* segsort_refusal(CloSegSort* ss, const void* src, const void* num_in, const void* keys_in, const void* values_in,
	const void* keys_out, const void* values_out, const void* num_out, size_t numel_seg, size_t numel, size_t word_bytes) {
	if (numel_seg > 0xffffffffull) return "numel_seg must be below 2^32";
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!num_out) return "num_out is required";
	if (!src && (numel_seg > 0 || ss->form == CLO_HIP_SEGSORT_OFFSETS))
		return ss->form == CLO_HIP_SEGSORT_OFFSETS ? "counts_or_offsets is required: the offsets" : "counts_or_offsets is required: the counts";
	if (!keys_in && numel > 0) return "keys_in is required";
	if (ss->value_size == 0 && (values_in || values_out)) return "values were passed to a sort with value_size 0";
	if (ss->value_size > 0 && !values_out) return "values_out is required";
	if (ss->value_size == 8 && !values_in) return "values_in is required with value_size 8 (the arg form has value_size 4)";
	if (!keys_out && !(ss->value_size == 4 && !values_in)) return "keys_out is required outside the arg form";
	const size_t kb = numel * clo_type_sizeof(ss->key_type), vb = numel * ss->value_size;
	const clo_range in[4] = { { src, segsort_src_bytes(ss, numel_seg) }, { num_in, word_bytes }, { keys_in, kb }, { values_in, vb } };
	const clo_range out[3] = { { keys_out, kb }, { values_out, vb }, { num_out, word_bytes } };
	switch (clo_ranges_conflict(in, 4, out, 3)) {
		case CLO_RANGES_OUT_IN: return "an output range (keys_out, values_out or num_out) overlaps an input range";
		case CLO_RANGES_OUT_OUT: return "keys_out, values_out and num_out overlap";
	}
	return NULL;
}

CCLEvent* clo_segsort_with_device_data(CloSegSort* ss, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* keys_in, CCLBuffer* values_in,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(ss != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[7] = { counts_or_offsets, num_in, keys_in, values_in, keys_out, values_out, num_out };
	void* p[7];
	clo_buffers_device_ptrs(buf, p, 7);
	const char* why = segsort_refusal(ss, p[0], p[1], p[2], p[3], p[4], p[5], p[6], numel_seg, numel, sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[6] & 7u)) why = "num_out must be 8-byte aligned";
	if (!why && ((uintptr_t) p[1] & 7u)) why = "num_in must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t cs = clo_type_sizeof(ss->count_type), ks = clo_type_sizeof(ss->key_type);
	const size_t need[7] = { segsort_src_bytes(ss, numel_seg), sizeof(cl_ulong), numel * ks, numel * ss->value_size,
		numel * ks, numel * ss->value_size, sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 7)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_seg (%zu) or numel (%zu) exceeds the size of the device buffers (counts_or_offsets "
			"holds numel_seg counts or numel_seg + 1 offsets, the keys and values numel rows, num_in and num_out 8 bytes)", numel_seg, numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SEGSORT: %s, %zu segments of type %s, %zu rows of %s with %zu-byte values", segsort_forms[ss->form], numel_seg,
		clo_type_get_name(ss->count_type), numel, clo_type_get_name(ss->key_type), ss->value_size);

	const size_t ws = clo_hip_segsort_workspace_bytes(numel_seg, numel, (int) ks, (int) ss->value_size);
	if (ws > 0 && !clo_op_reserve(&ss->head, cq_exec, ws, "hipMalloc(segsort workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SEGSORT_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_segsort(ss->form, p[0], (int) cs, (const uint64_t*) p[1], p[2], p[3], p[4], p[5], (uint64_t*) p[6], numel_seg, numel,
		(int) ss->key_type, (int) ss->value_size, ss->head.workspace.ptr, ss->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_segsort", err);
}

cl_bool clo_segsort_with_host_data(CloSegSort* ss, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err) {
	clo_return_val_if_fail(ss != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = segsort_refusal(ss, counts_or_offsets, num_in, keys_in, values_in, keys_out, values_out, num_out, numel_seg, numel, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const cl_ulong m_in = num_in ? (cl_ulong) *num_in : 0;
	*num_out = 0;
	if (numel_seg == 0 || (num_in && m_in == 0)) return CL_TRUE;   /* m == 0: no segments, no device needed */

	const size_t ks = clo_type_sizeof(ss->key_type), vs = ss->value_size;
	cl_ulong total = 0;
	clo_stage st;
	clo_stage_open(&st, ss->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, counts_or_offsets, segsort_src_bytes(ss, numel_seg));
	clo_stage_in(&st, 1, num_in ? &m_in : NULL, sizeof(cl_ulong));
	/* numel 0 (total is still wanted): what the caller passed stays present, as one byte that is never touched */
	const size_t kb = numel * ks, vb = numel * vs;
	clo_stage_in(&st, 2, keys_in, kb);
	if (vb) clo_stage_in(&st, 3, values_in, vb);
	else clo_stage_out(&st, 3, values_in, 1);
	clo_stage_out(&st, 4, keys_out, kb ? kb : 1);
	clo_stage_out(&st, 5, values_out, vb ? vb : 1);
	clo_stage_out(&st, 6, num_out, sizeof(cl_ulong));
	if (clo_stage_ok(&st))
		st.evt = clo_segsort_with_device_data(ss, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4], st.dev[5], st.dev[6],
			numel_seg, numel, &st.err);
	clo_stage_read(&st, 6, &total, sizeof(cl_ulong));
	const size_t rows = clo_stage_ok(&st) ? (total < numel ? (size_t) total : numel) : 0;   /* the rows that were written */
	clo_stage_read(&st, 4, keys_out, rows * ks);
	clo_stage_read(&st, 5, values_out, rows * vs);
	if (clo_stage_ok(&st)) *num_out = (size_t) total;
	return clo_stage_close(&st, err);
}

CCLContext* clo_segsort_get_context(CloSegSort* ss) {
	clo_return_val_if_fail(ss != NULL, NULL);
	return ss->head.ctx;
}

const char* clo_segsort_get_form(CloSegSort* ss) {
	clo_return_val_if_fail(ss != NULL, NULL);
	return segsort_forms[ss->form];
}

CloType clo_segsort_get_key_type(CloSegSort* ss) {
	clo_return_val_if_fail(ss != NULL, (CloType) -1);
	return ss->key_type;
}

size_t clo_segsort_get_key_size(CloSegSort* ss) {
	clo_return_val_if_fail(ss != NULL, 0);
	return clo_type_sizeof(ss->key_type);
}

size_t clo_segsort_get_value_size(CloSegSort* ss) {
	clo_return_val_if_fail(ss != NULL, 0);
	return ss->value_size;
}

CloType clo_segsort_get_count_type(CloSegSort* ss) {
	clo_return_val_if_fail(ss != NULL, (CloType) -1);
	return ss->count_type;
}

size_t clo_segsort_get_count_size(CloSegSort* ss) {
	clo_return_val_if_fail(ss != NULL, 0);
	return clo_type_sizeof(ss->count_type);
}
