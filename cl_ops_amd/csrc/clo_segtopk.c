/*
 * clo_segtopk.c — CloSegTopK (include/clo_segtopk.h; not upstream): the k smallest or largest rows of every segment,
 * the segments given by counts or by CSR offsets. The kernels are reached through the thin C-ABI (clo_hip_segtopk,
 * include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_segtopk.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SEGTOPK_EVENT "clo_segtopk"

struct clo_segtopk {
	clo_op_head head;        /* the workspace: the heads, the segment ends, the tiles' candidates (clo_hip_segtopk_workspace_bytes) */
	int which;               /* index in segtopk_which: what clo_hip_segtopk takes */
	int form;                /* index in segtopk_forms: likewise */
	CloType key_type, count_type;
	size_t value_size;
};

static const char* const segtopk_which[] = { "smallest", "largest" };
static const char* const segtopk_forms[] = { "counts", "offsets" };

CloSegTopK* clo_segtopk_new(const char* which, const char* form, const char* options, CCLContext* ctx,
	CloType key_type, size_t value_size, CloType count_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int whichi = clo_name_index(which, segtopk_which, 2);
	if (whichi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown which '%s' (one of: " CLO_SEGTOPK_WHICH ").", which ? which : "(null)");
		return NULL;
	}
	const int formi = clo_name_index(form, segtopk_forms, 2);
	if (formi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown segment form '%s' (one of: " CLO_SEGREDUCE_FORMS ").", form ? form : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a segmented top-k (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_segtopk_new needs a context.");
		return NULL;
	}
	if (clo_type_sizeof(key_type) == 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for a segmented top-k.", (int) key_type);
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The value_size of a segmented top-k is 0, 4 or 8 bytes, not %zu.", value_size);
		return NULL;
	}
	if (count_type != CLO_UINT && count_type != CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The count_type of a segmented top-k is uint or ulong, not type %d.", (int) count_type);
		return NULL;
	}
	CloSegTopK* st = (CloSegTopK*) clo_op_new(sizeof(CloSegTopK), ctx, err);
	if (!st) return NULL;
	st->which = whichi;
	st->form = formi;
	st->key_type = key_type;
	st->value_size = value_size;
	st->count_type = count_type;
	return st;
}

void clo_segtopk_destroy(CloSegTopK* st) {
	clo_return_if_fail(st != NULL);
	clo_op_destroy(st);
}

/* the bytes counts_or_offsets holds: numel_seg counts, or numel_seg + 1 offsets */
static size_t segtopk_src_bytes(const CloSegTopK* st, size_t numel_seg) {
	return (numel_seg + (st->form == CLO_HIP_SEGTOPK_OFFSETS ? 1 : 0)) * clo_type_sizeof(st->count_type);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * word_bytes: the size of what num_in and num_out point to (a cl_ulong of the device, a size_t of the host). */
static const char* segtopk_refusal(CloSegTopK* st, const void* src, const void* num_in, const void* keys_in, const void* values_in,
	const void* keys_out, const void* values_out, const void* counts_out, const void* num_out, size_t numel_seg, size_t numel, size_t k,
	size_t word_bytes) {
	if (numel_seg > 0xffffffffull) return "numel_seg must be below 2^32";
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (k > clo_hip_segtopk_k_max((int) clo_type_sizeof(st->key_type), (int) st->value_size))
		return "k is above the cap (clo_hip_segtopk_k_max): sort the segments with CloSegSort instead";
	if ((unsigned long long) numel_seg * k > 0xffffffffull) return "numel_seg * k must be below 2^32";
	if (!num_out) return "num_out is required";
	if (!src && (numel_seg > 0 || st->form == CLO_HIP_SEGTOPK_OFFSETS))
		return st->form == CLO_HIP_SEGTOPK_OFFSETS ? "counts_or_offsets is required: the offsets" : "counts_or_offsets is required: the counts";
	if (!keys_in && numel > 0) return "keys_in is required";
	if (st->value_size == 0 && (values_in || values_out)) return "values were passed to a top-k with value_size 0";
	if (st->value_size > 0 && !values_out) return "values_out is required";
	if (st->value_size == 8 && !values_in) return "values_in is required with value_size 8 (the arg form has value_size 4)";
	if (!keys_out && !(st->value_size == 4 && !values_in)) return "keys_out is required outside the arg form";
	if (!counts_out && numel_seg > 0 && k > 0) return "counts_out is required";
	const size_t ks = clo_type_sizeof(st->key_type), rows = numel_seg * k;
	const clo_range in[4] = { { src, segtopk_src_bytes(st, numel_seg) }, { num_in, word_bytes }, { keys_in, numel * ks }, { values_in, numel * st->value_size } };
	/* the outputs are sized by numel_seg rows of k slots, however many segments *num_in leaves; k 0: none is written */
	const clo_range out[4] = { { keys_out, rows * ks }, { values_out, rows * st->value_size }, { counts_out, k ? numel_seg * sizeof(cl_uint) : 0 }, { num_out, word_bytes } };
	switch (clo_ranges_conflict(in, 4, out, 4)) {
		case CLO_RANGES_OUT_IN: return "an output range (keys_out, values_out, counts_out or num_out) overlaps an input range";
		case CLO_RANGES_OUT_OUT: return "two of keys_out, values_out, counts_out and num_out overlap";
	}
	return NULL;
}

CCLEvent* clo_segtopk_with_device_data(CloSegTopK* st, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* keys_in, CCLBuffer* values_in,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* counts_out, CCLBuffer* num_out,
	size_t numel_seg, size_t numel, size_t k, GError** err) {
	clo_return_val_if_fail(st != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[8] = { counts_or_offsets, num_in, keys_in, values_in, keys_out, values_out, counts_out, num_out };
	void* p[8];
	clo_buffers_device_ptrs(buf, p, 8);
	const char* why = segtopk_refusal(st, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], numel_seg, numel, k, sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[7] & 7u)) why = "num_out must be 8-byte aligned";
	if (!why && ((uintptr_t) p[1] & 7u)) why = "num_in must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t cs = clo_type_sizeof(st->count_type), ks = clo_type_sizeof(st->key_type), rows = numel_seg * k;
	const size_t need[8] = { segtopk_src_bytes(st, numel_seg), sizeof(cl_ulong), numel * ks, numel * st->value_size,
		rows * ks, rows * st->value_size, k ? numel_seg * sizeof(cl_uint) : 0, sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 8)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_seg (%zu), numel (%zu) or k (%zu) exceeds the size of the device buffers (counts_or_offsets "
			"holds numel_seg counts or numel_seg + 1 offsets, keys_in and values_in numel rows, keys_out and values_out numel_seg * k rows, "
			"counts_out numel_seg cl_uints, num_in and num_out 8 bytes)", numel_seg, numel, k);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SEGTOPK: %s %zu, %s, %zu segments of type %s, %zu rows of %s with %zu-byte values", segtopk_which[st->which], k, segtopk_forms[st->form],
		numel_seg, clo_type_get_name(st->count_type), numel, clo_type_get_name(st->key_type), st->value_size);

	const size_t ws = clo_hip_segtopk_workspace_bytes(numel_seg, numel, k, (int) ks, (int) st->value_size);
	if (ws > 0 && !clo_op_reserve(&st->head, cq_exec, ws, "hipMalloc(segtopk workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SEGTOPK_EVENT, err);
	if (!evt) return NULL;
	const int status = clo_hip_segtopk(st->which, st->form, p[0], (int) cs, (const uint64_t*) p[1], p[2], p[3], p[4], p[5], (uint32_t*) p[6], (uint64_t*) p[7],
		numel_seg, numel, k, (int) st->key_type, (int) st->value_size, st->head.workspace.ptr, st->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, status, "clo_hip_segtopk", err);
}

cl_bool clo_segtopk_with_host_data(CloSegTopK* st, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, cl_uint* counts_out, size_t* num_out,
	size_t numel_seg, size_t numel, size_t k, GError** err) {
	clo_return_val_if_fail(st != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = segtopk_refusal(st, counts_or_offsets, num_in, keys_in, values_in, keys_out, values_out, counts_out, num_out, numel_seg, numel, k,
		sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const cl_ulong m_in = num_in ? (cl_ulong) *num_in : 0;
	*num_out = 0;
	if (numel_seg == 0 || (num_in && m_in == 0)) return CL_TRUE;   /* m == 0: no segments, no device needed */

	const size_t m = num_in && m_in < numel_seg ? (size_t) m_in : numel_seg;   /* the rows of the outputs that are written */
	const size_t ks = clo_type_sizeof(st->key_type), vs = st->value_size;
	cl_ulong total = 0;
	clo_stage sg;
	clo_stage_open(&sg, st->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&sg, 0, counts_or_offsets, segtopk_src_bytes(st, numel_seg));
	clo_stage_in(&sg, 1, num_in ? &m_in : NULL, sizeof(cl_ulong));
	/* numel 0 (total is still wanted): what the caller passed stays present, as one byte that is never touched */
	const size_t kb = numel * ks, vb = numel * vs;
	if (kb) clo_stage_in(&sg, 2, keys_in, kb);
	else clo_stage_out(&sg, 2, keys_in, 1);
	if (vb) clo_stage_in(&sg, 3, values_in, vb);
	else clo_stage_out(&sg, 3, values_in, 1);
	/* the outputs go up with what the caller left in them: the slots that are not written come back as they were. k 0:
	 * nothing is written, and what the caller passed stays present as one byte */
	const size_t rows = numel_seg * k;
	if (rows) {
		clo_stage_in(&sg, 4, keys_out, rows * ks);
		clo_stage_in(&sg, 5, values_out, rows * vs);
		clo_stage_in(&sg, 6, counts_out, numel_seg * sizeof(cl_uint));
	} else {
		clo_stage_out(&sg, 4, keys_out, 1);
		clo_stage_out(&sg, 5, values_out, 1);
		clo_stage_out(&sg, 6, counts_out, 1);
	}
	clo_stage_out(&sg, 7, num_out, sizeof(cl_ulong));
	if (clo_stage_ok(&sg))
		sg.evt = clo_segtopk_with_device_data(st, sg.cq_exec, sg.cq_comm, sg.dev[0], sg.dev[1], sg.dev[2], sg.dev[3], sg.dev[4], sg.dev[5], sg.dev[6],
			sg.dev[7], numel_seg, numel, k, &sg.err);
	clo_stage_read(&sg, 7, &total, sizeof(cl_ulong));
	if (k > 0) {
		clo_stage_read(&sg, 4, keys_out, m * k * ks);
		clo_stage_read(&sg, 5, values_out, m * k * vs);
		clo_stage_read(&sg, 6, counts_out, m * sizeof(cl_uint));
	}
	if (clo_stage_ok(&sg)) *num_out = (size_t) total;
	return clo_stage_close(&sg, err);
}

CCLContext* clo_segtopk_get_context(CloSegTopK* st) {
	clo_return_val_if_fail(st != NULL, NULL);
	return st->head.ctx;
}

const char* clo_segtopk_get_which(CloSegTopK* st) {
	clo_return_val_if_fail(st != NULL, NULL);
	return segtopk_which[st->which];
}

const char* clo_segtopk_get_form(CloSegTopK* st) {
	clo_return_val_if_fail(st != NULL, NULL);
	return segtopk_forms[st->form];
}

CloType clo_segtopk_get_key_type(CloSegTopK* st) {
	clo_return_val_if_fail(st != NULL, (CloType) -1);
	return st->key_type;
}

size_t clo_segtopk_get_key_size(CloSegTopK* st) {
	clo_return_val_if_fail(st != NULL, 0);
	return clo_type_sizeof(st->key_type);
}

size_t clo_segtopk_get_value_size(CloSegTopK* st) {
	clo_return_val_if_fail(st != NULL, 0);
	return st->value_size;
}

CloType clo_segtopk_get_count_type(CloSegTopK* st) {
	clo_return_val_if_fail(st != NULL, (CloType) -1);
	return st->count_type;
}

size_t clo_segtopk_get_count_size(CloSegTopK* st) {
	clo_return_val_if_fail(st != NULL, 0);
	return clo_type_sizeof(st->count_type);
}
