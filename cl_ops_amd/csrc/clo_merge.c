/*
 * clo_merge.c — CloMerge (include/clo_merge.h; not upstream): the stable merge of two sorted arrays, with values
 * or as argmerge. The kernels are reached through the thin C-ABI (clo_hip_merge, include/clo_hip.h); the host layer
 * is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_merge.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_MERGE_EVENT "clo_merge"

struct clo_merge {
	clo_op_head head;        /* the workspace: the tiles' split points (clo_hip_merge_workspace_bytes) */
	CloType key_type;
	size_t value_size;
};

CloMerge* clo_merge_new(const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for merge (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_merge_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for merge.", (int) key_type);
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Merge carries values of 0 (none), 4 or 8 bytes, not a value_size of %zu.", value_size);
		return NULL;
	}
	CloMerge* m = (CloMerge*) clo_op_new(sizeof(CloMerge), ctx, err);
	if (!m) return NULL;
	m->key_type = key_type;
	m->value_size = value_size;
	return m;
}

void clo_merge_destroy(CloMerge* m) {
	clo_return_if_fail(m != NULL);
	clo_op_destroy(m);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced. */
static const char* merge_refusal(CloMerge* m, const void* keys_a, const void* values_a, size_t numel_a,
	const void* keys_b, const void* values_b, size_t numel_b, const void* keys_out, const void* values_out) {
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull)
		return "numel_a + numel_b must be below 2^32";
	if (numel_a > 0 && !keys_a) return "keys_a is required";
	if (numel_b > 0 && !keys_b) return "keys_b is required";
	if (!keys_out && !values_out) return "keys_out and values_out are both NULL";
	if (m->value_size == 0 && (values_a || values_b || values_out)) return "values passed to a merge made with value_size 0";
	if (m->value_size > 0 && !values_out) return "values_out is required with a value_size above 0";
	if (numel_a > 0 && numel_b > 0 && (values_a == NULL) != (values_b == NULL))
		return "values_a and values_b must both be given, or both be NULL (argmerge)";
	if (m->value_size == 8 && ((numel_a > 0 && !values_a) || (numel_b > 0 && !values_b)))
		return "NULL values (argmerge) need a value_size of 4: the permutation is written as uint";
	const size_t ks = clo_type_sizeof(m->key_type), vs = m->value_size, n = numel_a + numel_b;
	const clo_range in[4] = { { keys_a, numel_a * ks }, { keys_b, numel_b * ks }, { values_a, numel_a * vs }, { values_b, numel_b * vs } };
	const clo_range out[2] = { { keys_out, n * ks }, { values_out, n * vs } };
	switch (clo_ranges_conflict(in, 4, out, 2)) {
		case CLO_RANGES_OUT_IN: return "an output range overlaps an input range (there is no in-place merge)";
		case CLO_RANGES_OUT_OUT: return "keys_out overlaps values_out";
	}
	return NULL;
}

CCLEvent* clo_merge_with_device_data(CloMerge* m, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_a, CCLBuffer* values_a, size_t numel_a, CCLBuffer* keys_b, CCLBuffer* values_b, size_t numel_b,
	CCLBuffer* keys_out, CCLBuffer* values_out, GError** err) {
	clo_return_val_if_fail(m != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[6] = { keys_a, values_a, keys_b, values_b, keys_out, values_out };
	void* p[6];
	clo_buffers_device_ptrs(buf, p, 6);
	const char* why = merge_refusal(m, p[0], p[1], numel_a, p[2], p[3], numel_b, p[4], p[5]);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(m->key_type), vs = m->value_size, n = numel_a + numel_b;
	const size_t need[6] = { numel_a * ks, numel_a * vs, numel_b * ks, numel_b * vs, n * ks, n * vs };
	if (!clo_buffers_hold(buf, need, 6)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_a (%zu) and numel_b (%zu) exceed the size of the device buffers", numel_a, numel_b);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("MERGE: %zu + %zu keys of type %s, %s", numel_a, numel_b, clo_type_get_name(m->key_type),
		vs == 0 ? "no values" : ((numel_a > 0 && !p[1]) || (numel_b > 0 && !p[3])) ? "argmerge" : vs == 4 ? "4-byte values" : "8-byte values");

	const size_t ws = clo_hip_merge_workspace_bytes(numel_a, numel_b);
	if (ws > 0 && !clo_op_reserve(&m->head, cq_exec, ws, "hipMalloc(merge workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_MERGE_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_merge(p[0], p[1], numel_a, p[2], p[3], numel_b, p[4], p[5], (int) ks, clo_type_key_kind(m->key_type), (int) vs,
		m->head.workspace.ptr, m->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_merge", err);
}

cl_bool clo_merge_with_host_data(CloMerge* m, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_a, const void* values_a, size_t numel_a, const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, GError** err) {
	clo_return_val_if_fail(m != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = merge_refusal(m, keys_a, values_a, numel_a, keys_b, values_b, numel_b, keys_out, values_out);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const size_t n = numel_a + numel_b;
	if (n == 0) return CL_TRUE;   /* no device needed */

	const size_t ks = clo_type_sizeof(m->key_type), vs = m->value_size;
	/* keys a, values a, keys b, values b, keys out, values out */
	void* const host[6] = { (void*) keys_a, (void*) values_a, (void*) keys_b, (void*) values_b, keys_out, values_out };
	const size_t bytes[6] = { numel_a * ks, numel_a * vs, numel_b * ks, numel_b * vs, n * ks, n * vs };
	clo_stage st;
	clo_stage_open(&st, m->head.ctx, cq_exec, cq_comm);
	for (int i = 0; i < 4; ++i) clo_stage_in(&st, i, host[i], bytes[i]);
	for (int i = 4; i < 6; ++i) clo_stage_out(&st, i, host[i], bytes[i]);
	if (clo_stage_ok(&st))
		st.evt = clo_merge_with_device_data(m, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], numel_a, st.dev[2], st.dev[3], numel_b,
			st.dev[4], st.dev[5], &st.err);
	for (int i = 4; i < 6; ++i) clo_stage_read(&st, i, host[i], bytes[i]);
	return clo_stage_close(&st, err);
}

CCLContext* clo_merge_get_context(CloMerge* m) {
	clo_return_val_if_fail(m != NULL, NULL);
	return m->head.ctx;
}

CloType clo_merge_get_key_type(CloMerge* m) {
	clo_return_val_if_fail(m != NULL, (CloType) -1);
	return m->key_type;
}

size_t clo_merge_get_key_size(CloMerge* m) {
	clo_return_val_if_fail(m != NULL, 0);
	return clo_type_sizeof(m->key_type);
}

size_t clo_merge_get_value_size(CloMerge* m) {
	clo_return_val_if_fail(m != NULL, 0);
	return m->value_size;
}
