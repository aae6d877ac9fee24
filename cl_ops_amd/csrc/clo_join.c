/*
 * clo_join.c — CloJoin (include/clo_join.h; not upstream): the inner, left, right or full outer equi-join of two sorted
 * key arrays as pairs of row indices, in ascending key order. The kernels are reached through the thin C-ABI
 * (clo_hip_join, include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_join.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_JOIN_EVENT "clo_join"

struct clo_join {
	clo_op_head head;        /* the workspace (clo_hip_join_workspace_bytes) */
	int kind;                /* index in join_kinds: what clo_hip_join takes */
	CloType key_type;
};

static const char* const join_kinds[] = { "inner", "left", "right", "full" };

static int join_emits_a(int kind) { return kind == CLO_HIP_JOIN_LEFT || kind == CLO_HIP_JOIN_FULL; }
static int join_emits_b(int kind) { return kind == CLO_HIP_JOIN_RIGHT || kind == CLO_HIP_JOIN_FULL; }

/* one key everywhere (numel_a * numel_b pairs), or no key shared (the unmatched rows the kind emits): whichever is more */
static size_t join_max_rows(int kind, size_t numel_a, size_t numel_b) {
	size_t prod = 0, alone = 0;
	if (numel_a > 0 && numel_b > 0) prod = numel_a > SIZE_MAX / numel_b ? SIZE_MAX : numel_a * numel_b;
	if (join_emits_a(kind)) alone += numel_a;
	if (join_emits_b(kind)) alone = alone + numel_b < alone ? SIZE_MAX : alone + numel_b;
	return prod > alone ? prod : alone;
}

CloJoin* clo_join_new(const char* kind, const char* options, CCLContext* ctx, CloType key_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int ki = clo_name_index(kind, join_kinds, 4);
	if (ki < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown join kind '%s' (one of: " CLO_JOIN_KINDS ").", kind ? kind : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a join (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_join_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for a join.", (int) key_type);
		return NULL;
	}
	CloJoin* jn = (CloJoin*) clo_op_new(sizeof(CloJoin), ctx, err);
	if (!jn) return NULL;
	jn->kind = ki;
	jn->key_type = key_type;
	return jn;
}

void clo_join_destroy(CloJoin* jn) {
	clo_return_if_fail(jn != NULL);
	clo_op_destroy(jn);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * count_bytes: the size of what num_out points to (a cl_ulong of the device, a size_t of the host). */
static const char* join_refusal(CloJoin* jn, const void* keys_a, size_t numel_a, const void* keys_b, size_t numel_b,
	const void* idx_a_out, const void* idx_b_out, const void* keys_out, size_t capacity, const void* num_out, size_t count_bytes) {
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull)
		return "numel_a + numel_b must be below 2^32";
	if (capacity > 0xffffffffull) return "capacity must be below 2^32";
	if (numel_a > 0 && !keys_a) return "keys_a is required";
	if (numel_b > 0 && !keys_b) return "keys_b is required";
	if (!num_out) return "num_out is required";
	if (capacity > 0 && !idx_a_out && !idx_b_out && !keys_out) return "a capacity above 0 with idx_a_out, idx_b_out and keys_out all NULL";
	const size_t ks = clo_type_sizeof(jn->key_type);
	const clo_range in[2] = { { keys_a, numel_a * ks }, { keys_b, numel_b * ks } };
	const clo_range out[4] = { { idx_a_out, capacity * sizeof(cl_uint) }, { idx_b_out, capacity * sizeof(cl_uint) },
		{ keys_out, capacity * ks }, { num_out, count_bytes } };
	switch (clo_ranges_conflict(in, 2, out, 4)) {
		case CLO_RANGES_OUT_IN: return "an output range overlaps an input range";
		case CLO_RANGES_OUT_OUT: return "two output ranges overlap";
	}
	return NULL;
}

CCLEvent* clo_join_with_device_data(CloJoin* jn, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_a, size_t numel_a, CCLBuffer* keys_b, size_t numel_b,
	CCLBuffer* idx_a_out, CCLBuffer* idx_b_out, CCLBuffer* keys_out, size_t capacity, CCLBuffer* num_out, GError** err) {
	clo_return_val_if_fail(jn != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[6] = { keys_a, keys_b, idx_a_out, idx_b_out, keys_out, num_out };
	void* p[6];
	clo_buffers_device_ptrs(buf, p, 6);
	const char* why = join_refusal(jn, p[0], numel_a, p[1], numel_b, p[2], p[3], p[4], capacity, p[5], sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[5] & 7u)) why = "num_out must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(jn->key_type);
	const size_t need[6] = { numel_a * ks, numel_b * ks, capacity * sizeof(cl_uint), capacity * sizeof(cl_uint), capacity * ks, sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 6)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_a (%zu), numel_b (%zu) or capacity (%zu) exceed the size of the device buffers "
			"(num_out holds 8 bytes)", numel_a, numel_b, capacity);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("JOIN: %s of %zu and %zu keys of type %s, capacity %zu%s", join_kinds[jn->kind], numel_a, numel_b, clo_type_get_name(jn->key_type),
		capacity, (!p[2] && !p[3] && !p[4]) ? " (the count form)" : "");

	const size_t ws = clo_hip_join_workspace_bytes(jn->kind, numel_a, numel_b);
	if (ws > 0 && !clo_op_reserve(&jn->head, cq_exec, ws, "hipMalloc(join workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_JOIN_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_join(jn->kind, p[0], numel_a, p[1], numel_b, (uint32_t*) p[2], (uint32_t*) p[3], p[4], capacity, (uint64_t*) p[5],
		(int) ks, clo_type_key_kind(jn->key_type), jn->head.workspace.ptr, jn->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_join", err);
}

cl_bool clo_join_with_host_data(CloJoin* jn, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_a, size_t numel_a, const void* keys_b, size_t numel_b,
	cl_uint* idx_a_out, cl_uint* idx_b_out, void* keys_out, size_t capacity, size_t* num_out, GError** err) {
	clo_return_val_if_fail(jn != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = join_refusal(jn, keys_a, numel_a, keys_b, numel_b, idx_a_out, idx_b_out, keys_out, capacity, num_out, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	*num_out = 0;
	if (numel_a + numel_b == 0) return CL_TRUE;   /* nothing to join: no device needed */

	const size_t ks = clo_type_sizeof(jn->key_type);
	/* keys a, keys b, idx a, idx b, keys out, the count */
	const void* const host[6] = { keys_a, keys_b, idx_a_out, idx_b_out, keys_out, num_out };
	const size_t bytes[6] = { numel_a * ks, numel_b * ks, capacity * sizeof(cl_uint), capacity * sizeof(cl_uint), capacity * ks, sizeof(cl_ulong) };
	cl_ulong k = 0;
	clo_stage st;
	clo_stage_open(&st, jn->head.ctx, cq_exec, cq_comm);
	for (int i = 0; i < 2; ++i) clo_stage_in(&st, i, host[i], bytes[i]);
	for (int i = 2; i < 6; ++i) clo_stage_out(&st, i, host[i], bytes[i]);
	if (clo_stage_ok(&st))
		st.evt = clo_join_with_device_data(jn, st.cq_exec, st.cq_comm, st.dev[0], numel_a, st.dev[1], numel_b,
			st.dev[2], st.dev[3], st.dev[4], capacity, st.dev[5], &st.err);
	/* the count first (blocking): it says how many rows there are to copy */
	clo_stage_read(&st, 5, &k, sizeof(cl_ulong));
	const size_t rows = k < capacity ? (size_t) k : capacity;
	clo_stage_read(&st, 2, idx_a_out, rows * sizeof(cl_uint));
	clo_stage_read(&st, 3, idx_b_out, rows * sizeof(cl_uint));
	clo_stage_read(&st, 4, keys_out, rows * ks);
	if (clo_stage_ok(&st)) *num_out = (size_t) k;
	return clo_stage_close(&st, err);
}

CCLContext* clo_join_get_context(CloJoin* jn) {
	clo_return_val_if_fail(jn != NULL, NULL);
	return jn->head.ctx;
}

CloType clo_join_get_key_type(CloJoin* jn) {
	clo_return_val_if_fail(jn != NULL, (CloType) -1);
	return jn->key_type;
}

size_t clo_join_get_key_size(CloJoin* jn) {
	clo_return_val_if_fail(jn != NULL, 0);
	return clo_type_sizeof(jn->key_type);
}

const char* clo_join_get_kind(CloJoin* jn) {
	clo_return_val_if_fail(jn != NULL, NULL);
	return join_kinds[jn->kind];
}

size_t clo_join_get_max_numel_out(CloJoin* jn, size_t numel_a, size_t numel_b) {
	clo_return_val_if_fail(jn != NULL, 0);
	return join_max_rows(jn->kind, numel_a, numel_b);
}
