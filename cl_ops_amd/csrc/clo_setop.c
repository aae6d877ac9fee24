/*
 * clo_setop.c — CloSetOp (include/clo_setop.h; not upstream): union, intersection, difference and symmetric
 * difference of two sorted arrays as multisets, with values or as indices. The kernels are reached through the thin
 * C-ABI (clo_hip_setop, include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_setop.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SETOP_EVENT "clo_setop"

struct clo_setop {
	clo_op_head head;        /* the workspace: split points and kept counts (clo_hip_setop_workspace_bytes) */
	int op;                  /* index in setop_ops: what clo_hip_setop takes */
	CloType key_type;
	size_t value_size;
};

static const char* const setop_ops[] = { "union", "intersection", "difference", "symmetric_difference" };

/* union and symmetric difference keep elements of B; the other two never look at values_b */
static int setop_keeps_b(int op) { return op == CLO_HIP_SETOP_UNION || op == CLO_HIP_SETOP_SYMMETRIC_DIFFERENCE; }

static size_t setop_capacity(int op, size_t numel_a, size_t numel_b) {
	if (setop_keeps_b(op)) return numel_a + numel_b;
	if (op == CLO_HIP_SETOP_DIFFERENCE) return numel_a;
	return numel_a < numel_b ? numel_a : numel_b;
}

CloSetOp* clo_setop_new(const char* op, const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int opi = clo_name_index(op, setop_ops, 4);
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown set operation '%s' (one of: " CLO_SETOP_OPS ").", op ? op : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a set operation (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_setop_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for a set operation.", (int) key_type);
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A set operation carries values of 0 (none), 4 or 8 bytes, not a value_size of %zu.", value_size);
		return NULL;
	}
	CloSetOp* so = (CloSetOp*) clo_op_new(sizeof(CloSetOp), ctx, err);
	if (!so) return NULL;
	so->op = opi;
	so->key_type = key_type;
	so->value_size = value_size;
	return so;
}

void clo_setop_destroy(CloSetOp* so) {
	clo_return_if_fail(so != NULL);
	clo_op_destroy(so);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * count_bytes: the size of what num_out points to (a cl_ulong of the device, a size_t of the host). */
static const char* setop_refusal(CloSetOp* so, const void* keys_a, const void* values_a, size_t numel_a,
	const void* keys_b, const void* values_b, size_t numel_b, const void* keys_out, const void* values_out,
	const void* num_out, size_t count_bytes) {
	if (numel_a > 0xffffffffull || numel_b > 0xffffffffull || numel_a + numel_b > 0xffffffffull)
		return "numel_a + numel_b must be below 2^32";
	if (numel_a > 0 && !keys_a) return "keys_a is required";
	if (numel_b > 0 && !keys_b) return "keys_b is required";
	if (!num_out) return "num_out is required";
	if (!keys_out && !values_out) return "keys_out and values_out are both NULL";
	if (so->value_size == 0 && (values_a || values_b || values_out)) return "values passed to a set operation made with value_size 0";
	if (so->value_size > 0 && !values_out) return "values_out is required with a value_size above 0";
	const int keeps_b = setop_keeps_b(so->op);
	if (keeps_b && numel_a > 0 && numel_b > 0 && (values_a == NULL) != (values_b == NULL))
		return "values_a and values_b must both be given, or both be NULL (the arg form)";
	if (so->value_size == 8 && ((numel_a > 0 && !values_a) || (keeps_b && numel_b > 0 && !values_b)))
		return "NULL values (the arg form) need a value_size of 4: the indices are written as uint";
	const size_t ks = clo_type_sizeof(so->key_type), vs = so->value_size, cap = setop_capacity(so->op, numel_a, numel_b);
	const clo_range in[4] = { { keys_a, numel_a * ks }, { keys_b, numel_b * ks }, { values_a, numel_a * vs },
		{ keeps_b ? values_b : NULL, numel_b * vs } };
	const clo_range out[3] = { { keys_out, cap * ks }, { values_out, cap * vs }, { num_out, count_bytes } };
	switch (clo_ranges_conflict(in, 4, out, 3)) {
		case CLO_RANGES_OUT_IN: return "an output range overlaps an input range (there is no in-place set operation)";
		case CLO_RANGES_OUT_OUT: return "two output ranges overlap";
	}
	return NULL;
}

CCLEvent* clo_setop_with_device_data(CloSetOp* so, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_a, CCLBuffer* values_a, size_t numel_a, CCLBuffer* keys_b, CCLBuffer* values_b, size_t numel_b,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* num_out, GError** err) {
	clo_return_val_if_fail(so != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[7] = { keys_a, values_a, keys_b, values_b, keys_out, values_out, num_out };
	void* p[7];
	clo_buffers_device_ptrs(buf, p, 7);
	const char* why = setop_refusal(so, p[0], p[1], numel_a, p[2], p[3], numel_b, p[4], p[5], p[6], sizeof(cl_ulong));
	if (!why && ((uintptr_t) p[6] & 7u)) why = "num_out must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const int keeps_b = setop_keeps_b(so->op);
	const size_t ks = clo_type_sizeof(so->key_type), vs = so->value_size, cap = setop_capacity(so->op, numel_a, numel_b);
	const size_t need[7] = { numel_a * ks, numel_a * vs, numel_b * ks, keeps_b ? numel_b * vs : 0, cap * ks, cap * vs, sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 7)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_a (%zu) and numel_b (%zu) exceed the size of the device buffers "
			"(the outputs hold %zu elements, num_out 8 bytes)", numel_a, numel_b, cap);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SETOP: %s of %zu + %zu keys of type %s, %s", setop_ops[so->op], numel_a, numel_b, clo_type_get_name(so->key_type),
		vs == 0 ? "no values" : ((numel_a > 0 && !p[1]) || (keeps_b && numel_b > 0 && !p[3])) ? "indices" : vs == 4 ? "4-byte values" : "8-byte values");

	const size_t ws = clo_hip_setop_workspace_bytes(numel_a, numel_b);
	if (ws > 0 && !clo_op_reserve(&so->head, cq_exec, ws, "hipMalloc(setop workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SETOP_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_setop(so->op, p[0], p[1], numel_a, p[2], keeps_b ? p[3] : NULL, numel_b, p[4], p[5], (uint64_t*) p[6],
		(int) ks, clo_type_key_kind(so->key_type), (int) vs, so->head.workspace.ptr, so->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_setop", err);
}

cl_bool clo_setop_with_host_data(CloSetOp* so, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_a, const void* values_a, size_t numel_a, const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, size_t* num_out, GError** err) {
	clo_return_val_if_fail(so != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = setop_refusal(so, keys_a, values_a, numel_a, keys_b, values_b, numel_b, keys_out, values_out, num_out, sizeof(size_t));
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	*num_out = 0;
	const size_t cap = setop_capacity(so->op, numel_a, numel_b);
	if (cap == 0) return CL_TRUE;   /* nothing can be kept: no device needed */

	const size_t ks = clo_type_sizeof(so->key_type), vs = so->value_size;
	/* keys a, values a, keys b, values b, keys out, values out, the count */
	const void* const host[7] = { keys_a, values_a, keys_b, setop_keeps_b(so->op) ? values_b : NULL, keys_out, values_out, num_out };
	const size_t bytes[7] = { numel_a * ks, numel_a * vs, numel_b * ks, numel_b * vs, cap * ks, cap * vs, sizeof(cl_ulong) };
	cl_ulong k = 0;
	clo_stage st;
	clo_stage_open(&st, so->head.ctx, cq_exec, cq_comm);
	for (int i = 0; i < 4; ++i) clo_stage_in(&st, i, host[i], bytes[i]);
	for (int i = 4; i < 7; ++i) clo_stage_out(&st, i, host[i], bytes[i]);
	if (clo_stage_ok(&st))
		st.evt = clo_setop_with_device_data(so, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], numel_a, st.dev[2], st.dev[3], numel_b,
			st.dev[4], st.dev[5], st.dev[6], &st.err);
	/* the count first (blocking): it says how many rows there are to copy */
	clo_stage_read(&st, 6, &k, sizeof(cl_ulong));
	if (clo_stage_ok(&st) && k > cap)
		clo_gerror_set(&st.err, CLO_ERROR, CLO_ERROR_LIBRARY, "set operation: %llu rows in outputs of %zu", (unsigned long long) k, cap);
	clo_stage_read(&st, 4, keys_out, (size_t) k * ks);
	clo_stage_read(&st, 5, values_out, (size_t) k * vs);
	if (clo_stage_ok(&st)) *num_out = (size_t) k;
	return clo_stage_close(&st, err);
}

CCLContext* clo_setop_get_context(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, NULL);
	return so->head.ctx;
}

CloType clo_setop_get_key_type(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, (CloType) -1);
	return so->key_type;
}

size_t clo_setop_get_key_size(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, 0);
	return clo_type_sizeof(so->key_type);
}

size_t clo_setop_get_value_size(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, 0);
	return so->value_size;
}

const char* clo_setop_get_op(CloSetOp* so) {
	clo_return_val_if_fail(so != NULL, NULL);
	return setop_ops[so->op];
}

size_t clo_setop_get_max_numel_out(CloSetOp* so, size_t numel_a, size_t numel_b) {
	clo_return_val_if_fail(so != NULL, 0);
	return setop_capacity(so->op, numel_a, numel_b);
}
