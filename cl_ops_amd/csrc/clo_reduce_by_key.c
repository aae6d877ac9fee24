/*
 * clo_reduce_by_key.c — CloReduceByKey (include/clo_reduce.h; not upstream): every run of equal keys collapsed
 * into one row. The kernels are reached through the thin C-ABI (clo_hip_reduce_by_key, include/clo_hip.h); the host
 * layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_reduce.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_REDUCE_BY_KEY_EVENT "clo_reduce_by_key"

struct clo_reduce_by_key {
	clo_op_head head;        /* the workspace: the tile states */
	CloType key_type, value_type, sum_type;
	int op;                  /* index in rbk_ops: what clo_hip_reduce_by_key takes */
};

static const char* const rbk_ops[] = { "sum", "min", "max" };

CloReduceByKey* clo_reduce_by_key_new(const char* op, const char* options, CCLContext* ctx,
	CloType key_type, CloType value_type, CloType sum_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int opi = clo_name_index(op, rbk_ops, 3);
	if (opi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown reduce-by-key operation '%s' (one of: " CLO_REDUCE_BY_KEY_OPS ").",
			op ? op : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for reduce by key.");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_reduce_by_key_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d.", (int) key_type);
		return NULL;
	}
	if (!clo_type_is_int32_or_64(value_type) || !clo_type_is_int32_or_64(sum_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Reduce by key takes values and sums of type int, uint, long or ulong "
			"(floating-point aggregates depend on the order of addition; narrower values are not built), not '%s' into '%s'.",
			clo_type_get_name(value_type) ? clo_type_get_name(value_type) : "?", clo_type_get_name(sum_type) ? clo_type_get_name(sum_type) : "?");
		return NULL;
	}
	if (clo_type_sizeof(sum_type) < clo_type_sizeof(value_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The sum type '%s' is narrower than the value type '%s'.",
			clo_type_get_name(sum_type), clo_type_get_name(value_type));
		return NULL;
	}
	CloReduceByKey* rbk = (CloReduceByKey*) clo_op_new(sizeof(CloReduceByKey), ctx, err);
	if (!rbk) return NULL;
	rbk->key_type = key_type;
	rbk->value_type = value_type;
	rbk->sum_type = sum_type;
	rbk->op = opi;
	return rbk;
}

void clo_reduce_by_key_destroy(CloReduceByKey* rbk) {
	clo_return_if_fail(rbk != NULL);
	clo_op_destroy(rbk);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced.
 * count: the address of the run count (8 bytes), an output like the other two. */
static const char* rbk_refusal(CloReduceByKey* rbk, const void* keys_in, const void* values_in, const void* keys_out,
	const void* aggr_out, const void* count, size_t numel) {
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!count) return "the run count is required";
	if (!keys_out && !aggr_out) return "keys_out and aggr_out cannot both be NULL";
	if (aggr_out && !values_in && rbk->op != 0) return "min / max need values (without values every value is 1: only the sum, the run length, is offered)";
	if (numel > 0 && !keys_in) return "keys_in is required";
	const size_t kb = numel * clo_type_sizeof(rbk->key_type), vb = numel * clo_type_sizeof(rbk->value_type),
		sb = numel * clo_type_sizeof(rbk->sum_type);
	const clo_range in[2] = { { keys_in, kb }, { values_in, vb } };
	const clo_range out[3] = { { keys_out, kb }, { aggr_out, sb }, { count, sizeof(cl_ulong) } };
	switch (clo_ranges_conflict(in, 2, out, 3)) {
		case CLO_RANGES_OUT_IN:
			return "an output range overlaps an input range (rows land below the elements they come from, in tiles that "
				"may not have been read yet: reduce by key does not work in place)";
		case CLO_RANGES_OUT_OUT: return "two output ranges overlap";
	}
	return NULL;
}

CCLEvent* clo_reduce_by_key_with_device_data(CloReduceByKey* rbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out, CCLBuffer* aggr_out,
	CCLBuffer* num_runs_out, size_t numel, GError** err) {
	clo_return_val_if_fail(rbk != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[5] = { keys_in, values_in, keys_out, aggr_out, num_runs_out };
	void* p[5];
	clo_buffers_device_ptrs(buf, p, 5);
	const char* why = rbk_refusal(rbk, p[0], p[1], p[2], p[3], p[4], numel);
	if (!why && ((uintptr_t) p[4] & 7u)) why = "the run count must be 8-byte aligned";
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t kb = numel * clo_type_sizeof(rbk->key_type), vb = numel * clo_type_sizeof(rbk->value_type),
		sb = numel * clo_type_sizeof(rbk->sum_type);
	const size_t need[5] = { kb, vb, kb, sb, sizeof(cl_ulong) };
	if (!clo_buffers_hold(buf, need, 5)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) exceeds the size of the device buffers", numel);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("REDUCE BY KEY: %s, numel=%zu, key %s, values %s, sum %s, keys out %s", rbk_ops[rbk->op], numel,
		clo_type_get_name(rbk->key_type), values_in ? clo_type_get_name(rbk->value_type) : "absent",
		aggr_out ? clo_type_get_name(rbk->sum_type) : "not written", keys_out ? "written" : "not written");

	if (numel > 0 && !clo_op_reserve(&rbk->head, cq_exec, clo_hip_reduce_by_key_workspace_bytes(numel), "hipMalloc(reduce-by-key workspace)", err))
		return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_REDUCE_BY_KEY_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_reduce_by_key(p[0], p[1], p[2], p[3], (uint64_t*) p[4], numel, (int) clo_type_sizeof(rbk->key_type),
		(int) rbk->value_type, (int) rbk->sum_type, rbk->op, rbk->head.workspace.ptr, rbk->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_reduce_by_key", err);
}

cl_bool clo_reduce_by_key_with_host_data(CloReduceByKey* rbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* keys_out, void* aggr_out,
	size_t* num_runs, size_t numel, GError** err) {
	clo_return_val_if_fail(rbk != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = rbk_refusal(rbk, keys_in, values_in, keys_out, aggr_out, num_runs, numel);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	*num_runs = 0;
	if (numel == 0) return CL_TRUE;

	const size_t ks = clo_type_sizeof(rbk->key_type), vs = clo_type_sizeof(rbk->value_type), ss = clo_type_sizeof(rbk->sum_type);
	cl_ulong m = 0;
	/* keys in, values in, keys out, aggregates out, run count */
	clo_stage st;
	clo_stage_open(&st, rbk->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, keys_in, numel * ks);
	clo_stage_in(&st, 1, values_in, numel * vs);
	clo_stage_out(&st, 2, keys_out, numel * ks);
	clo_stage_out(&st, 3, aggr_out, numel * ss);
	clo_stage_out(&st, 4, num_runs, sizeof(cl_ulong));
	if (clo_stage_ok(&st))
		st.evt = clo_reduce_by_key_with_device_data(rbk, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4], numel, &st.err);
	/* the run count first (blocking): it says how many rows there are to copy */
	clo_stage_read(&st, 4, &m, sizeof(cl_ulong));
	if (clo_stage_ok(&st) && m > numel)
		clo_gerror_set(&st.err, CLO_ERROR, CLO_ERROR_LIBRARY, "reduce by key: %llu runs of %zu elements", (unsigned long long) m, numel);
	clo_stage_read(&st, 2, keys_out, (size_t) m * ks);
	clo_stage_read(&st, 3, aggr_out, (size_t) m * ss);
	if (clo_stage_ok(&st)) *num_runs = (size_t) m;
	return clo_stage_close(&st, err);
}

CCLContext* clo_reduce_by_key_get_context(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, NULL);
	return rbk->head.ctx;
}

CloType clo_reduce_by_key_get_key_type(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, (CloType) -1);
	return rbk->key_type;
}

size_t clo_reduce_by_key_get_key_size(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, 0);
	return clo_type_sizeof(rbk->key_type);
}

CloType clo_reduce_by_key_get_value_type(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, (CloType) -1);
	return rbk->value_type;
}

size_t clo_reduce_by_key_get_value_size(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, 0);
	return clo_type_sizeof(rbk->value_type);
}

CloType clo_reduce_by_key_get_sum_type(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, (CloType) -1);
	return rbk->sum_type;
}

size_t clo_reduce_by_key_get_sum_size(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, 0);
	return clo_type_sizeof(rbk->sum_type);
}

const char* clo_reduce_by_key_get_op(CloReduceByKey* rbk) {
	clo_return_val_if_fail(rbk != NULL, NULL);
	return rbk_ops[rbk->op];
}
