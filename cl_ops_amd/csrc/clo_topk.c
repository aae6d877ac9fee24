/*
 * clo_topk.c — CloTopK (include/clo_topk.h; not upstream): the k smallest or largest keys, with values or as indices,
 * and the k-th key. The kernels are reached through the thin C-ABI (clo_hip_topk, include/clo_hip.h); the host layer
 * is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_topk.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_TOPK_EVENT "clo_topk"

struct clo_topk {
	clo_op_head head;        /* the workspace: clo_hip_topk_workspace_bytes */
	int which;               /* index in topk_which: what clo_hip_topk takes */
	int order;               /* index in topk_orders, likewise */
	CloType key_type;
	size_t value_size;
};

static const char* const topk_which[] = { "smallest", "largest" };
static const char* const topk_orders[] = { "input", "sorted" };

CloTopK* clo_topk_new(const char* which, const char* order, const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int whichi = clo_name_index(which, topk_which, 2), orderi = clo_name_index(order, topk_orders, 2);
	if (whichi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown top-k which '%s' (one of: " CLO_TOPK_WHICH ").", which ? which : "(null)");
		return NULL;
	}
	if (orderi < 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown top-k order '%s' (one of: " CLO_TOPK_ORDERS ").", order ? order : "(null)");
		return NULL;
	}
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a top-k (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_topk_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for a top-k.", (int) key_type);
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A top-k carries values of 0 (none), 4 or 8 bytes, not a value_size of %zu.", value_size);
		return NULL;
	}
	CloTopK* topk = (CloTopK*) clo_op_new(sizeof(CloTopK), ctx, err);
	if (!topk) return NULL;
	topk->which = whichi;
	topk->order = orderi;
	topk->key_type = key_type;
	topk->value_size = value_size;
	return topk;
}

void clo_topk_destroy(CloTopK* topk) {
	clo_return_if_fail(topk != NULL);
	clo_op_destroy(topk);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced. */
static const char* topk_refusal(CloTopK* topk, const void* keys_in, const void* values_in,
	const void* keys_out, const void* values_out, const void* kth_out, size_t numel, size_t k) {
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (!keys_out && !values_out && !kth_out) return "keys_out and values_out are both NULL and so is kth_out";
	if (topk->value_size == 0 && (values_in || values_out)) return "values passed to a top-k made with value_size 0";
	if (topk->value_size > 0 && !values_out) return "values_out is required with a value_size above 0";
	if (topk->value_size == 8 && !values_in) return "NULL values_in (the arg form) needs a value_size of 4: the indices are written as uint";
	if (numel > 0 && !keys_in) return "keys_in is required";
	const size_t ks = clo_type_sizeof(topk->key_type), vs = topk->value_size;
	if (kth_out && (uintptr_t) kth_out % ks) return "kth_out must be aligned to the key";
	const size_t m = k < numel ? k : numel;
	if (topk->order == CLO_HIP_TOPK_SORTED && m > clo_hip_topk_sorted_max((int) ks, (int) vs))
		return "min(k, numel) is above the cap of the sorted order (clo_hip_topk_sorted_max): take the input order and sort the rows";
	const clo_range in[2] = { { keys_in, numel * ks }, { values_in, numel * vs } };
	const clo_range out[3] = { { keys_out, m * ks }, { values_out, m * vs }, { kth_out, m ? ks : 0 } };
	switch (clo_ranges_conflict(in, 2, out, 3)) {
		case CLO_RANGES_OUT_IN: return "an output range overlaps an input range (there is no in-place top-k)";
		case CLO_RANGES_OUT_OUT: return "two output ranges overlap";
	}
	return NULL;
}

CCLEvent* clo_topk_with_device_data(CloTopK* topk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* kth_out,
	size_t numel, size_t k, GError** err) {
	clo_return_val_if_fail(topk != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[5] = { keys_in, values_in, keys_out, values_out, kth_out };
	void* p[5];
	clo_buffers_device_ptrs(buf, p, 5);
	const char* why = topk_refusal(topk, p[0], p[1], p[2], p[3], p[4], numel, k);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(topk->key_type), vs = topk->value_size;
	const size_t m = k < numel ? k : numel;
	const size_t need[5] = { numel * ks, numel * vs, m * ks, m * vs, ks };
	if (!clo_buffers_hold(buf, need, 5)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) or min(k, numel) (%zu) exceeds the size of the device buffers (the inputs hold "
			"numel rows, the outputs min(k, numel) rows, kth_out one key)", numel, m);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("TOPK: the %zu %s of %zu keys of type %s in %s order, %s", m, topk_which[topk->which], numel, clo_type_get_name(topk->key_type),
		topk_orders[topk->order], vs == 0 ? "no values" : !p[1] ? "indices" : vs == 4 ? "4-byte values" : "8-byte values");

	const size_t ws = m ? clo_hip_topk_workspace_bytes(numel, (int) ks, (int) vs) : 0;
	if (ws > 0 && !clo_op_reserve(&topk->head, cq_exec, ws, "hipMalloc(top-k workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_TOPK_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_topk(topk->which, topk->order, p[0], p[1], p[2], p[3], p[4], numel, k,
		(int) ks, clo_type_key_kind(topk->key_type), (int) vs, topk->head.workspace.ptr, topk->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_topk", err);
}

cl_bool clo_topk_with_host_data(CloTopK* topk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* kth_out,
	size_t numel, size_t k, GError** err) {
	clo_return_val_if_fail(topk != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = topk_refusal(topk, keys_in, values_in, keys_out, values_out, kth_out, numel, k);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const size_t m = k < numel ? k : numel;
	if (m == 0) return CL_TRUE;   /* nothing is chosen: no device needed */

	const size_t ks = clo_type_sizeof(topk->key_type), vs = topk->value_size;
	/* keys, values, keys out, values out, the k-th key */
	void* const host[5] = { (void*) keys_in, (void*) values_in, keys_out, values_out, kth_out };
	const size_t bytes[5] = { numel * ks, numel * vs, m * ks, m * vs, ks };
	clo_stage st;
	clo_stage_open(&st, topk->head.ctx, cq_exec, cq_comm);
	for (int i = 0; i < 2; ++i) clo_stage_in(&st, i, host[i], bytes[i]);
	for (int i = 2; i < 5; ++i) clo_stage_out(&st, i, host[i], bytes[i]);
	if (clo_stage_ok(&st))
		st.evt = clo_topk_with_device_data(topk, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4], numel, k, &st.err);
	for (int i = 2; i < 5; ++i) clo_stage_read(&st, i, host[i], bytes[i]);
	return clo_stage_close(&st, err);
}

CCLContext* clo_topk_get_context(CloTopK* topk) {
	clo_return_val_if_fail(topk != NULL, NULL);
	return topk->head.ctx;
}

CloType clo_topk_get_key_type(CloTopK* topk) {
	clo_return_val_if_fail(topk != NULL, (CloType) -1);
	return topk->key_type;
}

size_t clo_topk_get_key_size(CloTopK* topk) {
	clo_return_val_if_fail(topk != NULL, 0);
	return clo_type_sizeof(topk->key_type);
}

size_t clo_topk_get_value_size(CloTopK* topk) {
	clo_return_val_if_fail(topk != NULL, 0);
	return topk->value_size;
}

const char* clo_topk_get_which(CloTopK* topk) {
	clo_return_val_if_fail(topk != NULL, NULL);
	return topk_which[topk->which];
}

const char* clo_topk_get_order(CloTopK* topk) {
	clo_return_val_if_fail(topk != NULL, NULL);
	return topk_orders[topk->order];
}
