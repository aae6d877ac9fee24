/*
 * clo_topk.c — CloTopK (include/clo_topk.h; not upstream): the k smallest or largest keys, with values or as indices,
 * and the k-th key. The kernels are reached through the thin C-ABI (clo_hip_topk, include/clo_hip.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_topk.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_TOPK_EVENT "clo_topk"

struct clo_topk {
	CCLContext* ctx;
	int which;               /* index in topk_which: what clo_hip_topk takes */
	int order;               /* index in topk_orders, likewise */
	CloType key_type;
	size_t value_size;
	clo_devbuf workspace;    /* clo_hip_topk_workspace_bytes; grows, never shrinks */
	clo_stream_guard guard;  /* the workspace belongs to one queue at a time */
};

static const char* const topk_which[] = { "smallest", "largest" };
static const char* const topk_orders[] = { "input", "sorted" };

/* 0 unsigned, 1 signed, 2 IEEE total order: the key kinds of clo_sort_by_key_* */
static int topk_key_kind(CloType t) {
	if (t == CLO_CHAR || t == CLO_SHORT || t == CLO_INT || t == CLO_LONG) return 1;
	if (t == CLO_HALF || t == CLO_FLOAT || t == CLO_DOUBLE) return 2;
	return 0;
}

static int topk_index(const char* name, const char* const* names, int count) {
	for (int i = 0; name && i < count; ++i)
		if (!strcmp(name, names[i])) return i;
	return -1;
}

CloTopK* clo_topk_new(const char* which, const char* order, const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	const int whichi = topk_index(which, topk_which, 2), orderi = topk_index(order, topk_orders, 2);
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
	CloTopK* topk = (CloTopK*) calloc(1, sizeof(CloTopK));
	if (!topk) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	ccl_context_ref(ctx);
	topk->ctx = ctx;
	topk->which = whichi;
	topk->order = orderi;
	topk->key_type = key_type;
	topk->value_size = value_size;
	return topk;
}

void clo_topk_destroy(CloTopK* topk) {
	clo_return_if_fail(topk != NULL);
	clo_devbuf_release(&topk->workspace);
	clo_stream_guard_release(&topk->guard);
	ccl_context_unref(topk->ctx);
	free(topk);
}

typedef struct { const void* p; size_t bytes; } topk_range;

static int topk_overlap(topk_range a, topk_range b) {
	if (!a.p || !b.p || !a.bytes || !b.bytes) return 0;
	const uintptr_t a0 = (uintptr_t) a.p, b0 = (uintptr_t) b.p;
	return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
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
	const topk_range in[2] = { { keys_in, numel * ks }, { values_in, numel * vs } };
	const topk_range out[3] = { { keys_out, m * ks }, { values_out, m * vs }, { kth_out, m ? ks : 0 } };
	for (int o = 0; o < 3; ++o) {
		for (int i = 0; i < 2; ++i)
			if (topk_overlap(out[o], in[i])) return "an output range overlaps an input range (there is no in-place top-k)";
		for (int p = 0; p < o; ++p)
			if (topk_overlap(out[o], out[p])) return "two output ranges overlap";
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
	for (int i = 0; i < 5; ++i) p[i] = buf[i] ? ccl_buffer_get_device_ptr(buf[i]) : NULL;
	const char* why = topk_refusal(topk, p[0], p[1], p[2], p[3], p[4], numel, k);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(topk->key_type), vs = topk->value_size;
	const size_t m = k < numel ? k : numel;
	const size_t need[5] = { numel * ks, numel * vs, m * ks, m * vs, ks };
	for (int i = 0; i < 5; ++i) {
		if (buf[i] && need[i] > ccl_buffer_get_size(buf[i])) {
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) or min(k, numel) (%zu) exceeds the size of the device buffers (the inputs hold "
				"numel rows, the outputs min(k, numel) rows, kth_out one key)", numel, m);
			return NULL;
		}
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("TOPK: the %zu %s of %zu keys of type %s in %s order, %s", m, topk_which[topk->which], numel, clo_type_get_name(topk->key_type),
		topk_orders[topk->order], vs == 0 ? "no values" : !p[1] ? "indices" : vs == 4 ? "4-byte values" : "8-byte values");

	const size_t ws = m ? clo_hip_topk_workspace_bytes(numel, (int) ks, (int) vs) : 0;
	if (ws > 0) {
		if (clo_hip_failed(clo_stream_guard_enter(&topk->guard, cq_exec), err, "hipStreamWaitEvent")) return NULL;
		if (clo_hip_failed(clo_devbuf_reserve(&topk->workspace, ws), err, "hipMalloc(top-k workspace)")) return NULL;
	}
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_TOPK_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_topk(topk->which, topk->order, p[0], p[1], p[2], p[3], p[4], numel, k,
		(int) ks, topk_key_kind(topk->key_type), (int) vs, topk->workspace.ptr, topk->workspace.bytes, ccl_queue_get_stream(cq_exec));
	if (clo_hip_failed(st, err, "clo_hip_topk")) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	if (!ccl_queue_end_command(cq_exec, evt, err)) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	return evt;
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

	cl_bool status = CL_FALSE;
	const size_t ks = clo_type_sizeof(topk->key_type), vs = topk->value_size;
	/* keys, values, keys out, values out, the k-th key */
	const void* const host[5] = { keys_in, values_in, keys_out, values_out, kth_out };
	const size_t bytes[5] = { numel * ks, numel * vs, m * ks, m * vs, ks };
	CCLBuffer* dev[5] = { NULL, NULL, NULL, NULL, NULL };
	CCLQueue* intern_queue = NULL;
	CCLEvent* evt = NULL;
	CCLEventWaitList ewl = NULL;
	GError* err_internal = NULL;
	CCLContext* ctx = topk->ctx;

	if (cq_exec == NULL) {
		CCLDevice* d = ccl_context_get_device(ctx, 0, &err_internal);
		if (err_internal) goto error_handler;
		intern_queue = ccl_queue_new(ctx, d, 0, &err_internal);
		if (err_internal) goto error_handler;
		cq_exec = intern_queue;
	}
	if (cq_comm == NULL) cq_comm = cq_exec;
	for (int i = 0; i < 5; ++i) {
		if (!host[i] || bytes[i] == 0) continue;
		dev[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i], NULL, &err_internal);
		if (err_internal) goto error_handler;
		if (i < 2) {
			ccl_buffer_enqueue_write(dev[i], cq_comm, CL_TRUE, 0, bytes[i], (void*) host[i], NULL, &err_internal);
			if (err_internal) goto error_handler;
		}
	}
	evt = clo_topk_with_device_data(topk, cq_exec, cq_comm, dev[0], dev[1], dev[2], dev[3], dev[4], numel, k, &err_internal);
	if (err_internal) goto error_handler;
	for (int i = 2; i < 5; ++i) {
		if (!dev[i]) continue;
		ccl_buffer_enqueue_read(dev[i], cq_comm, CL_TRUE, 0, bytes[i], (void*) host[i], evt ? ccl_ewl(&ewl, evt, NULL) : NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	status = CL_TRUE;
	goto finish;

error_handler:
	clo_gerror_propagate(err, err_internal);
	status = CL_FALSE;

finish:
	ccl_event_wait_list_clear(&ewl);
	for (int i = 0; i < 5; ++i) if (dev[i]) ccl_buffer_destroy(dev[i]);
	if (intern_queue) ccl_queue_destroy(intern_queue);
	return status;
}

CCLContext* clo_topk_get_context(CloTopK* topk) {
	clo_return_val_if_fail(topk != NULL, NULL);
	return topk->ctx;
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
