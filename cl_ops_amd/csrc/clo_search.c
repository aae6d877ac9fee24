/*
 * clo_search.c — CloSearch (include/clo_search.h; not upstream): lower and upper bounds of many keys in a sorted
 * array. The kernels are reached through the thin C-ABI (clo_hip_search, include/clo_hip.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_search.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SEARCH_EVENT "clo_search"

struct clo_search {
	CCLContext* ctx;
	CloType key_type;
	clo_devbuf workspace;    /* the tiles' ranges (clo_hip_search_workspace_bytes); grows, never shrinks */
	clo_stream_guard guard;  /* the workspace belongs to one queue at a time */
};

/* 0 unsigned, 1 signed, 2 IEEE total order: the key kinds of clo_sort_by_key_* */
static int search_key_kind(CloType t) {
	if (t == CLO_CHAR || t == CLO_SHORT || t == CLO_INT || t == CLO_LONG) return 1;
	if (t == CLO_HALF || t == CLO_FLOAT || t == CLO_DOUBLE) return 2;
	return 0;
}

CloSearch* clo_search_new(const char* options, CCLContext* ctx, CloType key_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for search (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_search_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_DOUBLE) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Unknown key type %d for search.", (int) key_type);
		return NULL;
	}
	CloSearch* s = (CloSearch*) calloc(1, sizeof(CloSearch));
	if (!s) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	ccl_context_ref(ctx);
	s->ctx = ctx;
	s->key_type = key_type;
	return s;
}

void clo_search_destroy(CloSearch* s) {
	clo_return_if_fail(s != NULL);
	clo_devbuf_release(&s->workspace);
	clo_stream_guard_release(&s->guard);
	ccl_context_unref(s->ctx);
	free(s);
}

static int search_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
	if (!a || !b || !a_bytes || !b_bytes) return 0;
	const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
	return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced. */
static const char* search_refusal(CloSearch* s, const void* haystack, size_t numel_h, const void* needles, size_t numel_n,
	unsigned flags, const void* pos_out) {
	if (flags & ~(CLO_SEARCH_UPPER | CLO_SEARCH_NEEDLES_SORTED)) return "unknown flags (CLO_SEARCH_UPPER, CLO_SEARCH_NEEDLES_SORTED)";
	if (numel_h > 0xffffffffull) return "numel_h must be below 2^32";
	if (numel_n > 0xffffffffull) return "numel_n must be below 2^32";
	if (numel_h > 0 && !haystack) return "haystack is required";
	if (numel_n > 0 && !needles) return "needles is required";
	if (numel_n > 0 && !pos_out) return "pos_out is required";
	const size_t ks = clo_type_sizeof(s->key_type);
	if (search_overlap(pos_out, numel_n * sizeof(cl_uint), haystack, numel_h * ks)
		|| search_overlap(pos_out, numel_n * sizeof(cl_uint), needles, numel_n * ks))
		return "pos_out overlaps an input range (there is no in-place search)";
	return NULL;
}

CCLEvent* clo_search_with_device_data(CloSearch* s, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* haystack, size_t numel_h, CCLBuffer* needles, size_t numel_n, unsigned flags, CCLBuffer* pos_out, GError** err) {
	clo_return_val_if_fail(s != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[3] = { numel_h > 0 ? haystack : NULL, needles, pos_out };   /* the haystack of an empty search is not looked at */
	void* p[3];
	for (int i = 0; i < 3; ++i) p[i] = buf[i] ? ccl_buffer_get_device_ptr(buf[i]) : NULL;
	const char* why = search_refusal(s, p[0], numel_h, p[1], numel_n, flags, p[2]);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(s->key_type);
	const size_t need[3] = { numel_h * ks, numel_n * ks, numel_n * sizeof(cl_uint) };
	for (int i = 0; i < 3; ++i) {
		if (buf[i] && need[i] > ccl_buffer_get_size(buf[i])) {
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_h (%zu) and numel_n (%zu) exceed the size of the device buffers", numel_h, numel_n);
			return NULL;
		}
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SEARCH: %zu needles in %zu keys of type %s, %s bound%s", numel_n, numel_h, clo_type_get_name(s->key_type),
		(flags & CLO_SEARCH_UPPER) ? "upper" : "lower", (flags & CLO_SEARCH_NEEDLES_SORTED) ? ", needles sorted" : "");

	const size_t ws = clo_hip_search_workspace_bytes(numel_h, numel_n, flags);
	if (ws > 0) {
		if (clo_hip_failed(clo_stream_guard_enter(&s->guard, cq_exec), err, "hipStreamWaitEvent")) return NULL;
		if (clo_hip_failed(clo_devbuf_reserve(&s->workspace, ws), err, "hipMalloc(search workspace)")) return NULL;
	}
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SEARCH_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_search(p[0], numel_h, p[1], numel_n, p[2], (int) ks, search_key_kind(s->key_type), flags, 0,
		ws > 0 ? s->workspace.ptr : NULL, ws > 0 ? s->workspace.bytes : 0, ccl_queue_get_stream(cq_exec));
	if (clo_hip_failed(st, err, "clo_hip_search")) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	if (!ccl_queue_end_command(cq_exec, evt, err)) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	return evt;
}

cl_bool clo_search_with_host_data(CloSearch* s, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* haystack, size_t numel_h, const void* needles, size_t numel_n, unsigned flags, void* pos_out, GError** err) {
	clo_return_val_if_fail(s != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	if (numel_h == 0) haystack = NULL;   /* not looked at */
	const char* why = search_refusal(s, haystack, numel_h, needles, numel_n, flags, pos_out);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	if (numel_n == 0) return CL_TRUE;   /* no device needed */

	cl_bool status = CL_FALSE;
	const size_t ks = clo_type_sizeof(s->key_type);
	/* haystack, needles, positions */
	const void* const host[3] = { haystack, needles, pos_out };
	const size_t bytes[3] = { numel_h * ks, numel_n * ks, numel_n * sizeof(cl_uint) };
	CCLBuffer* dev[3] = { NULL, NULL, NULL };
	CCLQueue* intern_queue = NULL;
	CCLEvent* evt = NULL;
	CCLEventWaitList ewl = NULL;
	GError* err_internal = NULL;
	CCLContext* ctx = s->ctx;

	if (cq_exec == NULL) {
		CCLDevice* d = ccl_context_get_device(ctx, 0, &err_internal);
		if (err_internal) goto error_handler;
		intern_queue = ccl_queue_new(ctx, d, 0, &err_internal);
		if (err_internal) goto error_handler;
		cq_exec = intern_queue;
	}
	if (cq_comm == NULL) cq_comm = cq_exec;
	for (int i = 0; i < 3; ++i) {
		if (!host[i] || bytes[i] == 0) continue;
		dev[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i], NULL, &err_internal);
		if (err_internal) goto error_handler;
		if (i < 2) {
			ccl_buffer_enqueue_write(dev[i], cq_comm, CL_TRUE, 0, bytes[i], (void*) host[i], NULL, &err_internal);
			if (err_internal) goto error_handler;
		}
	}
	evt = clo_search_with_device_data(s, cq_exec, cq_comm, dev[0], numel_h, dev[1], numel_n, flags, dev[2], &err_internal);
	if (err_internal) goto error_handler;
	/* waits for the search and blocks */
	ccl_buffer_enqueue_read(dev[2], cq_comm, CL_TRUE, 0, bytes[2], pos_out, evt ? ccl_ewl(&ewl, evt, NULL) : NULL, &err_internal);
	if (err_internal) goto error_handler;
	status = CL_TRUE;
	goto finish;

error_handler:
	clo_gerror_propagate(err, err_internal);
	status = CL_FALSE;

finish:
	ccl_event_wait_list_clear(&ewl);
	for (int i = 0; i < 3; ++i) if (dev[i]) ccl_buffer_destroy(dev[i]);
	if (intern_queue) ccl_queue_destroy(intern_queue);
	return status;
}

CCLContext* clo_search_get_context(CloSearch* s) {
	clo_return_val_if_fail(s != NULL, NULL);
	return s->ctx;
}

CloType clo_search_get_key_type(CloSearch* s) {
	clo_return_val_if_fail(s != NULL, (CloType) -1);
	return s->key_type;
}

size_t clo_search_get_key_size(CloSearch* s) {
	clo_return_val_if_fail(s != NULL, 0);
	return clo_type_sizeof(s->key_type);
}
