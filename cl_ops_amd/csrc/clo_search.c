/*
 * clo_search.c — CloSearch (include/clo_search.h; not upstream): lower and upper bounds of many keys in a sorted
 * array. The kernels are reached through the thin C-ABI (clo_hip_search, include/clo_hip.h); the host layer is the
 * one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_search.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_SEARCH_EVENT "clo_search"

struct clo_search {
	clo_op_head head;        /* the workspace: the tiles' ranges (clo_hip_search_workspace_bytes) */
	CloType key_type;
};

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
	CloSearch* s = (CloSearch*) clo_op_new(sizeof(CloSearch), ctx, err);
	if (!s) return NULL;
	s->key_type = key_type;
	return s;
}

void clo_search_destroy(CloSearch* s) {
	clo_return_if_fail(s != NULL);
	clo_op_destroy(s);
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
	const clo_range in[2] = { { haystack, numel_h * ks }, { needles, numel_n * ks } };
	const clo_range out = { pos_out, numel_n * sizeof(cl_uint) };
	if (clo_ranges_conflict(in, 2, &out, 1)) return "pos_out overlaps an input range (there is no in-place search)";
	return NULL;
}

CCLEvent* clo_search_with_device_data(CloSearch* s, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* haystack, size_t numel_h, CCLBuffer* needles, size_t numel_n, unsigned flags, CCLBuffer* pos_out, GError** err) {
	clo_return_val_if_fail(s != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[3] = { numel_h > 0 ? haystack : NULL, needles, pos_out };   /* the haystack of an empty search is not looked at */
	void* p[3];
	clo_buffers_device_ptrs(buf, p, 3);
	const char* why = search_refusal(s, p[0], numel_h, p[1], numel_n, flags, p[2]);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(s->key_type);
	const size_t need[3] = { numel_h * ks, numel_n * ks, numel_n * sizeof(cl_uint) };
	if (!clo_buffers_hold(buf, need, 3)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel_h (%zu) and numel_n (%zu) exceed the size of the device buffers", numel_h, numel_n);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("SEARCH: %zu needles in %zu keys of type %s, %s bound%s", numel_n, numel_h, clo_type_get_name(s->key_type),
		(flags & CLO_SEARCH_UPPER) ? "upper" : "lower", (flags & CLO_SEARCH_NEEDLES_SORTED) ? ", needles sorted" : "");

	const size_t ws = clo_hip_search_workspace_bytes(numel_h, numel_n, flags);
	if (ws > 0 && !clo_op_reserve(&s->head, cq_exec, ws, "hipMalloc(search workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_SEARCH_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_search(p[0], numel_h, p[1], numel_n, p[2], (int) ks, clo_type_key_kind(s->key_type), flags, 0,
		ws > 0 ? s->head.workspace.ptr : NULL, ws > 0 ? s->head.workspace.bytes : 0, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_search", err);
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

	const size_t ks = clo_type_sizeof(s->key_type);
	/* haystack, needles, positions */
	clo_stage st;
	clo_stage_open(&st, s->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, haystack, numel_h * ks);
	clo_stage_in(&st, 1, needles, numel_n * ks);
	clo_stage_out(&st, 2, pos_out, numel_n * sizeof(cl_uint));
	if (clo_stage_ok(&st))
		st.evt = clo_search_with_device_data(s, st.cq_exec, st.cq_comm, st.dev[0], numel_h, st.dev[1], numel_n, flags, st.dev[2], &st.err);
	clo_stage_read(&st, 2, pos_out, numel_n * sizeof(cl_uint));   /* waits for the search and blocks */
	return clo_stage_close(&st, err);
}

CCLContext* clo_search_get_context(CloSearch* s) {
	clo_return_val_if_fail(s != NULL, NULL);
	return s->head.ctx;
}

CloType clo_search_get_key_type(CloSearch* s) {
	clo_return_val_if_fail(s != NULL, (CloType) -1);
	return s->key_type;
}

size_t clo_search_get_key_size(CloSearch* s) {
	clo_return_val_if_fail(s != NULL, 0);
	return clo_type_sizeof(s->key_type);
}
