/*
 * clo_histogram.c — CloHistogram (include/clo_histogram.h; not upstream): counts or sums of values per bin of
 * integer keys. The kernels are reached through the thin C-ABI (clo_hip_histogram, include/clo_hip.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_histogram.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_HISTOGRAM_EVENT "clo_histogram"

struct clo_histogram {
	CCLContext* ctx;
	CloType key_type, value_type, sum_type;
	int accumulate;
	clo_devbuf workspace;    /* what clo_hip_histogram_workspace_bytes asks for (nothing today); grows, never shrinks */
	clo_stream_guard guard;  /* the workspace belongs to one queue at a time */
};

static int hist_value_type_ok(CloType t) { return t == CLO_INT || t == CLO_UINT || t == CLO_LONG || t == CLO_ULONG; }
static int hist_key_signed(CloType t) { return t == CLO_CHAR || t == CLO_SHORT || t == CLO_INT || t == CLO_LONG; }

CloHistogram* clo_histogram_new(const char* options, CCLContext* ctx,
	CloType key_type, CloType value_type, CloType sum_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	int accumulate = 0;
	if (options != NULL && strlen(options) > 0) {
		if (strcmp(options, "accumulate") != 0) {
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for histogram (NULL, \"\" or \"accumulate\").");
			return NULL;
		}
		accumulate = 1;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_histogram_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Histogram keys are integers (char .. ulong), not '%s': the bin edges of "
			"floating-point keys need a rounding contract.", clo_type_get_name(key_type) ? clo_type_get_name(key_type) : "?");
		return NULL;
	}
	if (!hist_value_type_ok(value_type) || !hist_value_type_ok(sum_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Histogram takes values and sums of type int, uint, long or ulong, not '%s' into '%s'.",
			clo_type_get_name(value_type) ? clo_type_get_name(value_type) : "?", clo_type_get_name(sum_type) ? clo_type_get_name(sum_type) : "?");
		return NULL;
	}
	if (clo_type_sizeof(sum_type) < clo_type_sizeof(value_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The sum type '%s' is narrower than the value type '%s'.",
			clo_type_get_name(sum_type), clo_type_get_name(value_type));
		return NULL;
	}
	CloHistogram* hist = (CloHistogram*) calloc(1, sizeof(CloHistogram));
	if (!hist) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Out of host memory.");
		return NULL;
	}
	ccl_context_ref(ctx);
	hist->ctx = ctx;
	hist->key_type = key_type;
	hist->value_type = value_type;
	hist->sum_type = sum_type;
	hist->accumulate = accumulate;
	return hist;
}

void clo_histogram_destroy(CloHistogram* hist) {
	clo_return_if_fail(hist != NULL);
	clo_devbuf_release(&hist->workspace);
	clo_stream_guard_release(&hist->guard);
	ccl_context_unref(hist->ctx);
	free(hist);
}

static int hist_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
	if (!a || !b || !abytes || !bbytes) return 0;
	const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
	return a0 < b0 + bbytes && b0 < a0 + abytes;
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced. */
static const char* hist_refusal(CloHistogram* hist, const void* keys_in, const void* values_in, const void* hist_out,
	size_t numel, unsigned shift, size_t num_bins) {
	if (numel > 0xffffffffull) return "numel must be below 2^32 (larger arrays: pieces, with the option \"accumulate\")";
	if (num_bins == 0) return "num_bins must not be 0";
	if (num_bins > 0xffffffffull) return "num_bins must be below 2^32";
	if (shift >= 8u * clo_type_sizeof(hist->key_type)) return "shift must be below the number of bits of the key type";
	if (!hist_out) return "hist_out is required";
	if (numel > 0 && !keys_in) return "keys_in is required";
	const size_t hb = num_bins * clo_type_sizeof(hist->sum_type);
	if (hist_overlap(hist_out, hb, keys_in, numel * clo_type_sizeof(hist->key_type))
		|| hist_overlap(hist_out, hb, values_in, numel * clo_type_sizeof(hist->value_type)))
		return "the hist_out range overlaps an input range";
	return NULL;
}

/* *lower as the bits the thin ABI takes: the low key-size bytes of a uint64 (little-endian host, as the device) */
static uint64_t hist_lower_bits(CloHistogram* hist, const void* lower) {
	uint64_t bits = 0;
	if (lower) memcpy(&bits, lower, clo_type_sizeof(hist->key_type));
	return bits;
}

CCLEvent* clo_histogram_with_device_data(CloHistogram* hist, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* hist_out,
	size_t numel, const void* lower, unsigned shift, size_t num_bins, GError** err) {
	clo_return_val_if_fail(hist != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	void* kin = keys_in ? ccl_buffer_get_device_ptr(keys_in) : NULL;
	void* vin = values_in ? ccl_buffer_get_device_ptr(values_in) : NULL;
	void* out = hist_out ? ccl_buffer_get_device_ptr(hist_out) : NULL;
	const char* why = hist_refusal(hist, kin, vin, out, numel, shift, num_bins);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(hist->key_type), vs = clo_type_sizeof(hist->value_type), ss = clo_type_sizeof(hist->sum_type);
	if ((keys_in && numel * ks > ccl_buffer_get_size(keys_in)) || (values_in && numel * vs > ccl_buffer_get_size(values_in))
		|| num_bins * ss > ccl_buffer_get_size(hist_out)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) or num_bins (%zu) exceeds the size of the device buffers", numel, num_bins);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("HISTOGRAM: numel=%zu, key %s, values %s, sum %s, shift %u, %zu bins%s", numel, clo_type_get_name(hist->key_type),
		values_in ? clo_type_get_name(hist->value_type) : "absent", clo_type_get_name(hist->sum_type), shift, num_bins,
		hist->accumulate ? ", accumulating" : "");

	const size_t ws = clo_hip_histogram_workspace_bytes(numel, num_bins);
	if (ws > 0) {
		if (clo_hip_failed(clo_stream_guard_enter(&hist->guard, cq_exec), err, "hipStreamWaitEvent")) return NULL;
		if (clo_hip_failed(clo_devbuf_reserve(&hist->workspace, ws), err, "hipMalloc(histogram workspace)")) return NULL;
	}
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_HISTOGRAM_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_histogram(kin, vin, out, numel, (int) ks, hist_key_signed(hist->key_type), (int) hist->value_type,
		(int) hist->sum_type, hist_lower_bits(hist, lower), shift, num_bins, hist->accumulate, 0u,
		hist->workspace.ptr, hist->workspace.bytes, ccl_queue_get_stream(cq_exec));
	if (clo_hip_failed(st, err, "clo_hip_histogram")) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	if (!ccl_queue_end_command(cq_exec, evt, err)) { ccl_queue_abort_command(cq_exec, evt); return NULL; }
	return evt;
}

cl_bool clo_histogram_with_host_data(CloHistogram* hist, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* hist_out,
	size_t numel, const void* lower, unsigned shift, size_t num_bins, GError** err) {
	clo_return_val_if_fail(hist != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = hist_refusal(hist, keys_in, values_in, hist_out, numel, shift, num_bins);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const size_t ks = clo_type_sizeof(hist->key_type), vs = clo_type_sizeof(hist->value_type), ss = clo_type_sizeof(hist->sum_type);
	if (numel == 0) {   /* no device needed */
		if (!hist->accumulate) memset(hist_out, 0, num_bins * ss);
		return CL_TRUE;
	}

	cl_bool status = CL_FALSE;
	CCLBuffer* dev[3] = { NULL, NULL, NULL };   /* keys in, values in, histogram */
	CCLQueue* intern_queue = NULL;
	CCLEvent* evt = NULL;
	CCLEventWaitList ewl = NULL;
	GError* err_internal = NULL;
	const size_t bytes[3] = { numel * ks, numel * vs, num_bins * ss };
	const int used[3] = { 1, values_in != NULL, 1 };
	CCLContext* ctx = hist->ctx;

	if (cq_exec == NULL) {
		CCLDevice* d = ccl_context_get_device(ctx, 0, &err_internal);
		if (err_internal) goto error_handler;
		intern_queue = ccl_queue_new(ctx, d, 0, &err_internal);
		if (err_internal) goto error_handler;
		cq_exec = intern_queue;
	}
	if (cq_comm == NULL) cq_comm = cq_exec;
	for (int i = 0; i < 3; ++i) {
		if (!used[i]) continue;
		dev[i] = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, bytes[i], NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	ccl_buffer_enqueue_write(dev[0], cq_comm, CL_TRUE, 0, bytes[0], (void*) keys_in, NULL, &err_internal);
	if (err_internal) goto error_handler;
	if (values_in) {
		ccl_buffer_enqueue_write(dev[1], cq_comm, CL_TRUE, 0, bytes[1], (void*) values_in, NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	if (hist->accumulate) {   /* what hist_out holds is added onto */
		ccl_buffer_enqueue_write(dev[2], cq_comm, CL_TRUE, 0, bytes[2], hist_out, NULL, &err_internal);
		if (err_internal) goto error_handler;
	}
	evt = clo_histogram_with_device_data(hist, cq_exec, cq_comm, dev[0], dev[1], dev[2], numel, lower, shift, num_bins, &err_internal);
	if (err_internal) goto error_handler;
	ccl_buffer_enqueue_read(dev[2], cq_comm, CL_TRUE, 0, bytes[2], hist_out, evt ? ccl_ewl(&ewl, evt, NULL) : NULL, &err_internal);
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

CCLContext* clo_histogram_get_context(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, NULL);
	return hist->ctx;
}

CloType clo_histogram_get_key_type(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, (CloType) -1);
	return hist->key_type;
}

size_t clo_histogram_get_key_size(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, 0);
	return clo_type_sizeof(hist->key_type);
}

CloType clo_histogram_get_value_type(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, (CloType) -1);
	return hist->value_type;
}

size_t clo_histogram_get_value_size(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, 0);
	return clo_type_sizeof(hist->value_type);
}

CloType clo_histogram_get_sum_type(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, (CloType) -1);
	return hist->sum_type;
}

size_t clo_histogram_get_sum_size(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, 0);
	return clo_type_sizeof(hist->sum_type);
}

cl_bool clo_histogram_get_accumulate(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, CL_FALSE);
	return hist->accumulate ? CL_TRUE : CL_FALSE;
}
