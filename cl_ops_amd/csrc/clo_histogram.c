/*
 * clo_histogram.c — CloHistogram (include/clo_histogram.h; not upstream): counts or sums of values per bin of
 * integer keys. The kernels are reached through the thin C-ABI (clo_hip_histogram, include/clo_hip.h); the host layer
 * is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_histogram.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_HISTOGRAM_EVENT "clo_histogram"

struct clo_histogram {
	clo_op_head head;        /* the workspace: what clo_hip_histogram_workspace_bytes asks for (nothing today) */
	CloType key_type, value_type, sum_type;
	int accumulate;
};

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
	if (!clo_type_is_int32_or_64(value_type) || !clo_type_is_int32_or_64(sum_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Histogram takes values and sums of type int, uint, long or ulong, not '%s' into '%s'.",
			clo_type_get_name(value_type) ? clo_type_get_name(value_type) : "?", clo_type_get_name(sum_type) ? clo_type_get_name(sum_type) : "?");
		return NULL;
	}
	if (clo_type_sizeof(sum_type) < clo_type_sizeof(value_type)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The sum type '%s' is narrower than the value type '%s'.",
			clo_type_get_name(sum_type), clo_type_get_name(value_type));
		return NULL;
	}
	CloHistogram* hist = (CloHistogram*) clo_op_new(sizeof(CloHistogram), ctx, err);
	if (!hist) return NULL;
	hist->key_type = key_type;
	hist->value_type = value_type;
	hist->sum_type = sum_type;
	hist->accumulate = accumulate;
	return hist;
}

void clo_histogram_destroy(CloHistogram* hist) {
	clo_return_if_fail(hist != NULL);
	clo_op_destroy(hist);
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
	const clo_range in[2] = { { keys_in, numel * clo_type_sizeof(hist->key_type) }, { values_in, numel * clo_type_sizeof(hist->value_type) } };
	const clo_range out = { hist_out, num_bins * clo_type_sizeof(hist->sum_type) };
	if (clo_ranges_conflict(in, 2, &out, 1)) return "the hist_out range overlaps an input range";
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
	CCLBuffer* const buf[3] = { keys_in, values_in, hist_out };
	void* p[3];
	clo_buffers_device_ptrs(buf, p, 3);
	const char* why = hist_refusal(hist, p[0], p[1], p[2], numel, shift, num_bins);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(hist->key_type), vs = clo_type_sizeof(hist->value_type), ss = clo_type_sizeof(hist->sum_type);
	const size_t need[3] = { numel * ks, numel * vs, num_bins * ss };
	if (!clo_buffers_hold(buf, need, 3)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) or num_bins (%zu) exceeds the size of the device buffers", numel, num_bins);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("HISTOGRAM: numel=%zu, key %s, values %s, sum %s, shift %u, %zu bins%s", numel, clo_type_get_name(hist->key_type),
		values_in ? clo_type_get_name(hist->value_type) : "absent", clo_type_get_name(hist->sum_type), shift, num_bins,
		hist->accumulate ? ", accumulating" : "");

	const size_t ws = clo_hip_histogram_workspace_bytes(numel, num_bins);
	if (ws > 0 && !clo_op_reserve(&hist->head, cq_exec, ws, "hipMalloc(histogram workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_HISTOGRAM_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_histogram(p[0], p[1], p[2], numel, (int) ks, clo_type_is_signed(hist->key_type), (int) hist->value_type,
		(int) hist->sum_type, hist_lower_bits(hist, lower), shift, num_bins, hist->accumulate, 0u,
		hist->head.workspace.ptr, hist->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_histogram", err);
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

	/* keys in, values in, histogram */
	clo_stage st;
	clo_stage_open(&st, hist->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, keys_in, numel * ks);
	clo_stage_in(&st, 1, values_in, numel * vs);
	if (hist->accumulate) clo_stage_in(&st, 2, hist_out, num_bins * ss);   /* what hist_out holds is added onto */
	else clo_stage_out(&st, 2, hist_out, num_bins * ss);
	if (clo_stage_ok(&st))
		st.evt = clo_histogram_with_device_data(hist, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], numel, lower, shift, num_bins, &st.err);
	clo_stage_read(&st, 2, hist_out, num_bins * ss);
	return clo_stage_close(&st, err);
}

CCLContext* clo_histogram_get_context(CloHistogram* hist) {
	clo_return_val_if_fail(hist != NULL, NULL);
	return hist->head.ctx;
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
