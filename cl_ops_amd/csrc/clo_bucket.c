/*
 * clo_bucket.c — CloBucket (include/clo_bucket.h; not upstream): stable multi-way partition of rows by the bin of an
 * integer key, with values or as indices, and the buckets' CSR offsets. The kernels are reached through the thin C-ABI
 * (clo_hip_bucket, include/clo_hip.h); the host layer is the one the operation drivers share (clo_internal.h).
 *
 * Every argument is checked before anything touches the device, so that the refusals come back the same on a
 * context without one. err may be NULL everywhere.
 */
#include "clo_bucket.h"

#include <stdint.h>
#include <string.h>

#include "clo_internal.h"

#define CLO_BUCKET_EVENT "clo_bucket"

struct clo_bucket {
	clo_op_head head;        /* the workspace: what clo_hip_bucket_workspace_bytes asks for */
	CloType key_type, count_type;
	size_t value_size;
};

CloBucket* clo_bucket_new(const char* options, CCLContext* ctx, CloType key_type, size_t value_size, CloType count_type, GError** err) {
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	if (options != NULL && strlen(options) > 0) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Invalid options for a bucket partition (NULL or \"\").");
		return NULL;
	}
	if (!ctx) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "clo_bucket_new needs a context.");
		return NULL;
	}
	if ((int) key_type < (int) CLO_CHAR || (int) key_type > (int) CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "Bucket keys are integers (char .. ulong), not '%s': the bin edges of "
			"floating-point keys need a rounding contract.", clo_type_get_name(key_type) ? clo_type_get_name(key_type) : "?");
		return NULL;
	}
	if (value_size != 0 && value_size != 4 && value_size != 8) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "A bucket partition carries values of 0 (none), 4 or 8 bytes, not a value_size of %zu.", value_size);
		return NULL;
	}
	if (count_type != CLO_UINT && count_type != CLO_ULONG) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "The count_type of the offsets is uint or ulong, not '%s'.",
			clo_type_get_name(count_type) ? clo_type_get_name(count_type) : "?");
		return NULL;
	}
	CloBucket* bkt = (CloBucket*) clo_op_new(sizeof(CloBucket), ctx, err);
	if (!bkt) return NULL;
	bkt->key_type = key_type;
	bkt->count_type = count_type;
	bkt->value_size = value_size;
	return bkt;
}

void clo_bucket_destroy(CloBucket* bkt) {
	clo_return_if_fail(bkt != NULL);
	clo_op_destroy(bkt);
}

/* Why these arguments are refused, or NULL; pointers of the device or of the host, nothing is dereferenced. */
static const char* bucket_refusal(CloBucket* bkt, const void* keys_in, const void* values_in, const void* keys_out,
	const void* values_out, const void* offsets_out, size_t numel, unsigned shift, size_t num_bins) {
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	if (num_bins == 0) return "num_bins must not be 0";
	if (num_bins > CLO_BUCKET_MAX_BINS) return "num_bins must not exceed CLO_BUCKET_MAX_BINS (65535): sort instead";
	if (shift >= 8u * clo_type_sizeof(bkt->key_type)) return "shift must be below the number of bits of the key type";
	if (!offsets_out) return "offsets_out is required";
	if (numel > 0 && !keys_in) return "keys_in is required";
	if (bkt->value_size == 0 && (values_in || values_out)) return "values passed to a bucket partition made with value_size 0";
	if (bkt->value_size > 0 && !values_out) return "values_out is required with a value_size above 0";
	if (bkt->value_size == 8 && !values_in) return "NULL values_in (the arg form) needs a value_size of 4: the indices are written as uint";
	if (!keys_out && !(bkt->value_size == 4 && !values_in)) return "keys_out is required (only the arg form writes indices alone)";
	const size_t ks = clo_type_sizeof(bkt->key_type), vs = bkt->value_size;
	const clo_range in[2] = { { keys_in, numel * ks }, { values_in, numel * vs } };
	const clo_range out[3] = { { keys_out, numel * ks }, { values_out, numel * vs }, { offsets_out, (num_bins + 1) * clo_type_sizeof(bkt->count_type) } };
	switch (clo_ranges_conflict(in, 2, out, 3)) {
		case CLO_RANGES_OUT_IN: return "an output range overlaps an input range (there is no in-place bucket partition)";
		case CLO_RANGES_OUT_OUT: return "two output ranges overlap";
	}
	return NULL;
}

/* *lower as the bits the thin ABI takes: the low key-size bytes of a uint64 (little-endian host, as the device) */
static uint64_t bucket_lower_bits(CloBucket* bkt, const void* lower) {
	uint64_t bits = 0;
	if (lower) memcpy(&bits, lower, clo_type_sizeof(bkt->key_type));
	return bits;
}

CCLEvent* clo_bucket_with_device_data(CloBucket* bkt, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* offsets_out,
	size_t numel, const void* lower, unsigned shift, size_t num_bins, GError** err) {
	clo_return_val_if_fail(bkt != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;   /* nothing is copied */
	CCLBuffer* const buf[5] = { keys_in, values_in, keys_out, values_out, offsets_out };
	void* p[5];
	clo_buffers_device_ptrs(buf, p, 5);
	const char* why = bucket_refusal(bkt, p[0], p[1], p[2], p[3], p[4], numel, shift, num_bins);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	const size_t ks = clo_type_sizeof(bkt->key_type), vs = bkt->value_size, cs = clo_type_sizeof(bkt->count_type);
	const size_t need[5] = { numel * ks, numel * vs, numel * ks, numel * vs, (num_bins + 1) * cs };
	if (!clo_buffers_hold(buf, need, 5)) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "numel (%zu) or num_bins (%zu) exceeds the size of the device buffers (the inputs and "
			"the outputs hold numel rows, offsets_out num_bins + 1 entries)", numel, num_bins);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	clo_debug("BUCKET: %zu keys of type %s into %zu bins (shift %u), %s, offsets %s", numel, clo_type_get_name(bkt->key_type), num_bins, shift,
		vs == 0 ? "no values" : !p[1] ? "indices" : vs == 4 ? "4-byte values" : "8-byte values", clo_type_get_name(bkt->count_type));

	const size_t ws = clo_hip_bucket_workspace_bytes(numel, (int) ks, (int) vs, num_bins);
	if (ws > 0 && !clo_op_reserve(&bkt->head, cq_exec, ws, "hipMalloc(bucket workspace)", err)) return NULL;
	CCLEvent* evt = ccl_queue_begin_command(cq_exec, CLO_BUCKET_EVENT, err);
	if (!evt) return NULL;
	const int st = clo_hip_bucket(p[0], p[1], p[2], p[3], p[4], numel, (int) ks, clo_type_is_signed(bkt->key_type), (int) vs, (int) cs,
		bucket_lower_bits(bkt, lower), shift, num_bins, bkt->head.workspace.ptr, bkt->head.workspace.bytes, ccl_queue_get_stream(cq_exec));
	return clo_op_end_command(cq_exec, evt, st, "clo_hip_bucket", err);
}

cl_bool clo_bucket_with_host_data(CloBucket* bkt, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* offsets_out,
	size_t numel, const void* lower, unsigned shift, size_t num_bins, GError** err) {
	clo_return_val_if_fail(bkt != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const char* why = bucket_refusal(bkt, keys_in, values_in, keys_out, values_out, offsets_out, numel, shift, num_bins);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	const size_t ks = clo_type_sizeof(bkt->key_type), vs = bkt->value_size, cs = clo_type_sizeof(bkt->count_type);
	if (numel == 0) {   /* every bucket is empty: no device needed */
		memset(offsets_out, 0, (num_bins + 1) * cs);
		return CL_TRUE;
	}

	/* keys in, values in, keys out, values out, offsets */
	clo_stage st;
	clo_stage_open(&st, bkt->head.ctx, cq_exec, cq_comm);
	clo_stage_in(&st, 0, keys_in, numel * ks);
	clo_stage_in(&st, 1, values_in, numel * vs);
	clo_stage_out(&st, 2, keys_out, numel * ks);
	clo_stage_out(&st, 3, values_out, numel * vs);
	clo_stage_out(&st, 4, offsets_out, (num_bins + 1) * cs);
	if (clo_stage_ok(&st))
		st.evt = clo_bucket_with_device_data(bkt, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], st.dev[4],
			numel, lower, shift, num_bins, &st.err);
	clo_stage_read(&st, 4, offsets_out, (num_bins + 1) * cs);
	clo_stage_read(&st, 2, keys_out, numel * ks);
	clo_stage_read(&st, 3, values_out, numel * vs);
	return clo_stage_close(&st, err);
}

CCLContext* clo_bucket_get_context(CloBucket* bkt) {
	clo_return_val_if_fail(bkt != NULL, NULL);
	return bkt->head.ctx;
}

CloType clo_bucket_get_key_type(CloBucket* bkt) {
	clo_return_val_if_fail(bkt != NULL, (CloType) -1);
	return bkt->key_type;
}

size_t clo_bucket_get_key_size(CloBucket* bkt) {
	clo_return_val_if_fail(bkt != NULL, 0);
	return clo_type_sizeof(bkt->key_type);
}

size_t clo_bucket_get_value_size(CloBucket* bkt) {
	clo_return_val_if_fail(bkt != NULL, 0);
	return bkt->value_size;
}

CloType clo_bucket_get_count_type(CloBucket* bkt) {
	clo_return_val_if_fail(bkt != NULL, (CloType) -1);
	return bkt->count_type;
}

size_t clo_bucket_get_count_size(CloBucket* bkt) {
	clo_return_val_if_fail(bkt != NULL, 0);
	return clo_type_sizeof(bkt->count_type);
}
