/*
 * clo_reduce.h — CloReduceByKey: every run of equal keys collapsed into one row. NOT upstream (the reference has
 * sort, scan and rng only); it is what follows clo_sort_by_key_with_device_data (include/clo_sort.h): a group-by
 * sum, a histogram of arbitrary keys, a run-length encoding, the distinct keys, segment sizes.
 *
 * A RUN is a maximal stretch of consecutive elements whose keys have the same bytes (1, 2, 4 or 8 of them, any
 * CloType: -0.0f and +0.0f are different keys, two NaNs are equal exactly when their bits are). Keys need not be
 * sorted: unsorted input gives one row per stretch, not per distinct key. With m runs, run r covering [b_r, e_r):
 *   keys_out[r] = keys_in[b_r]
 *   aggr_out[r] = op over i in [b_r, e_r) of (sum_type) values_in[i]      op: "sum", "min" or "max"
 *   *num_runs   = m
 * The cast is the scan's C cast `(CLO_SCAN_SUM_TYPE) x`; sums wrap modulo 2^bits of the sum type, min / max compare
 * in the sum type, signed or unsigned as that type is. values_in NULL: every value is 1, so "sum" gives the run
 * lengths ("min" / "max" are refused then). keys_out or aggr_out may be NULL (not written), not both; with keys_out
 * alone the call is unique_consecutive. keys_out and aggr_out have room for numel entries; entries at index >= m are
 * NOT written. numel 0 gives m = 0.
 *
 * Types: keys of any CloType; values int, uint, long or ulong; the sum type int, uint, long or ulong and at least as
 * wide as the value type. Refused with CLO_ERROR_ARGS before any device call (err may be NULL): floating-point values
 * or sums, value types narrower than 4 bytes, a sum narrower than the values, numel >= 2^32, an unknown op, options
 * other than NULL / "", and an output range that overlaps an input range (rows land at lower addresses than the
 * elements they come from, in tiles another work-group may not have read yet: in place cannot work in one sweep).
 * Floating-point aggregates are out of scope: their sums depend on the order of addition.
 */
#ifndef CLO_REDUCE_H
#define CLO_REDUCE_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_REDUCE_BY_KEY_OPS "sum, min, max"

typedef struct clo_reduce_by_key CloReduceByKey;

/* Works on a context without a device (ccl_context_new_offline), as clo_sort_new does. value_type is ignored by calls
 * that pass no values, sum_type by calls that pass no aggr_out; both must be valid all the same. `options`: NULL or
 * empty (kept so that later switches do not change the signature). */
CloReduceByKey* clo_reduce_by_key_new(const char* op, const char* options, CCLContext* ctx,
	CloType key_type, CloType value_type, CloType sum_type, GError** err);
void clo_reduce_by_key_destroy(CloReduceByKey* rbk);

/* Asynchronous on cq_exec; never synchronises the device (once the object's scratch has grown to the size of the
 * call: it lives in the object and only ever grows), so that a sort by key followed by this call runs back to back.
 * num_runs_out: one cl_ulong of device memory, 8-byte aligned, required. cq_comm is not used. */
CCLEvent* clo_reduce_by_key_with_device_data(CloReduceByKey* rbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out, CCLBuffer* aggr_out,
	CCLBuffer* num_runs_out, size_t numel, GError** err);
/* Blocking: copy in, reduce, copy out (the m rows only). cq_exec NULL: a queue of its own; cq_comm NULL: cq_exec. */
cl_bool clo_reduce_by_key_with_host_data(CloReduceByKey* rbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* keys_out, void* aggr_out,
	size_t* num_runs, size_t numel, GError** err);

CCLContext* clo_reduce_by_key_get_context(CloReduceByKey* rbk);
CloType clo_reduce_by_key_get_key_type(CloReduceByKey* rbk);
size_t clo_reduce_by_key_get_key_size(CloReduceByKey* rbk);
CloType clo_reduce_by_key_get_value_type(CloReduceByKey* rbk);
size_t clo_reduce_by_key_get_value_size(CloReduceByKey* rbk);
CloType clo_reduce_by_key_get_sum_type(CloReduceByKey* rbk);
size_t clo_reduce_by_key_get_sum_size(CloReduceByKey* rbk);
const char* clo_reduce_by_key_get_op(CloReduceByKey* rbk);

#ifdef __cplusplus
}
#endif
#endif
