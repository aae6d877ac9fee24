/*
 * clo_scan_by_key.h — CloScanByKey: the running sum, min or max of every element within its run of equal keys, and
 * its rank there. NOT upstream (the reference has sort, scan and rng only); it is the third leg of the group-by
 * pipeline after clo_sort_by_key_with_device_data (include/clo_sort.h) and CloReduceByKey (include/clo_reduce.h):
 * the rank of an element inside its group (top-k per group, cumcount), running totals, minima and maxima per group,
 * the offsets that turn a run-length encoding back into positions.
 *
 * A RUN is defined as in clo_reduce.h: a maximal stretch of consecutive elements whose keys have the same bytes (1,
 * 2, 4 or 8 of them, any CloType: -0.0f and +0.0f are different keys, two NaNs are equal exactly when their bits
 * are). Keys need not be sorted. With b(i) the index of the first element of i's run and x[j] = (sum_type)
 * values_in[j] (the scan's C cast), for every i < numel:
 *   inclusive:  data_out[i] = x[b(i)] op ... op x[i]
 *   exclusive:  data_out[i] = x[b(i)] op ... op x[i-1], and the identity at i = b(i): 0 for "sum", the largest
 *               number of the sum type for "min", the smallest for "max"
 * op is "sum", "min" or "max". Sums wrap modulo 2^bits of the sum type; min / max compare in the sum type, signed or
 * unsigned as that type is. values_in NULL: every value is 1, so the exclusive sum is the element's rank in its run
 * (0-based) and the inclusive sum its 1-based rank ("min" / "max" are refused then). numel 0 launches nothing.
 *
 * `options` chooses the kind, in the library's k=v syntax: NULL or "" is exclusive (as CloScan is), "inclusive=1"
 * inclusive, "inclusive=0" exclusive; anything else is refused.
 *
 * In place: element i's result lands at index i, so data_out may be EXACTLY values_in (the same address) when the sum
 * type is as wide as the value type. Every other overlap of data_out with keys_in or values_in is refused.
 *
 * Types: keys of any CloType; values int, uint, long or ulong; the sum type int, uint, long or ulong and at least as
 * wide as the value type. Refused with CLO_ERROR_ARGS before any device call (err may be NULL): floating-point values
 * or sums, value types narrower than 4 bytes, a sum narrower than the values, numel >= 2^32, an unknown op, other
 * options, a missing keys_in or data_out, and the overlaps above. Out of scope: floating-point values
 * or sums (the order of addition; min / max of floats would be well defined but are left with them), values narrower
 * than 4 bytes, a scan without keys (inclusive and min / max forms of the plain scan belong to CloScan), a
 * user-supplied initial value for the exclusive form, a single-sweep look-back form.
 */
#ifndef CLO_SCAN_BY_KEY_H
#define CLO_SCAN_BY_KEY_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_SCAN_BY_KEY_OPS "sum, min, max"

typedef struct clo_scan_by_key CloScanByKey;

/* Works on a context without a device (ccl_context_new_offline). value_type is ignored by calls that pass no values;
 * it must be valid all the same. */
CloScanByKey* clo_scan_by_key_new(const char* op, const char* options, CCLContext* ctx,
	CloType key_type, CloType value_type, CloType sum_type, GError** err);
void clo_scan_by_key_destroy(CloScanByKey* sbk);

/* Asynchronous on cq_exec; never synchronises the device (once the object's scratch has grown to the size of the
 * call: it lives in the object and only ever grows), so that a sort by key, this call and a reduce by key run back to
 * back. values_in may be NULL. cq_comm is not used. */
CCLEvent* clo_scan_by_key_with_device_data(CloScanByKey* sbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* data_out, size_t numel, GError** err);
/* Blocking: copy in, scan, copy out. cq_exec NULL: a queue of its own; cq_comm NULL: cq_exec. data_out may be
 * values_in under the in-place rule. */
cl_bool clo_scan_by_key_with_host_data(CloScanByKey* sbk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* data_out, size_t numel, GError** err);

CCLContext* clo_scan_by_key_get_context(CloScanByKey* sbk);
CloType clo_scan_by_key_get_key_type(CloScanByKey* sbk);
size_t clo_scan_by_key_get_key_size(CloScanByKey* sbk);
CloType clo_scan_by_key_get_value_type(CloScanByKey* sbk);
size_t clo_scan_by_key_get_value_size(CloScanByKey* sbk);
CloType clo_scan_by_key_get_sum_type(CloScanByKey* sbk);
size_t clo_scan_by_key_get_sum_size(CloScanByKey* sbk);
const char* clo_scan_by_key_get_op(CloScanByKey* sbk);
cl_bool clo_scan_by_key_get_inclusive(CloScanByKey* sbk);

#ifdef __cplusplus
}
#endif
#endif
