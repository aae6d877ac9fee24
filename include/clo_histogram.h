/*
 * clo_histogram.h — CloHistogram: counts or sums of values per bin, for integer keys whose bin is known from the key
 * alone. NOT upstream (the reference has sort, scan and rng only). Where the key is a small integer (a bucket id, a
 * digit, a class label, a cell index) and the number of groups is known beforehand, this replaces
 * clo_sort_by_key_* followed by clo_reduce_by_key_* (include/clo_reduce.h): the keys are read once and nothing is
 * sorted. Followed by clo_scan_* it gives the bucket offsets of a counting sort.
 *
 * Keys are of an integer CloType (char .. ulong), B bits wide. `lower` points to ONE host value of the key type
 * (NULL: 0). Over the integers, d = key - lower. An element is COUNTED iff d >= 0 and (d >> shift) < num_bins; its
 * bin is d >> shift. Everything else is ignored. Then
 *   hist_out[b] = sum of (sum_type) values_in[i] over the counted elements i of bin b,
 * wrapping modulo 2^bits of the sum type. The cast is the C cast clo_reduce.h uses: int -> long sign-extends,
 * uint -> long zero-extends. values_in NULL: every value is 1, which gives counts. All num_bins entries of hist_out
 * are written, zeros included. With options "accumulate" the results are ADDED onto what hist_out holds and nothing is
 * zeroed, so batches and arrays beyond 2^32 elements can be fed in pieces. numel 0 zeroes hist_out, or leaves it
 * alone under "accumulate" (the host form does this without a device). Integer addition commutes: the result does
 * not depend on scheduling.
 *
 * Types: values int, uint, long or ulong; the sum type one of those four and at least as wide as the value type.
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL): floating-point or half keys (their bin edges
 * need a rounding contract: DESIGN.md §7), value or sum types outside the four, a sum narrower than the values,
 * num_bins 0 or >= 2^32, shift >= B, numel >= 2^32, options other than NULL, "" or "accumulate", NULL keys_in with
 * numel > 0, NULL hist_out, and a hist_out range that overlaps an input range.
 */
#ifndef CLO_HISTOGRAM_H
#define CLO_HISTOGRAM_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct clo_histogram CloHistogram;

/* Works on a context without a device (ccl_context_new_offline). value_type is ignored by calls that pass no values;
 * it must be valid all the same. */
CloHistogram* clo_histogram_new(const char* options, CCLContext* ctx,
	CloType key_type, CloType value_type, CloType sum_type, GError** err);
void clo_histogram_destroy(CloHistogram* hist);

/* Asynchronous on cq_exec; never synchronises the device. hist_out: num_bins entries of the sum type. cq_comm is not
 * used. */
CCLEvent* clo_histogram_with_device_data(CloHistogram* hist, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* hist_out,
	size_t numel, const void* lower, unsigned shift, size_t num_bins, GError** err);
/* Blocking: copy in (under "accumulate" hist_out too), histogram, copy out. cq_exec NULL: a queue of its own;
 * cq_comm NULL: cq_exec. */
cl_bool clo_histogram_with_host_data(CloHistogram* hist, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* hist_out,
	size_t numel, const void* lower, unsigned shift, size_t num_bins, GError** err);

CCLContext* clo_histogram_get_context(CloHistogram* hist);
CloType clo_histogram_get_key_type(CloHistogram* hist);
size_t clo_histogram_get_key_size(CloHistogram* hist);
CloType clo_histogram_get_value_type(CloHistogram* hist);
size_t clo_histogram_get_value_size(CloHistogram* hist);
CloType clo_histogram_get_sum_type(CloHistogram* hist);
size_t clo_histogram_get_sum_size(CloHistogram* hist);
cl_bool clo_histogram_get_accumulate(CloHistogram* hist);

#ifdef __cplusplus
}
#endif
#endif
