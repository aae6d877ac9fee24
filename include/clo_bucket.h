/*
 * clo_bucket.h — CloBucket: stable multi-way partition of rows into num_bins buckets by the bin of an integer key, with
 * values carried along or the indices written, and the buckets' CSR offsets written to device memory. NOT upstream (the
 * reference has sort, scan and rng only). It is the counting sort CloHistogram (include/clo_histogram.h) counts for:
 * where the grouping key is a small integer (a cell index, a class label, a digit, a destination rank), this replaces
 * clo_sort_by_key_* followed by clo_reduce_by_key_*, and its offsets feed the "offsets" form of CloExpand,
 * CloSegReduce, CloSegSort and CloSegScan on the same queue with no host wait.
 *
 * The bin mapping is CloHistogram's. Keys are of an integer CloType (char .. ulong), B bits wide. `lower` points to ONE
 * host value of the key type (NULL: 0). Over the integers, d = key - lower. A row is IN RANGE iff d >= 0 and
 * (d >> shift) < num_bins; its bin is then d >> shift. Every other row belongs to the REST.
 *
 * The rows go to the outputs bin by bin in ascending bin order, the rest last. Inside each bin, and inside the rest,
 * rows keep their input order: bit for bit a stable sort of the rows by bin, the rest counting as bin num_bins. All
 * numel rows are written: the outputs are a permutation of the inputs. offsets_out holds num_bins + 1 entries of
 * count_type (uint or ulong, as clo_segsort.h; numel < 2^32, so uint never overflows): offsets_out[0] = 0,
 * offsets_out[b + 1] - offsets_out[b] is the number of rows in bin b (CloHistogram's count), offsets_out[num_bins] is
 * the number of rows in range, and the rest occupies rows [offsets_out[num_bins], numel). All entries are written,
 * those of empty bins included. numel == 0 writes num_bins + 1 zeros (the host form does this without a device).
 *
 * Values are opaque words of value_size bytes, 0 (none), 4 or 8: values_out[j] belongs to keys_out[j]. Arg form:
 * value_size 4 and values_in NULL: values_out[j] is the input row index as uint. keys_out may then be NULL. There is no
 * in-place form.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * floating-point or half keys; a value_size other than 0, 4 or 8; a count_type other than uint or ulong; options other
 * than NULL or ""; num_bins 0 or above CLO_BUCKET_MAX_BINS; shift >= B; numel >= 2^32; NULL keys_in with numel > 0; NULL
 * offsets_out; values passed with value_size 0; values_out NULL with value_size > 0; NULL values_in with value_size 8;
 * keys_out NULL outside the arg form; a buffer too small; any output overlapping an input or another output.
 *
 * The mapping is total, so there is no precondition on the data: whatever the keys hold, every read stays inside the
 * inputs, every write inside [0, numel) of the row outputs and [0, num_bins] of offsets_out, and the call completes.
 *
 * Out of scope: more than 65 535 bins (sort instead); floating-point keys; get_key or run-time
 * compiled bin functions; numel >= 2^32; values wider than 8 bytes; numel read from device memory; dropping the rest
 * instead of writing it; the large-bin histogram built on top of this pass.
 */
#ifndef CLO_BUCKET_H
#define CLO_BUCKET_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_BUCKET_MAX_BINS 65535

typedef struct clo_bucket CloBucket;

/* Works on a context without a device (ccl_context_new_offline). */
CloBucket* clo_bucket_new(const char* options, CCLContext* ctx, CloType key_type, size_t value_size, CloType count_type, GError** err);
void clo_bucket_destroy(CloBucket* bkt);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the tiles' digit
 * counts and, above 255 bins, the rows between the two passes) belongs to one queue at a time and only grows. */
CCLEvent* clo_bucket_with_device_data(CloBucket* bkt, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* offsets_out,
	size_t numel, const void* lower, unsigned shift, size_t num_bins, GError** err);
/* Blocking: copy in, run, copy the rows and the offsets out. cq_exec NULL: a queue of its own; cq_comm NULL: cq_exec. */
cl_bool clo_bucket_with_host_data(CloBucket* bkt, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* offsets_out,
	size_t numel, const void* lower, unsigned shift, size_t num_bins, GError** err);

CCLContext* clo_bucket_get_context(CloBucket* bkt);
CloType clo_bucket_get_key_type(CloBucket* bkt);
size_t clo_bucket_get_key_size(CloBucket* bkt);
size_t clo_bucket_get_value_size(CloBucket* bkt);
CloType clo_bucket_get_count_type(CloBucket* bkt);
size_t clo_bucket_get_count_size(CloBucket* bkt);

#ifdef __cplusplus
}
#endif
#endif
