/*
 * clo_segscan.h — CloSegScan: the running sum, minimum or maximum of every row within its segment, the segments given by
 * counts or by CSR offsets. NOT upstream (the reference has sort, scan and rng only). The per-row counterpart of
 * clo_segreduce.h and the offsets form of clo_scan_by_key_*: running totals per CSR row, cumulative maxima per sequence
 * of a ragged batch, the prefix weights of a per-segment sampling step, the transform between clo_expand.h and
 * clo_segreduce.h. A caller with counts needs no segment ids: an expand into ids followed by a scan by key on them
 * writes and reads those ids and reads the values twice.
 *
 * op is one of CLO_SCAN_BY_KEY_OPS (clo_scan_by_key.h), form one of CLO_SEGSCAN_FORMS; count_type is uint or ulong for
 * both forms. options is scan by key's: NULL, "" and "inclusive=0" mean exclusive, "inclusive=1" inclusive; anything
 * else is refused. The segments are clo_segreduce.h's: with m_h = numel_seg and m = min(m_h, *num_in) when num_in is
 * given (one cl_ulong of device memory, 8-byte aligned; the host form: a host size_t), else m_h:
 *
 *   form "counts"   counts_or_offsets holds m_h counts c_r. e_r = c_0 + .. + c_r in 64-bit arithmetic, s_r = e_(r-1),
 *                   s_0 = 0, total = e_(m-1), 0 for m = 0. Entries at r >= m are not part of the sum.
 *   form "offsets"  counts_or_offsets holds m_h + 1 offsets, ascending (the precondition); entries [0, m] are read.
 *                   With base = offsets[0]: s_r = offsets[r] - base, e_r = offsets[r + 1] - base, total = offsets[m] -
 *                   base. offsets[0] = 0 is a CSR row pointer, anything else a slice of one, rebased.
 *
 * num_in exists so that num_runs_out of clo_reduce_by_key_with_device_data is passed straight in, numel_seg being the
 * buffers' row count, on the same queue and with no host wait.
 *
 * With n = numel, x[j] = (sum_type) values_in[j] and ct = min(total, n): every row i < ct lies in exactly one clipped
 * segment [min(s_r, n), min(e_r, n)); let b(i) be that segment's first row. Then
 *     inclusive   data_out[i] = x[b(i)] op .. op x[i]
 *     exclusive   data_out[i] = x[b(i)] op .. op x[i-1], and the IDENTITY at i = b(i): 0 for sum, the sum type's
 *                 largest value for min, its smallest for max.
 * The cast is C's, as in scan by key; sums wrap modulo 2^bits of the sum type; min and max compare in the sum type,
 * signed or unsigned as that type is. Rows i >= ct of data_out (which holds n rows) are NOT written. A segment without
 * a row owns none and changes nothing. num_out (one cl_ulong of device memory, 8-byte aligned, required) receives total
 * UNCLAMPED: num_out > numel tells the caller that segments were clipped. m = 0 writes num_out = 0 and nothing else (the
 * host form returns then without a device).
 *
 * In place: data_out may be EXACTLY values_in when the sum type is as wide as the value type (scan by key's rule).
 * Every other overlap of an output with an input, with num_in, or with the other output is refused.
 *
 * Values are int, uint, long or ulong; the sum type is one of the same four and at least as wide as the value type.
 * Floating-point aggregates stay out, for the reason clo_reduce.h gives: their sums depend on the order of addition.
 * values_in == NULL as "every value is 1" is not offered either: rank_out of clo_expand.h is that result.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * an unknown op or form; options other than those above; a value or sum type outside the four, a sum type narrower
 * than the value type, a count_type other than uint or ulong; numel_seg or numel >= 2^32; NULL counts_or_offsets with
 * numel_seg > 0, and in the offsets form always; NULL values_in or data_out with numel > 0; num_out NULL (device form:
 * misaligned, or below 8 bytes); num_in misaligned or below 8 bytes (device form); a buffer too small
 * (counts_or_offsets for m_h counts or m_h + 1 offsets, values_in and data_out for numel rows); data_out or num_out
 * overlapping an input, num_in or each other, but for the in-place case above.
 *
 * Whatever the arrays hold — offsets that do not ascend, sums that wrap 2^64, a *num_in above m_h — every read stays
 * inside the inputs, every write stays inside data_out[0, numel) and num_out, and the call completes; the contents are
 * then unspecified.
 *
 * Out of scope: floating point, reverse (suffix) scans, a caller's initial value per segment,
 * several value columns per call, numel >= 2^32, a single-sweep look-back form.
 */
#ifndef CLO_SEGSCAN_H
#define CLO_SEGSCAN_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_SEGSCAN_FORMS "counts, offsets"

typedef struct clo_segscan CloSegScan;

/* Works on a context without a device (ccl_context_new_offline). */
CloSegScan* clo_segscan_new(const char* op, const char* form, const char* options, CCLContext* ctx,
	CloType value_type, CloType sum_type, CloType count_type, GError** err);
void clo_segscan_destroy(CloSegScan* ss);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the segment
 * ends of the counts form, a few words per tile) belongs to one queue at a time and only grows. */
CCLEvent* clo_segscan_with_device_data(CloSegScan* ss, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* data_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err);
/* Blocking: copy in, run, copy the min(total, numel) rows of data_out and total back. cq_exec NULL: a queue of its own;
 * cq_comm NULL: cq_exec. */
cl_bool clo_segscan_with_host_data(CloSegScan* ss, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	void* data_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err);

CCLContext* clo_segscan_get_context(CloSegScan* ss);
const char* clo_segscan_get_op(CloSegScan* ss);
const char* clo_segscan_get_form(CloSegScan* ss);
cl_bool clo_segscan_get_inclusive(CloSegScan* ss);
CloType clo_segscan_get_value_type(CloSegScan* ss);
size_t clo_segscan_get_value_size(CloSegScan* ss);
CloType clo_segscan_get_sum_type(CloSegScan* ss);
size_t clo_segscan_get_sum_size(CloSegScan* ss);
CloType clo_segscan_get_count_type(CloSegScan* ss);
size_t clo_segscan_get_count_size(CloSegScan* ss);

#ifdef __cplusplus
}
#endif
#endif
