/*
 * clo_segreduce.h — CloSegReduce: the sum, minimum or maximum of every segment of an array, the segments given by
 * counts or by CSR offsets. NOT upstream (the reference has sort, scan and rng only). The offsets form of
 * clo_reduce_by_key_*: row sums and row maxima of a CSR matrix, the reduce half of an expand -> transform -> reduce
 * pipeline (clo_expand.h is the other half), pooling over sequences of different lengths. Unlike a reduce by key on
 * segment ids, a segment without a row keeps its output row: aggr_out[r] always speaks of segment r.
 *
 * op is one of CLO_REDUCE_BY_KEY_OPS (clo_reduce.h), form one of CLO_SEGREDUCE_FORMS; count_type is uint or ulong for
 * both forms. The segments are clo_expand.h's: with m_h = numel_seg and m = min(m_h, *num_in) when num_in is given (one
 * cl_ulong of device memory, 8-byte aligned; the host form: a host size_t), else m_h:
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
 * With n = numel, the rows of values_in, for every r < m:
 *     aggr_out[r] = op over i in [min(s_r, n), min(e_r, n)) of (sum_type) values_in[i]
 * The cast is C's, as in reduce by key; sums wrap modulo 2^bits of the sum type; min and max compare in the sum type,
 * signed or unsigned as that type is. A segment without a row — an empty one, or one that lies beyond n altogether —
 * receives the IDENTITY: 0 for sum, the sum type's largest value for min, its smallest for max. Rows r >= m of aggr_out
 * (which holds m_h rows) are NOT written. num_out (one cl_ulong of device memory, 8-byte aligned, required) receives
 * total UNCLAMPED: num_out > numel tells the caller that segments were clipped. m = 0 writes num_out = 0 and nothing
 * else (the host form returns then without a device).
 *
 * Values are int, uint, long or ulong; the sum type is one of the same four and at least as wide as the value type.
 * Floating-point aggregates stay out, for the reason clo_reduce.h gives: their sums depend on the order of addition.
 * (Floating-point sums per segment, with that order as their contract: CloSegFSum, clo_segfsum.h.)
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * an unknown op or form; options other than NULL or ""; a value or sum type outside the four, a sum type narrower than
 * the value type, a count_type other than uint or ulong; numel_seg or numel >= 2^32; NULL counts_or_offsets with
 * numel_seg > 0, and in the offsets form always; NULL values_in with numel > 0; NULL aggr_out with numel_seg > 0; num_out
 * NULL (device form: misaligned, or below 8 bytes); num_in misaligned or below 8 bytes (device form); a buffer too small
 * (counts_or_offsets for m_h counts or m_h + 1 offsets, values_in for numel rows, aggr_out for m_h rows); aggr_out or
 * num_out overlapping an input, num_in or each other.
 *
 * Whatever the arrays hold — offsets that do not ascend, sums that wrap 2^64, a *num_in above m_h — every read stays
 * inside the inputs, every write stays inside aggr_out[0, m_h) and num_out, and the call completes; the contents are
 * then unspecified.
 *
 * Out of scope: arg-min and arg-max, floating point, several value columns per call,
 * numel >= 2^32.
 */
#ifndef CLO_SEGREDUCE_H
#define CLO_SEGREDUCE_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_SEGREDUCE_FORMS "counts, offsets"

typedef struct clo_segreduce CloSegReduce;

/* Works on a context without a device (ccl_context_new_offline). */
CloSegReduce* clo_segreduce_new(const char* op, const char* form, const char* options, CCLContext* ctx,
	CloType value_type, CloType sum_type, CloType count_type, GError** err);
void clo_segreduce_destroy(CloSegReduce* sr);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the segment
 * ends of the counts form, a few words per tile) belongs to one queue at a time and only grows. */
CCLEvent* clo_segreduce_with_device_data(CloSegReduce* sr, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* aggr_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err);
/* Blocking: copy in, run, copy the m = min(numel_seg, *num_in) rows of aggr_out and total back. cq_exec NULL: a queue
 * of its own; cq_comm NULL: cq_exec. */
cl_bool clo_segreduce_with_host_data(CloSegReduce* sr, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	void* aggr_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err);

CCLContext* clo_segreduce_get_context(CloSegReduce* sr);
const char* clo_segreduce_get_op(CloSegReduce* sr);
const char* clo_segreduce_get_form(CloSegReduce* sr);
CloType clo_segreduce_get_value_type(CloSegReduce* sr);
size_t clo_segreduce_get_value_size(CloSegReduce* sr);
CloType clo_segreduce_get_sum_type(CloSegReduce* sr);
size_t clo_segreduce_get_sum_size(CloSegReduce* sr);
CloType clo_segreduce_get_count_type(CloSegReduce* sr);
size_t clo_segreduce_get_count_size(CloSegReduce* sr);

#ifdef __cplusplus
}
#endif
#endif
