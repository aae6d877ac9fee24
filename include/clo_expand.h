/*
 * clo_expand.h — CloExpand: run-length decode and segment ids from counts or from CSR offsets. NOT upstream (the
 * reference has sort, scan and rng only). The inverse of clo_reduce_by_key_* (repeat_interleave), the second half of a
 * counting sort built on CloHistogram, the CSR to COO conversion, and the step that gives the by-key operations an
 * offsets form: the segment id of every row is a key.
 *
 * form is one of CLO_EXPAND_FORMS; count_type is uint or ulong for both. With m_h = numel_in and m = min(m_h, *num_in)
 * when num_in is given (one cl_ulong of device memory, 8-byte aligned; the host form: a host size_t), else m_h:
 *
 *   form "counts"   counts_or_offsets holds m_h counts c_r. e_r = c_0 + .. + c_r in 64-bit arithmetic, s_r = e_(r-1),
 *                   s_0 = 0, total = e_(m-1), 0 for m = 0. Entries at r >= m are not part of the sum.
 *   form "offsets"  counts_or_offsets holds m_h + 1 offsets, ascending (the precondition); entries [0, m] are read.
 *                   With base = offsets[0]: s_r = offsets[r] - base, e_r = offsets[r + 1] - base, total = offsets[m] -
 *                   base. offsets[0] = 0 is a CSR row pointer, anything else a slice of one, rebased.
 *
 * num_in exists so that num_runs_out of clo_reduce_by_key_with_device_data is passed straight in, numel_in being the
 * buffers' row count, on the same queue and with no host wait.
 *
 * For every row j in [0, min(total, capacity)), r(j) = the number of r < m with e_r <= j (empty segments own no row;
 * under the precondition r(j) < m):
 *     values_out[j] = values_in[r(j)]     opaque words of the size of value_type (1, 2, 4 or 8 bytes)
 *     seg_out[j]    = r(j)                cl_uint
 *     rank_out[j]   = j - s_r(j)          cl_uint
 * Each of the three is optional, at least one must be given, and values_out is given exactly when values_in is. Rows at
 * index >= min(total, capacity) are NOT written. num_out (one cl_ulong of device memory, 8-byte aligned, required)
 * receives total UNCLAMPED: a caller sees truncation as num_out > capacity, and a call with capacity 0 is the size query
 * that writes num_out alone. m = 0 gives total 0 (the host form returns then without a device).
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * an unknown form; options other than NULL or ""; a count_type other than uint or ulong; an invalid value_type; numel_in
 * or capacity >= 2^32; NULL counts_or_offsets with numel_in > 0, and in the offsets form with numel_in 0 too whenever
 * capacity > 0; all three outputs NULL; exactly one of values_in / values_out; num_out NULL (device form: misaligned, or
 * below 8 bytes); num_in misaligned or below 8 bytes (device form); a buffer too small (the inputs for m_h rows, m_h + 1
 * offsets; the outputs for capacity rows); any output (each sized capacity rows, and num_out) overlapping an input,
 * num_in or another output.
 *
 * Whatever the arrays hold — offsets that do not ascend, sums that wrap 2^64, a *num_in above m_h — every read stays
 * inside the inputs, every gathered index and every segment id written is below m_h, every write stays inside
 * [0, capacity) of the outputs and num_out, and the call completes.
 *
 * Out of scope: capacity >= 2^32, values wider than 8 bytes, a fused decode-and-gather of several
 * value columns.
 */
#ifndef CLO_EXPAND_H
#define CLO_EXPAND_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_EXPAND_FORMS "counts, offsets"

typedef struct clo_expand CloExpand;

/* Works on a context without a device (ccl_context_new_offline). value_type is looked at only where values are passed. */
CloExpand* clo_expand_new(const char* form, const char* options, CCLContext* ctx, CloType value_type, CloType count_type, GError** err);
void clo_expand_destroy(CloExpand* ex);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the segment
 * ends of the counts form, one word per tile) belongs to one queue at a time and only grows. */
CCLEvent* clo_expand_with_device_data(CloExpand* ex, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* values_out, CCLBuffer* seg_out, CCLBuffer* rank_out, CCLBuffer* num_out,
	size_t numel_in, size_t capacity, GError** err);
/* Blocking: copy in, run, read total, copy min(total, capacity) rows of each output back. cq_exec NULL: a queue of its
 * own; cq_comm NULL: cq_exec. */
cl_bool clo_expand_with_host_data(CloExpand* ex, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	void* values_out, void* seg_out, void* rank_out, size_t* num_out,
	size_t numel_in, size_t capacity, GError** err);

CCLContext* clo_expand_get_context(CloExpand* ex);
const char* clo_expand_get_form(CloExpand* ex);
CloType clo_expand_get_value_type(CloExpand* ex);
size_t clo_expand_get_value_size(CloExpand* ex);
CloType clo_expand_get_count_type(CloExpand* ex);
size_t clo_expand_get_count_size(CloExpand* ex);

#ifdef __cplusplus
}
#endif
#endif
