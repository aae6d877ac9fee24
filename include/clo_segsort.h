/*
 * clo_segsort.h — CloSegSort: a stable ascending sort of every segment of an array on its own, the segments given by
 * counts or by CSR offsets. NOT upstream (the reference has sort, scan and rng only). The third member of the CSR
 * tool-box beside clo_expand.h and clo_segreduce.h: the column indices of CSR rows, ranking inside sequences of
 * different lengths, ordering inside groups. Millions of short segments cost one read and one write of every row;
 * a caller with a FEW HUGE segments should call clo_sort_* on each instead (a segment of 2^28 rows is moved about 17
 * times here).
 *
 * form is one of CLO_SEGSORT_FORMS; count_type is uint or ulong for both forms. The segments are exactly
 * clo_expand.h's and clo_segreduce.h's: with m_h = numel_seg and m = min(m_h, *num_in) when num_in is given (one
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
 * Keys are of any CloType; the key is the whole element. They compare in the order clo_merge.h and clo_sort_by_key_*
 * document: unsigned types by their bits, signed types numerically, half / float / double in IEEE total order (-NaN <
 * -inf < .. < -0 < +0 < .. < +inf < +NaN). Keys are written with their original bits.
 *
 * With n = numel, segment r < m covers rows [min(s_r, n), min(e_r, n)). keys_out restricted to those rows holds that
 * segment's keys ascending; equal keys keep their input order: bit for bit a STABLE sort of each clipped segment.
 * values_out[j] is the value of the row that moved to j; values are opaque words of value_size 0 (none), 4 or 8 bytes.
 * ARG form: value_size 4 and values_in NULL; values_out[j] is then the GLOBAL row index, as uint, of the row that moved
 * to j (clo_sort_by_key_*'s convention), and keys_out may be NULL. Rows i >= min(total, n) of the outputs (which hold
 * numel rows) are NOT written. num_out (one cl_ulong of device memory, 8-byte aligned; the host form: a size_t;
 * required) receives total UNCLAMPED: num_out > numel tells the caller that segments were clipped. m = 0 writes
 * num_out = 0 and nothing else (the host form returns then without a device). There is no in-place form.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * an unknown form; options other than NULL or ""; a value_size other than 0, 4 or 8; a count_type other than uint or
 * ulong; numel_seg or numel >= 2^32; NULL counts_or_offsets with numel_seg > 0, and in the offsets form always; NULL
 * keys_in with numel > 0; values passed with value_size 0; values_out NULL with value_size > 0; NULL values_in with
 * value_size 8; keys_out NULL outside the arg form; num_out NULL (device form: misaligned, or below 8 bytes); num_in
 * misaligned or below 8 bytes (device form); a buffer too small (counts_or_offsets for m_h counts or m_h + 1 offsets,
 * keys_in, keys_out, values_in and values_out for numel rows); an output overlapping an input, num_in, num_out or the
 * other output.
 *
 * Whatever the arrays hold — offsets that do not ascend, sums that wrap 2^64, a *num_in above m_h, a scribbled
 * workspace — every read stays inside the inputs, every write stays inside [0, numel) of the outputs and num_out, and
 * the call completes; the contents are then unspecified.
 *
 * Out of scope: descending order, get_key / run-time comparisons, numel >= 2^32, values wider than
 * 8 bytes, the k smallest per segment (see clo_segtopk.h).
 */
#ifndef CLO_SEGSORT_H
#define CLO_SEGSORT_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_SEGSORT_FORMS "counts, offsets"

typedef struct clo_segsort CloSegSort;

/* Works on a context without a device (ccl_context_new_offline). */
CloSegSort* clo_segsort_new(const char* form, const char* options, CCLContext* ctx,
	CloType key_type, size_t value_size, CloType count_type, GError** err);
void clo_segsort_destroy(CloSegSort* ss);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (a second copy
 * of the rows, a byte per row, the segment ends of the counts form) belongs to one queue at a time and only grows. */
CCLEvent* clo_segsort_with_device_data(CloSegSort* ss, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* keys_in, CCLBuffer* values_in,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err);
/* Blocking: copy in, run, copy the min(total, numel) rows of the outputs and total back. cq_exec NULL: a queue of its
 * own; cq_comm NULL: cq_exec. */
cl_bool clo_segsort_with_host_data(CloSegSort* ss, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err);

CCLContext* clo_segsort_get_context(CloSegSort* ss);
const char* clo_segsort_get_form(CloSegSort* ss);
CloType clo_segsort_get_key_type(CloSegSort* ss);
size_t clo_segsort_get_key_size(CloSegSort* ss);
size_t clo_segsort_get_value_size(CloSegSort* ss);
CloType clo_segsort_get_count_type(CloSegSort* ss);
size_t clo_segsort_get_count_size(CloSegSort* ss);

#ifdef __cplusplus
}
#endif
#endif
