/*
 * clo_segtopk.h — CloSegTopK: the k smallest or largest rows of every segment of an array, the segments given by counts
 * or by CSR offsets. NOT upstream (the reference has sort, scan and rng only). The "k per segment" that the out-of-scope
 * lines of clo_topk.h, clo_segarg.h and clo_segsort.h name: the k nearest candidates per query, the k best edges per
 * vertex, a beam of k per sequence of ragged length. CloTopK does it for one array, CloSegArg for k = 1, CloSegSort
 * sorts every segment completely; this one sorts every tile of rows on chip once and combines, for a segment that spans
 * several tiles, only the k candidates of each tile.
 *
 * A caller with k = 1 should use CloSegArg (one read of the rows, no sort); a caller with ONE huge segment CloTopK (a
 * radix select); a caller who needs more than the cap on k CloSegSort and the first rows of every segment.
 *
 * which is one of CLO_SEGTOPK_WHICH, form one of CLO_SEGREDUCE_FORMS (clo_segreduce.h); count_type is uint or ulong for
 * both forms. The segments are clo_segsort.h's, word for word: with m_h = numel_seg and m = min(m_h, *num_in) when num_in
 * is given (one cl_ulong of device memory, 8-byte aligned; the host form: a host size_t), else m_h:
 *
 *   form "counts"   counts_or_offsets holds m_h counts c_r. e_r = c_0 + .. + c_r in 64-bit arithmetic, s_r = e_(r-1),
 *                   s_0 = 0, total = e_(m-1), 0 for m = 0. Entries at r >= m are not part of the sum.
 *   form "offsets"  counts_or_offsets holds m_h + 1 offsets, ascending (the precondition); entries [0, m] are read.
 *                   With base = offsets[0]: s_r = offsets[r] - base, e_r = offsets[r + 1] - base, total = offsets[m] -
 *                   base. offsets[0] = 0 is a CSR row pointer, anything else a slice of one, rebased.
 *
 * With n = numel, segment r < m covers rows [min(s_r, n), min(e_r, n)), len_r of them.
 *
 * The order is CloTopK's: the by-key total order for all eleven key types — unsigned keys by their bits, signed keys
 * numerically, half / float / double in IEEE total order (-NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN, NaNs by
 * payload). Keys are equal iff their bits are equal. With c_r = min(k, len_r):
 *   which "smallest"   the first c_r rows of the stable ascending sort of the clipped segment.
 *   which "largest"    the first c_r rows of the stable sort by the complemented order key: the largest key comes first,
 *                      and ties go by ASCENDING row index. This is not the reversed ascending sort.
 * The result is fully determined by the input: two calls agree bit for bit.
 *
 * The outputs are dense with stride k: keys_out[r * k + j] and values_out[r * k + j], for j < c_r, are the j-th chosen
 * row of segment r in the order above, so that every segment's rows come out sorted. Keys are written with their
 * original bits; values are opaque words of value_size 0 (none), 4 or 8 bytes. ARG form: value_size 4 and values_in
 * NULL; values_out then holds the GLOBAL row index as uint, and keys_out may be NULL. counts_out[r] = c_r (a cl_uint,
 * required) for every r < m. NOT written: slots j >= c_r of a row of the outputs, rows r >= m, and counts_out[r >= m];
 * a caller who wants padding fills the outputs first. num_out (one cl_ulong of device memory, 8-byte aligned; the host
 * form: a size_t; required) receives total UNCLAMPED: num_out > numel tells the caller that segments were clipped.
 * m = 0 writes num_out = 0 and nothing else (the host form returns then without a device). k = 0 succeeds and writes
 * num_out and nothing else. There is no in-place form.
 *
 * k is a host argument, consumed when the call is enqueued. 1 <= k <= clo_hip_segtopk_k_max(key_size, value_size)
 * (include/clo_hip.h): 1024, half a tile of rows, for every size built; above the cap the call is refused.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * an unknown which or form; options other than NULL or ""; a value_size other than 0, 4 or 8; a count_type other than
 * uint or ulong; numel_seg or numel >= 2^32; k above the cap; m_h * k >= 2^32; NULL counts_or_offsets with numel_seg > 0,
 * and in the offsets form always; NULL keys_in with numel > 0; values passed with value_size 0; values_out NULL with
 * value_size > 0; NULL values_in with value_size 8; keys_out NULL outside the arg form; counts_out NULL with
 * numel_seg > 0 and k > 0; num_out NULL (device form: misaligned, or below 8 bytes); num_in misaligned or below 8 bytes
 * (device form); a buffer too small (counts_or_offsets for m_h counts or m_h + 1 offsets, keys_in and values_in for
 * numel rows, keys_out and values_out for m_h * k rows, counts_out for m_h cl_uints); any output overlapping an input,
 * num_in, num_out or another output.
 *
 * Whatever the arrays hold — offsets that do not ascend, ends that wrap 2^64, a *num_in above m_h, a scribbled
 * workspace — every read stays inside the inputs, every write stays inside [0, m_h * k) of keys_out and values_out,
 * counts_out[0, m_h) and num_out, and the call completes; the contents are then unspecified.
 *
 * Out of scope: k per segment read from device memory, a compacted (CSR) output, padding, get_key /
 * run-time comparisons, numel >= 2^32, values wider than 8 bytes, a k above the cap.
 */
#ifndef CLO_SEGTOPK_H
#define CLO_SEGTOPK_H

#include "clo_common.h"
#include "clo_segreduce.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_SEGTOPK_WHICH "smallest, largest"

typedef struct clo_segtopk CloSegTopK;

/* Works on a context without a device (ccl_context_new_offline). */
CloSegTopK* clo_segtopk_new(const char* which, const char* form, const char* options, CCLContext* ctx,
	CloType key_type, size_t value_size, CloType count_type, GError** err);
void clo_segtopk_destroy(CloSegTopK* st);

/* Asynchronous on cq_exec; never synchronises the device and never reads anything back to the host. cq_comm is not
 * used. The object's workspace (a byte and a segment number per row, the segment ends of the counts form, two lists of
 * k candidates per tile) belongs to one queue at a time and only grows. */
CCLEvent* clo_segtopk_with_device_data(CloSegTopK* st, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* keys_in, CCLBuffer* values_in,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* counts_out, CCLBuffer* num_out,
	size_t numel_seg, size_t numel, size_t k, GError** err);
/* Blocking: copy in (the outputs too, so that what is not written keeps the caller's contents), run, copy the
 * m = min(numel_seg, *num_in) rows of k slots of the outputs, the m counts and total back. cq_exec NULL: a queue of its
 * own; cq_comm NULL: cq_exec. */
cl_bool clo_segtopk_with_host_data(CloSegTopK* st, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, cl_uint* counts_out, size_t* num_out,
	size_t numel_seg, size_t numel, size_t k, GError** err);

CCLContext* clo_segtopk_get_context(CloSegTopK* st);
const char* clo_segtopk_get_which(CloSegTopK* st);
const char* clo_segtopk_get_form(CloSegTopK* st);
CloType clo_segtopk_get_key_type(CloSegTopK* st);
size_t clo_segtopk_get_key_size(CloSegTopK* st);
size_t clo_segtopk_get_value_size(CloSegTopK* st);
CloType clo_segtopk_get_count_type(CloSegTopK* st);
size_t clo_segtopk_get_count_size(CloSegTopK* st);

#ifdef __cplusplus
}
#endif
#endif
