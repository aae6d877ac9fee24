/*
 * clo_segarg.h — CloSegArg: WHERE the minimum or maximum of every segment of an array lies, and its value, the segments
 * given by counts or by CSR offsets. NOT upstream (the reference has sort, scan and rng only). The index half of
 * clo_segreduce.h's min and max: the best edge per vertex, the nearest candidate per query, arg-max pooling over sequences
 * of different lengths, the column of a row's pivot — callers that gather other columns by the row found. Unlike the
 * sums of the segment family, a minimum does not depend on the order of evaluation, so floating-point values are taken.
 *
 * op is one of CLO_SEGARG_OPS, tie one of CLO_SEGARG_TIES, form one of CLO_SEGREDUCE_FORMS (clo_segreduce.h);
 * count_type is uint or ulong for both forms. The segments are clo_segreduce.h's, word for word: with m_h = numel_seg and
 * m = min(m_h, *num_in) when num_in is given (one cl_ulong of device memory, 8-byte aligned; the host form: a host
 * size_t), else m_h:
 *
 *   form "counts"   counts_or_offsets holds m_h counts c_r. e_r = c_0 + .. + c_r in 64-bit arithmetic, s_r = e_(r-1),
 *                   s_0 = 0, total = e_(m-1), 0 for m = 0. Entries at r >= m are not part of the sum.
 *   form "offsets"  counts_or_offsets holds m_h + 1 offsets, ascending (the precondition); entries [0, m] are read.
 *                   With base = offsets[0]: s_r = offsets[r] - base, e_r = offsets[r + 1] - base, total = offsets[m] -
 *                   base. offsets[0] = 0 is a CSR row pointer, anything else a slice of one, rebased.
 *
 * num_in exists so that a device-side segment count (num_runs_out of clo_reduce_by_key_with_device_data, CloBucket's
 * offsets with their count) is passed straight in, on the same queue and with no host wait.
 *
 * The order. x(i) is the ORDER KEY of values_in[i], an unsigned number of the value's width: the bits themselves for
 * uint and ulong; the sign bit flipped for int and long; for float and double every bit flipped where the sign bit is
 * set and the sign bit flipped elsewhere, which is the IEEE total order
 *     -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN,
 * NaNs among themselves by their payloads. Two values have the same key exactly when their bits are the same. For
 * "argmax" x(i) is complemented, and everything below reads the same.
 *
 * With n = numel, the rows of values_in, for every r < m whose clipped range [min(s_r, n), min(e_r, n)) holds a row:
 *     idx_out[r] (a cl_uint) = the row i of that range with the smallest x(i); among equal x the smallest i for tie
 *                              "first", the largest for "last". i indexes values_in, whatever offsets[0] is.
 *     val_out[r]             = values_in[i], bit for bit: a -0.0 and a NaN's payload survive.
 * A segment without a row — an empty one, or one that lies beyond n altogether — receives idx_out[r] = CLO_SEGARG_NONE
 * and val_out[r] = the value that comes LAST in the order for argmin and FIRST for argmax:
 *     uint 0xffffffff / 0; int INT_MAX / INT_MIN; float the bit patterns 0x7fffffff / 0xffffffff (+NaN and -NaN with
 *     every payload bit set); long, ulong and double likewise in 64 bits.
 * For the four integer types these are clo_segreduce.h's identities, and val_out is its min or max. Whether a segment
 * has a row is decided from its clipped ends, never from a sentinel: a row that holds that last value, row 0 under
 * "last" included, is reported like any other.
 *
 * val_out may be NULL (indices only). Rows r >= m of idx_out and val_out (which hold m_h rows) are NOT written. num_out
 * (one cl_ulong of device memory, 8-byte aligned, required) receives total UNCLAMPED: num_out > numel tells the caller
 * that segments were clipped. m = 0 writes num_out = 0 and nothing else (the host form returns then without a device).
 *
 * Value types: int, uint, long, ulong, float, double. count_type: uint or ulong.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * an unknown op, tie or form; options other than NULL or ""; a value type outside the six, a count_type other than uint
 * or ulong; numel_seg or numel >= 2^32; NULL counts_or_offsets with numel_seg > 0, and in the offsets form always; NULL
 * values_in with numel > 0; NULL idx_out with numel_seg > 0; num_out NULL (device form: misaligned, or below 8 bytes);
 * num_in misaligned or below 8 bytes (device form); a buffer too small (counts_or_offsets for m_h counts or m_h + 1
 * offsets, values_in for numel rows, idx_out for m_h cl_uints, val_out for m_h values); idx_out, val_out or num_out
 * overlapping an input, num_in or one another.
 *
 * Whatever the arrays hold — offsets that do not ascend, ends that wrap 2^64, a *num_in above m_h — every read stays
 * inside the inputs, every write stays inside idx_out[0, m_h), val_out[0, m_h) and num_out, and the call completes; the
 * contents are then unspecified.
 *
 * Out of scope: half and narrower value types, get_key expressions, several value columns per
 * call, a segment-relative index, the k smallest per segment (see clo_segtopk.h), numel >= 2^32.
 */
#ifndef CLO_SEGARG_H
#define CLO_SEGARG_H

#include "clo_common.h"
#include "clo_segreduce.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_SEGARG_OPS  "argmin, argmax"
#define CLO_SEGARG_TIES "first, last"
#define CLO_SEGARG_NONE 0xffffffffu

typedef struct clo_segarg CloSegArg;

/* Works on a context without a device (ccl_context_new_offline). */
CloSegArg* clo_segarg_new(const char* op, const char* tie, const char* form, const char* options, CCLContext* ctx,
	CloType value_type, CloType count_type, GError** err);
void clo_segarg_destroy(CloSegArg* sa);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the segment
 * ends of the counts form, a few words per tile) belongs to one queue at a time and only grows. */
CCLEvent* clo_segarg_with_device_data(CloSegArg* sa, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* idx_out, CCLBuffer* val_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err);
/* Blocking: copy in, run, copy the m = min(numel_seg, *num_in) rows of idx_out and of val_out (where given) and total
 * back. cq_exec NULL: a queue of its own; cq_comm NULL: cq_exec. */
cl_bool clo_segarg_with_host_data(CloSegArg* sa, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	cl_uint* idx_out, void* val_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err);

CCLContext* clo_segarg_get_context(CloSegArg* sa);
const char* clo_segarg_get_op(CloSegArg* sa);
const char* clo_segarg_get_tie(CloSegArg* sa);
const char* clo_segarg_get_form(CloSegArg* sa);
CloType clo_segarg_get_value_type(CloSegArg* sa);
size_t clo_segarg_get_value_size(CloSegArg* sa);
CloType clo_segarg_get_count_type(CloSegArg* sa);
size_t clo_segarg_get_count_size(CloSegArg* sa);

#ifdef __cplusplus
}
#endif
#endif
