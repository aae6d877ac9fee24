/*
 * clo_join.h — CloJoin: the equi-join of two arrays of keys that are already sorted, as pairs of row indices: inner,
 * left, right and full outer. NOT upstream (the reference has sort, scan and rng only). Which row of a sorted table B
 * matches which row of a sorted batch A — what clo_merge_*, clo_search_*, clo_setop_* and clo_expand_* were so far
 * assembled into by hand, in one call that also says how large the result is before any buffer for it exists.
 *
 * Inputs as for clo_merge_* and clo_setop_*: keys_a[0, numel_a) and keys_b[0, numel_b) of any CloType, each ascending
 * in the by-key sort's order (unsigned keys by their bits, signed keys numerically, half / float / double in IEEE total
 * order). Two keys are EQUAL iff their bits are equal: -0 and +0 are different keys, NaNs are equal by payload.
 *
 * kind is one of CLO_JOIN_KINDS. Let a key x occur at rows a0 .. a0 + m - 1 of A and at rows b0 .. b0 + n - 1 of B. The
 * rows (idx_a, idx_b) for x are
 *
 *   m > 0 and n > 0     the m * n pairs (a0 + i, b0 + j), ordered by i, then by j          every kind
 *   m > 0 and n = 0     the m rows (a0 + i, CLO_JOIN_NONE)                                 "left" and "full" only
 *   m = 0 and n > 0     the n rows (CLO_JOIN_NONE, b0 + j)                                 "right" and "full" only
 *
 * and the result is the concatenation of these groups in ASCENDING KEY ORDER, for all four kinds: unmatched rows of B
 * stand where their key belongs, not at the end. The result is therefore sorted by key and can go into the next join
 * or into clo_reduce_by_key_* without a sort.
 *
 * Outputs: idx_a_out and idx_b_out are arrays of uint; keys_out holds the row's key with its original bits, taken from
 * whichever side has it. Any of the three may be NULL. `capacity` (< 2^32) is the number of rows each output that is
 * not NULL can hold. num_out is one cl_ulong of device memory, 8-byte aligned, required: it receives the row count K of
 * the WHOLE join, also when K > capacity, and K may be above 2^32 (one key m times in A and n times in B gives m * n
 * rows). Exactly the first min(K, capacity) rows are written; nothing is written at an index >= min(K, capacity).
 * Count form: all three outputs NULL and capacity 0 writes num_out alone — this is how a caller sizes its buffers.
 * Either input may be empty (a left join against an empty B gives numel_a rows); with both empty K = 0, which the
 * host form finds without a device.
 *
 * Unsorted inputs: the contents and K are unspecified, but every read stays inside the inputs, every write inside [0,
 * capacity) of the outputs, every index written is below its side's numel or is CLO_JOIN_NONE, and the call completes.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL; nothing is written): an unknown kind; options
 * other than NULL or ""; numel_a + numel_b >= 2^32; capacity >= 2^32; NULL keys of a non-empty input; num_out NULL
 * (device form: not 8-byte aligned, or a buffer below 8 bytes); capacity > 0 with all outputs NULL; any output (sized
 * by capacity) or num_out that overlaps an input or another output.
 *
 * Out of scope: values carried along (gather with the indices), a key field inside a wider element
 * (get_key), descending order, non-equi joins, 64-bit row indices, unsorted inputs (sort first).
 */
#ifndef CLO_JOIN_H
#define CLO_JOIN_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_JOIN_KINDS "inner, left, right, full"
#define CLO_JOIN_NONE 0xFFFFFFFFu

typedef struct clo_join CloJoin;

/* Works on a context without a device (ccl_context_new_offline). */
CloJoin* clo_join_new(const char* kind, const char* options, CCLContext* ctx, CloType key_type, GError** err);
void clo_join_destroy(CloJoin* jn);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (split points,
 * tile offsets, one 16-byte entry per input element, the output tiles' first emitters) belongs to one queue at a time
 * and only grows. */
CCLEvent* clo_join_with_device_data(CloJoin* jn, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_a, size_t numel_a, CCLBuffer* keys_b, size_t numel_b,
	CCLBuffer* idx_a_out, CCLBuffer* idx_b_out, CCLBuffer* keys_out, size_t capacity, CCLBuffer* num_out, GError** err);
/* Blocking: copy in, run, read K, copy the min(K, capacity) rows out; *num_out = K. cq_exec NULL: a queue of its own;
 * cq_comm NULL: cq_exec. */
cl_bool clo_join_with_host_data(CloJoin* jn, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_a, size_t numel_a, const void* keys_b, size_t numel_b,
	cl_uint* idx_a_out, cl_uint* idx_b_out, void* keys_out, size_t capacity, size_t* num_out, GError** err);

CCLContext* clo_join_get_context(CloJoin* jn);
CloType clo_join_get_key_type(CloJoin* jn);
size_t clo_join_get_key_size(CloJoin* jn);
const char* clo_join_get_kind(CloJoin* jn);
/* The largest K a join of this kind can have for inputs of these sizes (one key everywhere, or no key shared),
 * saturating at SIZE_MAX. An upper bound only, not a capacity the calls require: use the count form. */
size_t clo_join_get_max_numel_out(CloJoin* jn, size_t numel_a, size_t numel_b);

#ifdef __cplusplus
}
#endif
#endif
