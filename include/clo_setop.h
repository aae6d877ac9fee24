/*
 * clo_setop.h — CloSetOp: union, intersection, difference and symmetric difference of two arrays that are already
 * sorted, as multisets, with values carried along or the indices written. NOT upstream (the reference has sort, scan
 * and rng only). Which rows of a sorted batch are not yet in the sorted table (difference, the anti-join), which are in
 * both (intersection, the semi-join), the table extended by the rows it lacks (union), what changed between two
 * snapshots (symmetric difference).
 *
 * Inputs as for clo_merge_* (include/clo_merge.h): keys_a[0, numel_a) and keys_b[0, numel_b) of any CloType, each
 * ascending in the by-key sort's order (unsigned keys by their bits, signed keys numerically, half / float / double in
 * IEEE total order). Two keys are EQUAL iff their bits are equal: -0 and +0 are different keys, NaNs are equal by
 * payload.
 *
 * The operations are those of std::set_* and thrust::set_* on multisets. Let a key x occur m times in A and n times in
 * B, let A's element be the r-th of its run and B's the s-th of its run (0-based):
 *
 *   op                      kept from A   kept from B   copies of x
 *   "union"                 all           s >= m        max(m, n)
 *   "intersection"          r < n         none          min(m, n)
 *   "difference"            r >= n        none          max(m - n, 0)
 *   "symmetric_difference"  r >= n        s >= m        |m - n|
 *
 * The kept elements are written in merge order: ascending, equal keys of A before those of B, input order kept inside
 * each — the output is the subsequence of clo_merge_*'s output that the table selects. Keys keep their original bits.
 * Values are opaque words of value_size bytes, 0 (none), 4 or 8: values_out[j] is the value of the element at
 * keys_out[j]. Intersection and difference keep no element of B: values_b is never looked at and may be NULL.
 * Arg form: value_size 4 and NULL input values: values_out[j] is the element's index in A || B (i for A[i], numel_a + i
 * for B[i]; for intersection and difference these are indices into A). keys_out may then be NULL.
 *
 * num_out is one cl_ulong of device memory, 8-byte aligned, required (as num_runs_out of clo_reduce_by_key_*). It
 * receives the number k of elements written; entries at index >= k are NOT written. The outputs must hold the op's
 * capacity, clo_setop_get_max_numel_out(): numel_a + numel_b for union and symmetric difference, min(numel_a, numel_b)
 * for intersection, numel_a for difference. Either input may be empty; with both empty the call succeeds and num_out
 * still becomes 0 (the host form does this without a device).
 *
 * Unsorted inputs: the contents and k are unspecified, but every read stays inside the inputs, every write inside [0,
 * capacity) of the outputs, k <= capacity, and the call completes.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL; nothing is written): clo_merge's list (a
 * value_size other than 0, 4 or 8; options other than NULL or ""; n >= 2^32; NULL keys of a non-empty input; exactly
 * one of values_a / values_b NULL where both are looked at; values passed with value_size 0; values_out NULL with
 * value_size > 0; NULL values with value_size 8; both outputs NULL), an unknown op, num_out NULL (device form: not
 * 8-byte aligned, or a buffer below 8 bytes), and any of keys_out, values_out (each sized by the capacity) and num_out
 * that overlaps an input or another of the three.
 *
 * Out of scope: descending order, a key field inside a wider element (get_key), run-time compiled
 * comparisons, more than two inputs, 64-bit positions, a deduplicating mode (for the set of DISTINCT keys run
 * clo_reduce_by_key_* with keys_out alone first).
 */
#ifndef CLO_SETOP_H
#define CLO_SETOP_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_SETOP_OPS "union, intersection, difference, symmetric_difference"

typedef struct clo_setop CloSetOp;

/* Works on a context without a device (ccl_context_new_offline). */
CloSetOp* clo_setop_new(const char* op, const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err);
void clo_setop_destroy(CloSetOp* so);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the tiles'
 * split points and kept counts) belongs to one queue at a time and only grows. */
CCLEvent* clo_setop_with_device_data(CloSetOp* so, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_a, CCLBuffer* values_a, size_t numel_a,
	CCLBuffer* keys_b, CCLBuffer* values_b, size_t numel_b,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* num_out, GError** err);
/* Blocking: copy in, run, read k, copy the k rows out. cq_exec NULL: a queue of its own; cq_comm NULL: cq_exec. */
cl_bool clo_setop_with_host_data(CloSetOp* so, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_a, const void* values_a, size_t numel_a,
	const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, size_t* num_out, GError** err);

CCLContext* clo_setop_get_context(CloSetOp* so);
CloType clo_setop_get_key_type(CloSetOp* so);
size_t clo_setop_get_key_size(CloSetOp* so);
size_t clo_setop_get_value_size(CloSetOp* so);
const char* clo_setop_get_op(CloSetOp* so);
/* The elements keys_out and values_out must hold for inputs of these sizes. */
size_t clo_setop_get_max_numel_out(CloSetOp* so, size_t numel_a, size_t numel_b);

#ifdef __cplusplus
}
#endif
#endif
