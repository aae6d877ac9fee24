/*
 * clo_merge.h — CloMerge: the stable merge of two arrays that are already sorted, with values carried along or the
 * permutation written (argmerge). NOT upstream (the reference has sort, scan and rng only). A sorted table and a sorted
 * batch of new rows, two sorted shards, runs sorted in pieces: instead of clo_sort_by_key_* on the concatenation (four
 * trips through memory) every element is read once and written once.
 *
 * Keys are of any CloType; the key is the whole element. They compare in the order clo_sort_by_key_* documents:
 * unsigned keys by their bits, signed keys numerically, half / float / double keys in IEEE total order (-0 < +0, NaNs
 * at the ends by sign). Two keys are EQUAL iff their bits are equal.
 *
 * Precondition: keys_a[0, numel_a) and keys_b[0, numel_b) are each ascending in that order.
 * Result, with n = numel_a + numel_b: keys_out holds the n keys ascending; among equal keys every element of A comes
 * before every element of B, and within A and within B the input order is kept. Equivalently: output position j holds
 * element p[j] of the concatenation A || B, where p is the STABLE argsort of the concatenation's keys — the merge is, bit
 * for bit, clo_sort_by_key_* of the concatenation. Keys are written with their original bits.
 * Values are opaque words of value_size bytes, 0 (none), 4 or 8: values_out[j] is the value of element p[j].
 * Argmerge: value_size 4, values_a and values_b NULL, a values_out: values_out[j] = p[j] as uint, where i stands for
 * A[i] and numel_a + i for B[i] (clo_sort_by_key_*'s convention that NULL values mean the index). keys_out may then be
 * NULL and only the permutation is written. The values pointer of an EMPTY input is not looked at.
 * Either input may be empty; the other is then copied. With both empty nothing is enqueued and the call succeeds
 * (the host form does this without a device).
 *
 * Unsorted inputs: the contents of the outputs are unspecified, but every read stays inside the inputs, every write
 * inside [0, n) of the outputs, and the call completes.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL; nothing is written): a value_size other than
 * 0, 4 or 8; options other than NULL or ""; n >= 2^32; NULL keys_a with numel_a > 0, and the same for B; exactly one
 * of values_a / values_b NULL while both inputs are non-empty; values passed with value_size 0; values_out NULL with
 * value_size > 0; NULL values with value_size 8; both outputs NULL; keys_out NULL with value_size 0; any output range
 * that overlaps an input range or the other output (there is no in-place form: a merge reads ahead of where it
 * writes).
 *
 * Out of scope: descending order, a key field inside a wider element (get_key), run-time compiled
 * comparisons, more than two inputs. The set operations on sorted arrays (union, intersection, difference, symmetric
 * difference) are CloSetOp, include/clo_setop.h.
 */
#ifndef CLO_MERGE_H
#define CLO_MERGE_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct clo_merge CloMerge;

/* Works on a context without a device (ccl_context_new_offline). */
CloMerge* clo_merge_new(const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err);
void clo_merge_destroy(CloMerge* m);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the tiles'
 * split points) belongs to one queue at a time and only grows. */
CCLEvent* clo_merge_with_device_data(CloMerge* m, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_a, CCLBuffer* values_a, size_t numel_a,
	CCLBuffer* keys_b, CCLBuffer* values_b, size_t numel_b,
	CCLBuffer* keys_out, CCLBuffer* values_out, GError** err);
/* Blocking: copy in, merge, copy out. cq_exec NULL: a queue of its own; cq_comm NULL: cq_exec. */
cl_bool clo_merge_with_host_data(CloMerge* m, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_a, const void* values_a, size_t numel_a,
	const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, GError** err);

CCLContext* clo_merge_get_context(CloMerge* m);
CloType clo_merge_get_key_type(CloMerge* m);
size_t clo_merge_get_key_size(CloMerge* m);
size_t clo_merge_get_value_size(CloMerge* m);

#ifdef __cplusplus
}
#endif
#endif
