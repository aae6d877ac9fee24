/*
 * clo_select.h — CloSelect: stable selection and partition of an array by flags or by comparison with a threshold,
 * with values carried along or the indices written. NOT upstream (the reference has sort, scan and rng only). The rows
 * whose flag is set, the keys below a pivot, the indices of the nonzero entries (nonzero / argpartition), a filter
 * between a sort and a reduce by key.
 *
 * op is one of CLO_SELECT_OPS, pred one of CLO_SELECT_PREDS.
 *
 *   pred "flagged"     flags_or_threshold holds numel bytes (cl_uchar); element i is KEPT iff flags[i] != 0. The keys
 *                      are opaque.
 *   pred "lt" .. "ne"  flags_or_threshold holds ONE key of key_type in device memory (the host form: a host pointer to
 *                      one key), so that a pivot computed on the device chains without a host wait. keys_in[i] is kept
 *                      iff keys_in[i] <pred> threshold in the by-key sort's order: unsigned keys by their bits, signed
 *                      keys numerically, half / float / double in IEEE total order. The order is total, so "eq" means
 *                      equal bits: -0 is not +0, NaNs compare by payload.
 *
 *   op "select"        the k kept elements are written in input order to rows [0, k); rows >= k are NOT written.
 *   op "partition"     the kept elements go to rows [0, k) in input order, the rejected ones to rows [k, numel), ALSO in
 *                      input order (both sides are stable): all numel rows are written.
 *
 * num_out is one cl_ulong of device memory, 8-byte aligned, required (as num_runs_out of clo_reduce_by_key_*); it
 * receives k. The outputs hold numel rows for both ops.
 *
 * Values are opaque words of value_size bytes, 0 (none), 4 or 8: values_out[j] belongs to keys_out[j]. Arg form:
 * value_size 4 and values_in NULL: values_out[j] is the element's index i. keys_out may then be NULL, and with "flagged"
 * keys_in too (the indices of the set flags alone).
 *
 * numel == 0 succeeds and num_out becomes 0 (the host form does this without a device).
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * an unknown op or pred; options other than NULL or ""; a value_size other than 0, 4 or 8; values passed with
 * value_size 0; values_out NULL with value_size > 0; NULL values_in with value_size 8; both outputs NULL; NULL keys_in
 * where the keys are read (a comparison, or keys_out given; numel > 0); NULL flags_or_threshold (but the flags of
 * numel 0); a flags buffer below numel bytes or a threshold buffer below one key; numel >= 2^32; num_out NULL (device
 * form: misaligned, or below 8 bytes); any of keys_out, values_out (each sized numel rows) and num_out overlapping an
 * input, the flags, the threshold or one another. There is no in-place form.
 *
 * Whatever the arrays hold, every read stays inside the inputs and every write inside [0, numel) of the outputs,
 * k <= numel, and the call completes.
 *
 * Out of scope: a single sweep that reads the input once, run-time compiled predicates,
 * numel >= 2^32, a key field inside a wider element (get_key), top-k.
 */
#ifndef CLO_SELECT_H
#define CLO_SELECT_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_SELECT_OPS "select, partition"
#define CLO_SELECT_PREDS "flagged, lt, le, gt, ge, eq, ne"

typedef struct clo_select CloSelect;

/* Works on a context without a device (ccl_context_new_offline). */
CloSelect* clo_select_new(const char* op, const char* pred, const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err);
void clo_select_destroy(CloSelect* sel);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the tiles' kept
 * counts) belongs to one queue at a time and only grows. */
CCLEvent* clo_select_with_device_data(CloSelect* sel, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* flags_or_threshold,
	CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* num_out, size_t numel, GError** err);
/* Blocking: copy in, run, read k, copy the rows out (k of a select, numel of a partition). cq_exec NULL: a queue of its
 * own; cq_comm NULL: cq_exec. */
cl_bool clo_select_with_host_data(CloSelect* sel, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, const void* flags_or_threshold,
	void* keys_out, void* values_out, size_t numel, size_t* num_out, GError** err);

CCLContext* clo_select_get_context(CloSelect* sel);
CloType clo_select_get_key_type(CloSelect* sel);
size_t clo_select_get_key_size(CloSelect* sel);
size_t clo_select_get_value_size(CloSelect* sel);
const char* clo_select_get_op(CloSelect* sel);
const char* clo_select_get_pred(CloSelect* sel);

#ifdef __cplusplus
}
#endif
#endif
