/*
 * clo_topk.h — CloTopK: the k smallest or largest keys of an array, with values carried along or the indices written,
 * and the k-th key itself. NOT upstream (the reference has sort, scan and rng only). The k best scores and who holds
 * them (topk / argtopk), a quantile or nth_element, the pivot of a partition computed where the data is. It is the
 * "top-k" that the out-of-scope line of clo_select.h names: a radix select on the device finds the k-th key without a
 * sort and without a host wait, and a compaction in CloSelect's shape cuts the ties at an exact rank, which CloSelect
 * cannot do (it keeps all of the "eq" elements or none).
 *
 * which is one of CLO_TOPK_WHICH, order one of CLO_TOPK_ORDERS.
 *
 * The order is the by-key sort's total order for all eleven key types: unsigned keys by their bits, signed keys
 * numerically, half / float / double in IEEE total order (-0 < +0, NaNs at the ends by sign and payload). Keys are
 * equal iff their bits are equal.
 *
 * Let m = min(k, numel).
 *   which "smallest"   the chosen elements are the first m of the stable ascending sort of the keys.
 *   which "largest"    the first m of the stable sort by the complemented order key: the largest key comes first.
 * In both the lower index comes first among equal keys: where the m-th key has ties, the tied elements with the lowest
 * indices are taken. The result is fully determined by the input: two calls agree bit for bit.
 *
 *   order "input"      the m chosen rows in increasing input index (stable, as a select would write them).
 *   order "sorted"     the m rows in the order of the sort above ("largest": descending, ties by ascending index).
 *                      Provided for m <= clo_hip_topk_sorted_max(key_size, value_size) (include/clo_hip.h; 4096 for
 *                      every size built): one work-group sorts the m compacted rows in LDS. Above that the call is
 *                      refused; take "input" order and chain clo_sort_by_key_* on the m rows. A sorted form for any k
 *                      is out of scope.
 *
 * Exactly m rows of keys_out / values_out are written; rows >= m are NOT touched and the outputs need hold m rows only.
 *
 * kth_out (optional, may be NULL) is one key of key_type in device memory, aligned to the key (the host form: a host
 * pointer to one key). It receives the key of the m-th chosen element in the sort's order — the largest of the m
 * smallest, the smallest of the m largest — with its original bits. It is written on the same queue, so a CloSelect
 * with pred "lt" / "le" / "gt" / "ge" can take it as its threshold with no host wait in between. It is not written
 * when m == 0. With kth_out given both outputs may be NULL (value_size 0): only the k-th key is computed.
 *
 * Values are opaque words of value_size bytes, 0 (none), 4 or 8: values_out[j] belongs to keys_out[j]. Arg form:
 * value_size 4 and values_in NULL: values_out[j] is the element's index i. keys_out may then be NULL.
 *
 * k is a host argument, consumed when the call is enqueued. numel == 0 or k == 0 succeeds and writes nothing (the host
 * form does so without a device).
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is
 * written): an unknown which or order; options other than NULL or ""; a value_size other than 0, 4 or 8; values passed
 * with value_size 0; NULL values_in with value_size 8; values_out NULL with value_size > 0; both outputs NULL and
 * kth_out NULL; NULL keys_in with numel > 0; numel >= 2^32; an input buffer below numel rows or an output below m rows;
 * kth_out below one key or misaligned; "sorted" with m above the cap; any of keys_out, values_out (each sized m rows)
 * and kth_out overlapping an input or one another. There is no in-place form.
 *
 * Whatever the arrays hold, every read stays inside the inputs, every write inside rows [0, m) and kth_out, and the
 * call completes.
 *
 * Out of scope: sorted output above the cap, numel >= 2^32, a key field inside a wider element
 * (get_key), k per segment (see clo_segtopk.h), k read from device memory.
 */
#ifndef CLO_TOPK_H
#define CLO_TOPK_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_TOPK_WHICH "smallest, largest"
#define CLO_TOPK_ORDERS "input, sorted"

typedef struct clo_topk CloTopK;

/* Works on a context without a device (ccl_context_new_offline). */
CloTopK* clo_topk_new(const char* which, const char* order, const char* options, CCLContext* ctx, CloType key_type, size_t value_size, GError** err);
void clo_topk_destroy(CloTopK* topk);

/* Asynchronous on cq_exec; never synchronises the device and never reads anything back to the host. cq_comm is not
 * used. The object's workspace (digit tables, the k-th key found, the tiles' counts) belongs to one queue at a time and
 * only grows. */
CCLEvent* clo_topk_with_device_data(CloTopK* topk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out, CCLBuffer* values_out, CCLBuffer* kth_out,
	size_t numel, size_t k, GError** err);
/* Blocking: copy in, run, copy the m rows and the k-th key out. cq_exec NULL: a queue of its own; cq_comm NULL:
 * cq_exec. */
cl_bool clo_topk_with_host_data(CloTopK* topk, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* kth_out,
	size_t numel, size_t k, GError** err);

CCLContext* clo_topk_get_context(CloTopK* topk);
CloType clo_topk_get_key_type(CloTopK* topk);
size_t clo_topk_get_key_size(CloTopK* topk);
size_t clo_topk_get_value_size(CloTopK* topk);
const char* clo_topk_get_which(CloTopK* topk);
const char* clo_topk_get_order(CloTopK* topk);

#ifdef __cplusplus
}
#endif
#endif
