/*
 * clo_search.h — CloSearch: the lower or upper bounds of many keys (the needles) in an array that is already sorted
 * (the haystack), a vectorised binary search. NOT upstream (the reference has sort, scan and rng only). What the sorts
 * and the merge produce can be looked things up in: the bin of a key in a table of edges is upper_bound - 1, the
 * number of matches of a probe key is upper - lower.
 *
 * Keys are of any CloType; the key is the whole element. They compare in the order clo_sort_by_key_* and clo_merge_*
 * document: unsigned keys by their bits, signed keys numerically, half / float / double keys in IEEE total order
 * (-0 < +0, NaNs at the ends by sign). Two keys are EQUAL iff their bits are equal.
 *
 * Precondition: haystack[0, numel_h) is ascending in that order.
 * Result: pos_out holds numel_n values of uint. Without flags (lower bound) pos_out[i] is the number of haystack keys
 * < needles[i]; with CLO_SEARCH_UPPER it is the number of haystack keys <= needles[i]. Every result is <= numel_h.
 * numel_h == 0 gives all zeros and reads no haystack: the haystack pointer is then not looked at. numel_n == 0
 * enqueues nothing and succeeds (the host form does this without a device).
 *
 * CLO_SEARCH_NEEDLES_SORTED is a promise by the caller that needles[0, numel_n) is ascending in the same order. It
 * selects the form that reads each touched haystack key once instead of once per needle that passes it. When the
 * promise holds the results are identical with and without the flag.
 *
 * A haystack that is not sorted, or needles that are not under the flag: the contents of pos_out are unspecified, but
 * every read stays inside the two inputs, every write inside pos_out[0, numel_n), every value written is <= numel_h,
 * and the call completes.
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL; nothing is written): options other than NULL or
 * ""; flag bits other than the two above; numel_h >= 2^32 or numel_n >= 2^32; NULL haystack with numel_h > 0; NULL
 * needles or NULL pos_out with numel_n > 0; pos_out overlapping the haystack or the needles (there is no in-place
 * form).
 *
 * Out of scope: equal_range in one call, 64-bit positions, a key field inside a wider element
 * (get_key), descending order.
 */
#ifndef CLO_SEARCH_H
#define CLO_SEARCH_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct clo_search CloSearch;

#define CLO_SEARCH_UPPER          1u   /* otherwise lower */
#define CLO_SEARCH_NEEDLES_SORTED 2u   /* the needles are ascending too */

/* Works on a context without a device (ccl_context_new_offline). */
CloSearch* clo_search_new(const char* options, CCLContext* ctx, CloType key_type, GError** err);
void clo_search_destroy(CloSearch* s);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the tiles'
 * ranges of the sorted-needles form) belongs to one queue at a time and only grows. */
CCLEvent* clo_search_with_device_data(CloSearch* s, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* haystack, size_t numel_h, CCLBuffer* needles, size_t numel_n,
	unsigned flags, CCLBuffer* pos_out, GError** err);
/* Blocking: copy in, search, copy out. cq_exec NULL: a queue of its own; cq_comm NULL: cq_exec. */
cl_bool clo_search_with_host_data(CloSearch* s, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* haystack, size_t numel_h, const void* needles, size_t numel_n,
	unsigned flags, void* pos_out, GError** err);

CCLContext* clo_search_get_context(CloSearch* s);
CloType clo_search_get_key_type(CloSearch* s);
size_t clo_search_get_key_size(CloSearch* s);

#ifdef __cplusplus
}
#endif
#endif
