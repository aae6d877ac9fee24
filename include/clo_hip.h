/*
 * clo_hip.h — the thin C-ABI layer over HIP that replaces the cf4ocl2/OpenCL
 * dispatch of cl_ops for the sort/scan hot path.
 *
 * Plain C, plain pointers and sizes; no C++/torch/HIP types in any signature
 * (streams and events travel as void*). The host drivers in
 * cl_ops_amd/csrc (clo_sort_*.c, clo_scan_*.c; plain C, built with gcc) call ONLY this header; the
 * implementations live in the .hip files of cl_ops_amd/csrc/hip (built with hipcc for
 * gfx950). Everything returns 0 on success or a non-zero status that
 * clo_hip_error_string() decodes (positive = hipError_t, negative = CLO_HIP_E*).
 *
 * What each entry point stands in for upstream is cited as file:line relative
 * to the reference tree's src/cl_ops/.
 */
#ifndef CLO_HIP_H
#define CLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLO_HIP_EARGS      (-1)  /* invalid argument combination */
#define CLO_HIP_EUNSUPPORTED (-2)  /* type/option not built into this library */
#define CLO_HIP_EWORKSPACE (-3)  /* workspace too small */
#define CLO_HIP_ETIMEOUT   (-4)  /* an in-kernel bounded spin gave up (see clo_hip_check_status) */
#define CLO_HIP_ENOTREADY  (-5)  /* clo_hip_stream_query: work enqueued on the stream is still running */
#define CLO_HIP_ERCCL      (-100) /* RCCL failures: CLO_HIP_ERCCL - ncclResult_t */

/* Alignment. Data arrays (sources, destinations, keys, values, first digits) need only be aligned to their element
 * size: a view into a larger allocation (a torch slice such as t[3:]) is fine, and kernels pick their vector loads
 * from the pointers they are given. Scratch the kernels poll and count in is not: every `workspace` must start
 * CLO_HIP_WORKSPACE_ALIGN bytes aligned (what hipMalloc and torch's allocator return), and every device uint64 word
 * the kernels add to or hand over (carry_in_dev, carry_out_dev, total_dev, counts_dev) 8 bytes aligned. An entry
 * given a misaligned one returns CLO_HIP_EARGS before anything is enqueued. */
#define CLO_HIP_WORKSPACE_ALIGN 256

/* ---- device / runtime (replaces ccl_context_*, ccl_queue_*, ccl_buffer_*,
 *      ccl_event_*, ccl_prof_* as used at sort/clo_sort_abstract.c:335-395,
 *      scan/clo_scan_abstract.c:290-339, benchmarks/clo_sort_bench.c:148-208) ---- */

typedef struct {
	char name[128];
	int compute_units;
	int max_threads_per_block;  /* CL_DEVICE_MAX_WORK_GROUP_SIZE stand-in */
	int wavefront_size;
	size_t lds_bytes_per_block;
	size_t global_mem_bytes;
	char gcn_arch[64];
} clo_hip_device_props;

int clo_hip_device_count(int* count);
int clo_hip_set_device(int device);
int clo_hip_get_device(int* device);
int clo_hip_get_device_props(int device, clo_hip_device_props* props);

int clo_hip_stream_create(void** stream);
/* The same with the device's highest stream priority: for the transfer stream of the sharded sort, whose (few)
 * work-groups should be dispatched ahead of the sort kernels' that fill the device beside them. */
int clo_hip_stream_create_high_priority(void** stream);
int clo_hip_stream_destroy(void* stream);
int clo_hip_stream_synchronize(void* stream);
int clo_hip_stream_query(void* stream);   /* 0 = everything enqueued so far has completed; CLO_HIP_ENOTREADY = not yet; else an error */

int clo_hip_malloc(void** dptr, size_t bytes);
int clo_hip_free(void* dptr);
int clo_hip_memcpy_h2d_async(void* dst, const void* src, size_t bytes, void* stream);
int clo_hip_memcpy_d2h_async(void* dst, const void* src, size_t bytes, void* stream);
int clo_hip_memcpy_d2d_async(void* dst, const void* src, size_t bytes, void* stream);
int clo_hip_memset_async(void* dst, int value, size_t bytes, void* stream);
/* Pin / unpin a caller's host range so that copies to and from it are true
 * asynchronous DMA (the *_with_host_data pipelines, sort/clo_sort_abstract.c:348-395,
 * scan/clo_scan_abstract.c:290-339). Failure is not fatal: pageable copies still work. */
int clo_hip_host_register(void* host_ptr, size_t bytes);
int clo_hip_host_unregister(void* host_ptr);

/* Re-reads the library's environment switches (CLO_MAX_SPINS, CLO_RADIX_SWEEP, CLO_R1_POOLS, CLO_RADIX_NO_DIGITS;
 * INTEGRATION.md lists them all). The C API calls it whenever a sorter / scanner is made; calls in between use what
 * was read then — nothing is read per call. */
void clo_hip_env_refresh(void);
int clo_hip_event_create(void** event);
int clo_hip_event_destroy(void* event);
int clo_hip_event_record(void* event, void* stream);
int clo_hip_event_synchronize(void* event);
int clo_hip_event_query(void* event);   /* 0 = the event has completed; anything else: not yet (or an error) */
int clo_hip_event_elapsed_ms(void* start, void* stop, float* ms);
/* Make `stream` wait for `event` (cq_exec waiting on a cq_comm copy,
 * sort/clo_sort_sbitonic.c:86-95). */
int clo_hip_stream_wait_event(void* stream, void* event);

/* Stream capture into an executable graph: a launch-bound sequence (sbitonic
 * makes one launch per (stage, step): 136 for 2^16 elements) is recorded once
 * and replayed with one call. begin/end bracket the launches on `stream`;
 * end instantiates the graph. */
int clo_hip_stream_is_capturing(void* stream);   /* 1: a capture is active (or the state is unknown), 0: none */
int clo_hip_graph_capture_begin(void* stream);
int clo_hip_graph_capture_end(void* stream, void** graph_exec);
int clo_hip_graph_launch(void* graph_exec, void* stream);
int clo_hip_graph_destroy(void* graph_exec);

const char* clo_hip_error_string(int status);

/* ---- exclusive prefix sum (replaces the three launches of
 *      scan/clo_scan_blelloch.c:146-195: workgroupScan, workgroupSumsScan,
 *      addWorkgroupSums — scan/clo_scan_blelloch.cl:49-211) ----
 * data_out[i] = sum_{j<i} (sum_t) data_in[j], wrap-around in the sum type.
 * elem_size, sum_size in {1,2,4,8} bytes with sum_size >= elem_size (unsigned
 * widening; signed inputs: pass elem_signed=1 for sign extension).
 * workspace: clo_hip_scan_workspace_bytes() bytes of device memory that
 * clo_hip_scan_workspace_init() has zeroed ONCE (after allocating it, and again
 * after a call that ended in CLO_HIP_ETIMEOUT); from then on the scans keep it
 * consistent themselves — look-back entries carry the epoch of the call that
 * wrote them, counters are put back by the last work-group to leave — so a
 * call clears nothing. One scan at a time per workspace. Asynchronous on
 * `stream`. */
size_t clo_hip_scan_workspace_bytes(size_t numel, int elem_size, int sum_size);
int clo_hip_scan_workspace_init(void* workspace, size_t workspace_bytes, void* stream);
/* RULE: every scan on a workspace passes the SAME workspace_bytes the range was
 * initialised with (where the scan keeps its accumulators follows from that
 * size; a workspace sized for the largest array serves every smaller one under
 * its full byte count). The library remembers what clo_hip_scan_workspace_init
 * prepared (pointer and byte count, host side) and answers CLO_HIP_EWORKSPACE
 * to a scan on a range it did not prepare or under another byte count — round 1's
 * "contents don't care, pass clo_hip_scan_workspace_bytes(n) per call" would
 * otherwise return wrong sums silently. clo_hip_scan_workspace_forget: the
 * caller is about to free the range (optional; initialising a range that
 * overlaps a remembered one replaces it). */
int clo_hip_scan_workspace_forget(void* workspace);
/* Test hook: sets the epoch the next scan on this workspace continues from
 * (epochs run 1 .. 2^30-1, then the workspace is zeroed in-kernel and they start
 * over); lets a test cross the wrap without 2^30 calls. */
int clo_hip_scan_workspace_set_epoch(void* workspace, unsigned epoch, void* stream);
int clo_hip_scan_exclusive(const void* data_in, void* data_out, size_t numel,
	int elem_size, int elem_signed, int sum_size,
	void* workspace, size_t workspace_bytes, void* stream);
/* The same scan as one chunk of a longer array (new: the chunked host-data
 * pipeline of clo_scan_with_host_data and the sharded multi-GPU scan):
 * *carry_in_dev (device uint64, low sum_size bytes used; NULL = 0) is added to
 * every output, *carry_out_dev (NULL = not wanted) receives carry_in + the sum
 * of the chunk, i.e. the next chunk's carry_in. */
int clo_hip_scan_exclusive_carry(const void* data_in, void* data_out, size_t numel,
	int elem_size, int elem_signed, int sum_size,
	const uint64_t* carry_in_dev, uint64_t* carry_out_dev,
	void* workspace, size_t workspace_bytes, void* stream);
/* The same scan with a FLOATING-POINT sum type (float: sum_size 4, double: 8);
 * elem_type is a CloType number (any of the eleven), elements are converted to the
 * sum type on load as upstream's kernels do (scan/clo_scan_blelloch.cl:79-80).
 * Reduce / scan the tile sums / apply, every addition in an order fixed by the
 * layout alone: deterministic, equal to upstream's result to rounding (its order
 * is the Blelloch tree of its own work-group size). No look-back, no polling.
 * The order is part of the contract (tests/fscan_model.py restates it in numpy and
 * the GPU tests hold every result to it bit for bit): each element is converted by
 * the C cast `(sum type) x` (round to nearest even, beyond the range an infinity);
 * a tile is 256 threads x 16 consecutive elements, slots past numel count as +0; a
 * thread adds its 16 left to right from +0; a wave's 64 thread sums are scanned by
 * the shuffle tree (off = 1, 2, .. 32: lanes >= off add the value off lanes below);
 * the four wave sums are added left to right, which gives each wave's base and the
 * tile's total; a thread starts from (base + inclusive value of the lane below) +
 * the tile's offset, never from `inclusive - own`, and emits the running value, then
 * adds the element; the tile totals are scanned by the same procedure one level up
 * (one tile / up to 4096 tiles / three levels). Every addition is an IEEE addition
 * in the sum type: subnormals (half, float and double) are kept, -0 elements sum to
 * +0, out[0] is +0, a NaN or inf - inf poisons exactly what lies behind it. */
/* Every other pair of CloTypes upstream's generic kernel accepts (scan/clo_scan_abstract.c:122-125 pastes any two
 * type names): a half sum type, floating-point elements summed in an integer type (each element truncated by the
 * cast `(sum type) x`, as upstream's kernel does), integer sums narrower than the elements (the cast keeps the low
 * bits). The same deterministic reduce / scan / apply kernels, arithmetic in the sum type. clo_hip_scan_is_typed
 * says which pairs go here (1) and which to clo_hip_scan_exclusive (0). elem_type / sum_type: CloType numbers. */
int clo_hip_scan_is_typed(int elem_type, int sum_type);
size_t clo_hip_scan_typed_workspace_bytes(size_t numel, int sum_type);
int clo_hip_scan_exclusive_typed(const void* data_in, void* data_out, size_t numel, int elem_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream);
size_t clo_hip_scan_fp_workspace_bytes(size_t numel, int sum_size);
int clo_hip_scan_exclusive_fp(const void* data_in, void* data_out, size_t numel, int elem_type, int sum_size,
	void* workspace, size_t workspace_bytes, void* stream);
/* Sum of the elements mod 2^64 into *total_dev (device): what a shard hands
 * to the later shards of a multi-GPU scan. */
int clo_hip_reduce_sum(const void* data_in, size_t numel, int elem_size, int elem_signed,
	uint64_t* total_dev, void* stream);   /* total_dev: 8-byte aligned */

/* ---- reduce by key (new functionality: CloReduceByKey, include/clo_reduce.h) ----
 * A run is a maximal stretch of consecutive elements whose keys (key_size 1, 2, 4 or 8 bytes) have the same bytes;
 * with m runs, run r = [b_r, e_r): keys_out[r] = keys_in[b_r], aggr_out[r] = op over the run of (sum type) value,
 * *num_runs_dev = m (device uint64, 8-byte aligned, required). Rows at index >= m are not written. op: 0 sum
 * (wrap-around in the sum type), 1 min, 2 max (compared in the sum type). value_type / sum_type: CloType numbers, int,
 * uint, long or ulong, the sum at least as wide as the value (anything else: CLO_HIP_EUNSUPPORTED). values_in NULL:
 * every value is 1 (run lengths; sum only, value_type ignored). keys_out or aggr_out may be NULL (not written; without
 * aggr_out neither values nor types are looked at), not both. No output range may overlap an input range. numel below
 * 2^32; numel 0 sets *num_runs_dev and launches nothing. Three launches (tile sweep, scan of the tile states by one
 * work-group, apply sweep), none of which waits for another work-group; asynchronous on `stream`.
 * clo_hip_reduce_by_key_tile: the elements per tile for keys of key_size and values of value_size (0: none) bytes. */
size_t clo_hip_reduce_by_key_tile(int key_size, int value_size);
size_t clo_hip_reduce_by_key_workspace_bytes(size_t numel);
int clo_hip_reduce_by_key(const void* keys_in, const void* values_in, void* keys_out, void* aggr_out, uint64_t* num_runs_dev,
	size_t numel, int key_size, int value_type, int sum_type, int op,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- scan by key (new functionality: CloScanByKey, include/clo_scan_by_key.h) ----
 * Runs, op, value_type / sum_type and values_in NULL as for reduce by key above. With b(i) the first element of i's
 * run: inclusive 1: out[i] = op over [b(i), i] of (sum type) value; inclusive 0: over [b(i), i), the identity at
 * i = b(i) (0 for sum, the sum type's largest number for min, its smallest for max). Anything but 0 or 1 for
 * `inclusive`, an op out of range, min / max without values, numel >= 2^32, a missing keys_in / out / workspace, a
 * misaligned workspace or an `out` not aligned to its element: CLO_HIP_EARGS before anything is enqueued; types not built: CLO_HIP_EUNSUPPORTED; a workspace
 * below clo_hip_scan_by_key_workspace_bytes(numel): CLO_HIP_EWORKSPACE. `out` may be exactly values_in when the sum
 * type is as wide as the value type; no other overlap of out with an input is allowed (not checked here: the driver
 * does). numel 0 launches nothing. Three launches (tile sweep, scan of the tile states by one work-group, apply
 * sweep), none of which waits for another work-group; asynchronous on `stream`.
 * clo_hip_scan_by_key_tile: the elements per tile for keys of key_size and values of value_size (0: none) bytes, 0
 * for sizes not built. clo_hip_scan_by_key_workspace_bytes is monotone in numel. */
size_t clo_hip_scan_by_key_tile(int key_size, int value_size);
size_t clo_hip_scan_by_key_workspace_bytes(size_t numel);
int clo_hip_scan_by_key(const void* keys_in, const void* values_in, void* out, size_t numel,
	int key_size, int value_type, int sum_type, int op, int inclusive,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- histogram (new functionality: CloHistogram, include/clo_histogram.h) ----
 * Keys are integers of key_size (1, 2, 4, 8) bytes, two's complement when key_signed is not 0; `lower` holds the
 * lower bound's bits in its low key_size bytes. With d = key - lower over the integers, an element is counted iff
 * d >= 0 and (d >> shift) < num_bins, in bin d >> shift; hist_out[b] = sum over bin b's elements of (sum type) value,
 * modulo 2^bits of the sum type. value_type / sum_type: CloType numbers, int, uint, long or ulong, the sum at least
 * as wide as the value (anything else, and key sizes not built: CLO_HIP_EUNSUPPORTED). values_in NULL: every value is
 * 1 (value_type ignored). accumulate 0: all num_bins entries are written (zeroed by a fill on `stream` first);
 * otherwise the sums are added onto what hist_out holds. numel 0 launches no kernel. CLO_HIP_EARGS before anything
 * is enqueued: hist_out NULL or not aligned to the sum type, num_bins 0 or >= 2^32, numel >= 2^32, shift >= 8 *
 * key_size, keys_in NULL with numel > 0, keys or values not aligned to their element. hist_out must not overlap an
 * input (not checked here: the driver does). max_groups: 0, or an upper bound on the work-groups launched (tests walk
 * the grid-stride loop with 1, 2, 3). One launch of a fixed grid; no work-group waits for another; asynchronous on
 * `stream`. The workspace may be NULL when clo_hip_histogram_workspace_bytes says 0 (it does today: every counter
 * lives in LDS or in hist_out).
 * clo_hip_histogram_tile: the elements per tile for keys of key_size and values of value_size (0: none) bytes, 0 for
 * sizes not built. clo_hip_histogram_lds_bins: the largest num_bins whose counters a work-group keeps in LDS for sums
 * of sum_size (4, 8) bytes, 0 for other sizes; above it the adds go straight to hist_out. */
size_t clo_hip_histogram_tile(int key_size, int value_size);
size_t clo_hip_histogram_lds_bins(int sum_size);
size_t clo_hip_histogram_workspace_bytes(size_t numel, size_t num_bins);
int clo_hip_histogram(const void* keys_in, const void* values_in, void* hist_out, size_t numel, int key_size, int key_signed,
	int value_type, int sum_type, uint64_t lower, unsigned shift, size_t num_bins, int accumulate, unsigned max_groups,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- merge (new functionality: CloMerge, include/clo_merge.h) ----
 * The stable merge of keys_a[0, numel_a) and keys_b[0, numel_b), each ascending, into keys_out[0, n), n = numel_a +
 * numel_b: ties go to A, the order inside A and inside B is kept. Keys are key_size (1, 2, 4, 8) bytes and compare
 * by key_kind: 0 unsigned, 1 signed (two's complement), 2 IEEE total order (2, 4, 8 bytes). value_size 0: keys only.
 * value_size 4 or 8: values_out[j] is the value of the element at keys_out[j]; with value_size 4 and the values of
 * every non-empty input NULL it is that element's index in A || B instead (argmerge: i for A[i], numel_a + i for
 * B[i]). keys_out may be NULL when values_out is given. The values pointer of an empty input is not looked at.
 * CLO_HIP_EARGS before anything is enqueued: key_kind out of range, n >= 2^32, NULL keys of a non-empty input, both
 * outputs NULL, values (in or out) with value_size 0, values_out NULL with value_size > 0, values given for one
 * non-empty input and NULL for the other, NULL values with value_size 8, a pointer not aligned to its element, a
 * missing or misaligned workspace. Sizes not built: CLO_HIP_EUNSUPPORTED. A workspace below
 * clo_hip_merge_workspace_bytes(numel_a, numel_b): CLO_HIP_EWORKSPACE. No output may overlap an input or the other
 * output (not checked here: the driver does). n 0 launches nothing and needs no workspace. On inputs that are not
 * sorted the outputs' contents are unspecified; reads stay inside the inputs and writes inside [0, n) of the outputs.
 * Two launches (the tiles' split points into the workspace, then one work-group per tile of the output); no work-group
 * waits for another; asynchronous on `stream`; nothing is allocated and the host never waits, so the call can be
 * captured into a graph.
 * clo_hip_merge_tile: the output elements per tile for keys of key_size and values of value_size (0: none) bytes, 0
 * for sizes not built. clo_hip_merge_workspace_bytes is monotone in numel_a + numel_b and 0 for n = 0. */
size_t clo_hip_merge_tile(int key_size, int value_size);
size_t clo_hip_merge_workspace_bytes(size_t numel_a, size_t numel_b);
int clo_hip_merge(const void* keys_a, const void* values_a, size_t numel_a,
	const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, int key_size, int key_kind,
	int value_size, void* workspace, size_t workspace_bytes, void* stream);

/* ---- search (new functionality: CloSearch, include/clo_search.h) ----
 * pos_out[i], a uint, = how many of haystack[0, numel_h), ascending, are < needles[i] (flags & CLO_HIP_SEARCH_UPPER:
 * <= needles[i]), for i in [0, numel_n). Keys are key_size (1, 2, 4, 8) bytes and compare by key_kind as in
 * clo_hip_merge. CLO_HIP_SEARCH_NEEDLES_SORTED: the caller promises that the needles are ascending too; the results
 * are then the same and each touched haystack key is read once (two launches: the tiles' ranges of the haystack into
 * the workspace, then one work-group per tile of needles). Without it: one launch of a grid-stride loop over the
 * tiles, at most max_groups work-groups when max_groups is not 0 (tests walk the loop with 1, 2, 3); max_groups bounds
 * the second launch of the sorted form too.
 * CLO_HIP_EARGS before anything is enqueued: key_kind out of range, other flag bits, numel_h or numel_n >= 2^32, NULL
 * haystack with numel_h > 0, NULL needles or pos_out with numel_n > 0, a pointer not aligned to its element, a
 * missing or misaligned workspace where clo_hip_search_workspace_bytes is not 0. Sizes not built:
 * CLO_HIP_EUNSUPPORTED. A workspace below that size: CLO_HIP_EWORKSPACE. pos_out must not overlap an input (not
 * checked here: the driver does). numel_n 0 launches nothing; numel_h 0 writes zeros and reads no haystack. On a
 * haystack that is not sorted, or needles that break the promise, the contents of pos_out are unspecified; reads stay
 * inside the inputs, writes inside pos_out[0, numel_n), every value written is <= numel_h. No work-group waits for
 * another; asynchronous on `stream`; nothing is allocated and the host never waits, so the call can be captured into
 * a graph.
 * clo_hip_search_tile: needles per tile; clo_hip_search_lds_keys: the longest haystack (general form) or range of it
 * (sorted form) a work-group keeps in LDS; clo_hip_search_pivots: the entries of the sampled table the general form
 * keeps in LDS for a longer haystack; each 0 for key sizes not built. clo_hip_search_workspace_bytes is monotone in
 * numel_n, 0 for numel_n = 0, for numel_h = 0 and without CLO_HIP_SEARCH_NEEDLES_SORTED. */
#define CLO_HIP_SEARCH_UPPER          1u
#define CLO_HIP_SEARCH_NEEDLES_SORTED 2u
size_t clo_hip_search_tile(int key_size);
size_t clo_hip_search_lds_keys(int key_size);
size_t clo_hip_search_pivots(int key_size);
size_t clo_hip_search_workspace_bytes(size_t numel_h, size_t numel_n, unsigned flags);
int clo_hip_search(const void* haystack, size_t numel_h, const void* needles, size_t numel_n, void* pos_out,
	int key_size, int key_kind, unsigned flags, unsigned max_groups,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- set operations (new functionality: CloSetOp, include/clo_setop.h) ----
 * The multiset union, intersection, difference (A - B) or symmetric difference of keys_a[0, numel_a) and keys_b[0,
 * numel_b), each ascending: the subsequence of clo_hip_merge's output that the op keeps (include/clo_setop.h has the
 * table), written to keys_out[0, k) and values_out[0, k); *num_out = k, a uint64_t of device memory, 8-byte aligned.
 * Nothing is written at index >= k. The outputs hold at least the op's capacity: numel_a + numel_b (union, symmetric
 * difference), min(numel_a, numel_b) (intersection), numel_a (difference). Keys, key_kind, value_size and the arg form
 * (value_size 4 and NULL values: the element's index in A || B) are clo_hip_merge's. Intersection and difference keep
 * no element of B: values_b is not looked at.
 * CLO_HIP_EARGS before anything is enqueued: clo_hip_merge's list, an op outside the four, num_out NULL or not 8-byte
 * aligned. CLO_HIP_EUNSUPPORTED and CLO_HIP_EWORKSPACE as clo_hip_merge. No output may overlap an input, the other
 * output or num_out (not checked here: the driver does). n 0 needs no workspace and still writes *num_out = 0. On
 * inputs that are not sorted k and the contents are unspecified; reads stay inside the inputs, writes inside [0,
 * capacity) of the outputs, k <= capacity.
 * Four launches (the tiles' split points, the tiles' kept counts, one work-group that turns the counts into offsets
 * and writes num_out, the compacting merge); no work-group waits for another and there are no atomics; asynchronous on
 * `stream`; nothing is allocated and the host never waits, so the call can be captured into a graph.
 * clo_hip_setop_tile: the merged elements per tile, 0 for sizes not built. clo_hip_setop_workspace_bytes is monotone
 * in numel_a + numel_b and 0 for n = 0. */
#define CLO_HIP_SETOP_UNION                0
#define CLO_HIP_SETOP_INTERSECTION         1
#define CLO_HIP_SETOP_DIFFERENCE           2
#define CLO_HIP_SETOP_SYMMETRIC_DIFFERENCE 3
size_t clo_hip_setop_tile(int key_size, int value_size);
size_t clo_hip_setop_workspace_bytes(size_t numel_a, size_t numel_b);
int clo_hip_setop(int op, const void* keys_a, const void* values_a, size_t numel_a,
	const void* keys_b, const void* values_b, size_t numel_b,
	void* keys_out, void* values_out, uint64_t* num_out, int key_size, int key_kind,
	int value_size, void* workspace, size_t workspace_bytes, void* stream);

/* ---- equi-join (new functionality: CloJoin, include/clo_join.h) ----
 * The inner, left, right or full outer join of keys_a[0, numel_a) and keys_b[0, numel_b), each ascending (keys and
 * key_kind as for clo_hip_merge), as rows (idx_a, idx_b, key) in ascending key order; a side without a partner holds
 * CLO_HIP_JOIN_NONE (include/clo_join.h has the rows and their order). *num_out = K, the rows of the whole join, a
 * uint64_t of device memory, 8-byte aligned: K may exceed both `capacity` and 2^32. Rows [0, min(K, capacity)) are
 * written to those of idx_a_out, idx_b_out and keys_out that are not NULL, each holding `capacity` (< 2^32) rows;
 * nothing is written at an index >= min(K, capacity). All three NULL and capacity 0: the count form, which writes
 * num_out alone. numel_a + numel_b < 2^32.
 *
 * Status: CLO_HIP_EARGS (a kind outside 0..3, key_kind outside 0..2, NULL keys of a non-empty input, num_out NULL or
 * misaligned, capacity > 0 with all outputs NULL, a pointer not aligned to its element, numel_a + numel_b or capacity
 * >= 2^32, the workspace NULL or not CLO_HIP_WORKSPACE_ALIGN-aligned while numel_a + numel_b > 0), CLO_HIP_EUNSUPPORTED
 * (a key_size other than 1, 2, 4, 8; key_kind 2 with key_size 1), CLO_HIP_EWORKSPACE.
 * Five launches, three in the count form (the merged tiles' split points; every merged element's rows and the tiles'
 * totals; one work-group that turns the totals into offsets and writes num_out; the output tiles' first emitters; the
 * write, one work-group per clo_hip_join_out_tile() rows of the RESULT); no work-group waits for another and there are
 * no global atomics; asynchronous on `stream`; nothing is allocated and the host never waits, so the call can be
 * captured into a graph. clo_hip_join_tile: the merged elements per tile, 0 for sizes not built.
 * clo_hip_join_workspace_bytes is monotone in numel_a and numel_b, 0 for n = 0 or an unknown kind. */
#define CLO_HIP_JOIN_INNER 0
#define CLO_HIP_JOIN_LEFT  1
#define CLO_HIP_JOIN_RIGHT 2
#define CLO_HIP_JOIN_FULL  3
#define CLO_HIP_JOIN_NONE  0xFFFFFFFFu
size_t clo_hip_join_tile(int key_size);
size_t clo_hip_join_out_tile(void);
size_t clo_hip_join_workspace_bytes(int kind, size_t numel_a, size_t numel_b);
int clo_hip_join(int kind, const void* keys_a, size_t numel_a, const void* keys_b, size_t numel_b,
	uint32_t* idx_a_out, uint32_t* idx_b_out, void* keys_out, size_t capacity,
	uint64_t* num_out, int key_size, int key_kind,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- selection and partition (new functionality: CloSelect, include/clo_select.h) ----
 * Element i of keys_in[0, numel) is KEPT iff flags[i] != 0 (pred CLO_HIP_SELECT_FLAGGED: flags_or_threshold points to
 * numel bytes, the keys are opaque) or iff keys_in[i] <pred> threshold in clo_hip_merge's order of key_kind (0 unsigned,
 * 1 signed, 2 IEEE total order; flags_or_threshold points to ONE key in device memory, aligned to key_size). The order
 * is total: EQ means equal bits. op CLO_HIP_SELECT_SELECT: the k kept elements go to rows [0, k) of keys_out and
 * values_out in input order, rows >= k are not written. CLO_HIP_SELECT_PARTITION: the rejected elements go to rows [k,
 * numel) behind them, in input order too. *num_out = k, a uint64_t of device memory, 8-byte aligned. The outputs hold
 * numel rows. value_size 0 (none), 4 or 8: opaque words; value_size 4 with values_in NULL: values_out[j] is the
 * element's index (the arg form); keys_out may then be NULL, and with FLAGGED keys_in too.
 * CLO_HIP_EARGS before anything is enqueued: an op, pred or key_kind out of range, numel >= 2^32, flags_or_threshold
 * NULL (but the flags of numel 0), num_out NULL or not 8-byte aligned, both outputs NULL, values (in or out) with value_size 0, values_out NULL
 * with value_size > 0, NULL values_in with value_size 8, keys_in NULL with numel > 0 where the keys are read (a comparison, or
 * keys_out given), a pointer not aligned to its element, a missing or misaligned workspace with numel > 0. Sizes not
 * built: CLO_HIP_EUNSUPPORTED. A workspace below clo_hip_select_workspace_bytes(numel, key_size, value_size):
 * CLO_HIP_EWORKSPACE. No output may overlap an input, the flags, the threshold, the other output or num_out (not
 * checked here: the driver does). numel 0 needs no workspace and still writes *num_out = 0.
 * Whatever the arrays hold, reads stay inside the inputs, writes inside [0, numel) of the outputs, and k <= numel.
 * Three launches (the tiles' kept counts; one work-group that turns them into offsets and writes num_out, taking
 * CLO_HIP_SELECT_SCAN_TRIP counts per trip of its loop; the compacting sweep); no work-group waits for another and there
 * are no atomics; asynchronous on `stream`; nothing is allocated and the host never waits, so the call can be captured
 * into a graph. clo_hip_select_tile: the elements per tile, 0 for sizes not built. clo_hip_select_workspace_bytes is
 * monotone in numel, 0 for numel 0 and a multiple of CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_SELECT_SELECT    0
#define CLO_HIP_SELECT_PARTITION 1
#define CLO_HIP_SELECT_FLAGGED 0
#define CLO_HIP_SELECT_LT      1
#define CLO_HIP_SELECT_LE      2
#define CLO_HIP_SELECT_GT      3
#define CLO_HIP_SELECT_GE      4
#define CLO_HIP_SELECT_EQ      5
#define CLO_HIP_SELECT_NE      6
#define CLO_HIP_SELECT_SCAN_TRIP 2048
size_t clo_hip_select_tile(int key_size, int value_size);
size_t clo_hip_select_workspace_bytes(size_t numel, int key_size, int value_size);
int clo_hip_select(int op, int pred, const void* keys_in, const void* values_in, const void* flags_or_threshold,
	void* keys_out, void* values_out, uint64_t* num_out, size_t numel, int key_size, int key_kind,
	int value_size, void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-way partition by bin (new functionality: CloBucket, include/clo_bucket.h) ----
 * The bin of keys_in[i] is clo_hip_histogram's: with d = key - lower over the integers (lower: the low key_size bytes,
 * key_signed: two's complement), the row is IN RANGE iff d >= 0 and (d >> shift) < num_bins, and its bin is d >> shift;
 * every other row belongs to the rest, which counts as bin num_bins. The numel rows go to keys_out / values_out in
 * ascending (bin, input index) order — a stable sort by bin, the rest last — and offsets_out receives num_bins + 1
 * entries of count_size (4 or 8) bytes: offsets_out[b] = the rows in the bins below b, offsets_out[num_bins] = the rows
 * in range. Values: value_size 0 (none), 4 or 8 opaque bytes; value_size 4 with values_in NULL writes the input row
 * indices (uint32) and keys_out may then be NULL. numel 0 writes num_bins + 1 zeros and needs no workspace.
 * CLO_HIP_EARGS: offsets_out NULL or misaligned, num_bins 0 or above CLO_HIP_BUCKET_MAX_BINS, numel >= 2^32, shift >= 8
 * key_size, values passed with value_size 0, values_out NULL with value_size > 0, values_in NULL with value_size 8,
 * keys_out NULL outside the index form, keys_in NULL with numel > 0, a misaligned array, a workspace that is NULL or not
 * CLO_HIP_WORKSPACE_ALIGN aligned (numel > 0). Key sizes other than 1, 2, 4, 8, value sizes other than 0, 4, 8 and count
 * sizes other than 4, 8: CLO_HIP_EUNSUPPORTED. A workspace below clo_hip_bucket_workspace_bytes(numel, key_size,
 * value_size, num_bins): CLO_HIP_EWORKSPACE, nothing is launched. Nothing overlaps (the caller checks).
 * Asynchronous on `stream`: one pass of five launches where num_bins + 1 <= 256 (count, the three launches of the
 * counter scan, scatter), two such passes through the workspace plus clo_hip_histogram and a one-group scan above; no
 * work-group waits for another, no host wait, so the calls record into a graph. Timing labels: "bucket_count",
 * "bucket_scan", "bucket_scatter", "bucket_offsets". The counter scan gives CLO_HIP_BUCKET_SCAN_GROUP counters (digits of
 * the pass x tiles) to a work-group and scans the groups' sums CLO_HIP_BUCKET_SCAN_TRIP per trip of its loop.
 * clo_hip_bucket_tile: the rows per tile, 0 for sizes not built. clo_hip_bucket_workspace_bytes is monotone in numel and
 * num_bins, 0 for numel 0 and a multiple of CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_BUCKET_MAX_BINS 65535
#define CLO_HIP_BUCKET_SCAN_GROUP 4096
#define CLO_HIP_BUCKET_SCAN_TRIP 2048
size_t clo_hip_bucket_tile(int key_size, int value_size);
size_t clo_hip_bucket_workspace_bytes(size_t numel, int key_size, int value_size, size_t num_bins);
int clo_hip_bucket(const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* offsets_out, size_t numel,
	int key_size, int key_signed, int value_size, int count_size, uint64_t lower, unsigned shift, size_t num_bins,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- top-k (new functionality: CloTopK, include/clo_topk.h) ----
 * With m = min(k, numel): the first m elements of the stable ascending sort of keys_in[0, numel) (which
 * CLO_HIP_TOPK_SMALLEST) or of the stable sort by the complemented order key (CLO_HIP_TOPK_LARGEST: the largest key
 * first), in clo_hip_merge's order of key_kind (0 unsigned, 1 signed, 2 IEEE total order); the lower index comes first
 * among equal keys, so where the m-th key has ties the tied elements with the lowest indices are taken. They go to rows
 * [0, m) of keys_out and values_out in increasing input index (order CLO_HIP_TOPK_INPUT) or in the order of that sort
 * (CLO_HIP_TOPK_SORTED, for m <= clo_hip_topk_sorted_max only); rows >= m are not written, the outputs need hold m rows
 * only. kth_out (may be NULL; device memory, one key, aligned to key_size) receives the key of the m-th chosen element
 * of that sort, with its original bits; with both outputs NULL it is all that is computed. value_size 0 (none), 4 or 8:
 * opaque words; value_size 4 with values_in NULL: values_out[j] is the element's index (the arg form), keys_out may
 * then be NULL. numel 0 or k 0: success, nothing is enqueued, no workspace is needed.
 * CLO_HIP_EARGS before anything is enqueued: which, order or key_kind out of range, numel >= 2^32, keys_out, values_out
 * and kth_out all NULL, values (in or out) with value_size 0, values_out NULL with value_size > 0, NULL values_in with
 * value_size 8, keys_in NULL with numel > 0, a pointer not aligned to its element, SORTED with m above
 * clo_hip_topk_sorted_max, a missing or misaligned workspace with m > 0. Sizes not built: CLO_HIP_EUNSUPPORTED. A
 * workspace below clo_hip_topk_workspace_bytes(numel, key_size, value_size): CLO_HIP_EWORKSPACE. No output may overlap
 * an input, another output or kth_out (not checked here: the driver does).
 * Whatever the arrays hold, reads stay inside the inputs and writes inside rows [0, m) and kth_out.
 * key_size digit sweeps of 8 bits, most significant first, each followed by one work-group that picks the digit holding
 * the remaining rank; then the tiles' counts of keys before and equal to the m-th, one launch that turns both into
 * offsets (CLO_HIP_TOPK_SCAN_TRIP tiles per trip of its loop), the compacting sweep and, for SORTED, one work-group that
 * sorts the m rows in LDS. Every sweep reads all numel keys: the time does not depend on the data. No work-group waits
 * for another; global atomic adds go to the 256-word digit tables in the workspace alone (cleared by a fill on
 * `stream`); asynchronous on `stream`; nothing is allocated and the host never waits or reads anything back, so the call
 * can be captured into a linear graph and replayed after the keys were rewritten. k is a host argument: it is baked into
 * the captured launches.
 * clo_hip_topk_tile: the elements per tile of the count and apply sweeps, 0 for sizes not built.
 * clo_hip_topk_sweep_groups: the work-groups a digit sweep launches on the current device where the number of its tiles
 * (of clo_hip_topk_tile(key_size, 0) keys) does not limit it; above that many tiles a group takes several, grid-stride.
 * clo_hip_topk_sorted_max: the largest m SORTED takes (at least 1024), 0 for sizes not built.
 * clo_hip_topk_workspace_bytes is monotone in numel, 0 for numel 0 and a multiple of CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_TOPK_SMALLEST 0
#define CLO_HIP_TOPK_LARGEST  1
#define CLO_HIP_TOPK_INPUT  0
#define CLO_HIP_TOPK_SORTED 1
#define CLO_HIP_TOPK_SCAN_TRIP 2048
size_t clo_hip_topk_tile(int key_size, int value_size);
size_t clo_hip_topk_sweep_groups(void);
size_t clo_hip_topk_sorted_max(int key_size, int value_size);
size_t clo_hip_topk_workspace_bytes(size_t numel, int key_size, int value_size);
int clo_hip_topk(int which, int order, const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* kth_out,
	size_t numel, size_t k, int key_size, int key_kind, int value_size, void* workspace, size_t workspace_bytes, void* stream);

/* ---- run-length decode and segment ids (new functionality: CloExpand, include/clo_expand.h) ----
 * With m = min(numel_in, *num_in) (num_in: a uint64_t of device memory, 8-byte aligned, or NULL: m = numel_in) and the
 * inclusive ends e_r of the m segments — form CLO_HIP_EXPAND_COUNTS: the running sums, in 64 bits, of the numel_in
 * counts at counts_or_offsets, those at r >= m adding 0; CLO_HIP_EXPAND_OFFSETS: offsets[r + 1] - offsets[0] of numel_in
 * + 1 ascending offsets — and total = e_(m-1) (0 for m 0): for every row j < min(total, capacity), with r(j) = the
 * number of r < m with e_r <= j, values_out[j] = values_in[r(j)] (opaque words of value_size 1, 2, 4 or 8 bytes),
 * seg_out[j] = r(j) and rank_out[j] = j - e_(r(j)-1), both uint32. Each output may be NULL, not all three; values_in
 * and values_out come together (value_size is not looked at without them). Rows >= min(total, capacity) are not
 * written. *num_out = total, unclamped (a uint64_t of device memory, 8-byte aligned). count_size 4 or 8: uint32 or
 * uint64 counts or offsets.
 * CLO_HIP_EARGS before anything is enqueued: a form out of range, numel_in or capacity >= 2^32, counts_or_offsets NULL
 * with numel_in > 0 (offsets: with capacity > 0 too), num_out NULL or misaligned, num_in misaligned, all outputs NULL,
 * one of values_in / values_out without the other, values with value_size 0, a pointer not aligned to its element, a
 * missing or misaligned workspace with numel_in > 0. Sizes not built: CLO_HIP_EUNSUPPORTED. A workspace below
 * clo_hip_expand_workspace_bytes(numel_in, capacity): CLO_HIP_EWORKSPACE. No output may overlap an input, num_in or
 * another output (not checked here: the driver does). numel_in 0 needs no workspace and still writes *num_out = 0.
 * Whatever the arrays hold, reads stay inside the inputs, every index gathered by and every seg_out value is below
 * numel_in, writes stay inside [0, capacity) of the outputs and num_out, and the call completes.
 * Launches: for the counts form three that write the ends into the workspace (tile sums, one work-group that scans
 * them, the tiles' write); one thread per tile boundary that finds the tile's first segment by a bounded halving and
 * writes num_out; one work-group per tile of clo_hip_expand_tile rows, which marks the segment starts in LDS when the
 * tile has at most clo_hip_expand_lds_segments of them and halves per row in global memory otherwise. No work-group
 * waits for another and there are no global atomics; asynchronous on `stream`; nothing is allocated and the host never
 * waits, so the call can be captured into a graph. clo_hip_expand_tile: 0 for value sizes not built (0, none, is
 * built). clo_hip_expand_workspace_bytes is monotone in both arguments, 0 for (0, 0) and a multiple of
 * CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_EXPAND_COUNTS 0
#define CLO_HIP_EXPAND_OFFSETS 1
size_t clo_hip_expand_tile(int value_size);
size_t clo_hip_expand_lds_segments(void);
size_t clo_hip_expand_workspace_bytes(size_t numel_in, size_t capacity);
int clo_hip_expand(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* values_out, void* seg_out, void* rank_out, uint64_t* num_out, size_t numel_in, size_t capacity, int value_size,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- sum, min and max per segment (new functionality: CloSegReduce, include/clo_segreduce.h) ----
 * m = min(numel_seg, *num_in), the forms (CLO_HIP_SEGREDUCE_COUNTS, CLO_HIP_SEGREDUCE_OFFSETS), the inclusive ends e_r,
 * count_size and num_out = e_(m-1) unclamped are clo_hip_expand's above. With n = numel rows of values_in and e_(-1) = 0,
 * for every r < m: aggr_out[r] = op over i in [min(e_(r-1), n), min(e_r, n)) of (sum type) values_in[i], and the
 * identity where that range is empty (0 for sum, the sum type's largest number for min, its smallest for max). op, the
 * cast, value_type and sum_type (CloType numbers: int, uint, long or ulong, the sum at least as wide as the value) are
 * clo_hip_reduce_by_key's. Rows r >= m of aggr_out are not written.
 * CLO_HIP_EARGS before anything is enqueued: an op or form out of range, numel_seg or numel >= 2^32, counts_or_offsets
 * NULL with numel_seg > 0 (offsets: always), values_in NULL with numel > 0, aggr_out NULL with numel_seg > 0, num_out
 * NULL or misaligned, num_in misaligned, a pointer not aligned to its element, a missing or misaligned workspace with
 * numel_seg > 0. Types and count sizes not built: CLO_HIP_EUNSUPPORTED. A workspace below
 * clo_hip_segreduce_workspace_bytes(numel_seg, numel): CLO_HIP_EWORKSPACE. Neither output may overlap an input, num_in
 * or the other output (not checked here: the driver does). numel_seg 0 needs no workspace and writes *num_out = 0 alone.
 * Whatever the arrays hold, reads stay inside the inputs, writes inside aggr_out[0, numel_seg) and num_out, and the
 * call completes.
 * Launches: for the counts form the three of clo_hip_expand that write the ends into the workspace; one thread per tile
 * boundary of the MERGE of the m clipped ends with the n row indices, which finds its split by a halving and writes
 * num_out; one work-group per tile of clo_hip_segreduce_tile merge steps (a step closes a segment or takes a row, so
 * that a tile's work does not depend on how many segments are empty), which writes every segment that closes in it and
 * leaves the tile's open aggregate in the workspace; one work-group that scans the tiles' open aggregates; one thread
 * per tile that adds the carry to the tile's first closing segment. values_in is read once. No work-group waits for
 * another and there are no global atomics; asynchronous on `stream`; nothing is allocated and the host never waits, so
 * the call can be captured into a graph. clo_hip_segreduce_tile: 0 for sizes not built.
 * clo_hip_segreduce_workspace_bytes is monotone in both arguments, 0 for (0, 0) and a multiple of
 * CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_SEGREDUCE_COUNTS 0
#define CLO_HIP_SEGREDUCE_OFFSETS 1
size_t clo_hip_segreduce_tile(int value_size, int sum_size);
size_t clo_hip_segreduce_workspace_bytes(size_t numel_seg, size_t numel);
int clo_hip_segreduce(int op, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* aggr_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- a stable sort inside every segment (new functionality: CloSegSort, include/clo_segsort.h) ----
 * m = min(numel_seg, *num_in), the forms (CLO_HIP_SEGSORT_COUNTS, CLO_HIP_SEGSORT_OFFSETS), the inclusive ends e_r,
 * count_size and num_out = e_(m-1) unclamped are clo_hip_expand's above. With n = numel rows and e_(-1) = 0, for every
 * r < m the rows [min(e_(r-1), n), min(e_r, n)) of keys_out hold the same rows of keys_in ascending, equal keys in their
 * input order; key_type is a CloType number and gives the key's size and its order (unsigned by bits, signed
 * numerically, half / float / double in IEEE total order); the keys' bits are not changed. values_out[j] is the value
 * (an opaque word of value_size 4 or 8 bytes) of the row that moved to j; value_size 4 with values_in NULL is the ARG
 * form: values_out[j] is that row's global index as uint32, and keys_out may then be NULL. Rows >= min(total, n) of the
 * outputs are not written.
 * CLO_HIP_EARGS before anything is enqueued: a form out of range, numel_seg or numel >= 2^32, counts_or_offsets NULL
 * with numel_seg > 0 (offsets: always), keys_in NULL with numel > 0, values with value_size 0, values_out NULL with
 * value_size > 0, values_in NULL with value_size 8, keys_out NULL outside the arg form, num_out NULL or misaligned,
 * num_in misaligned, a pointer not aligned to its element, a missing or misaligned workspace with numel_seg > 0. Key
 * types, value and count sizes not built: CLO_HIP_EUNSUPPORTED. A workspace below
 * clo_hip_segsort_workspace_bytes(numel_seg, numel, key_size, value_size): CLO_HIP_EWORKSPACE. No output may overlap an
 * input, num_in or another output (not checked here: the driver does). numel_seg 0 needs no workspace and writes
 * *num_out = 0 alone. Whatever the arrays hold, reads stay inside the inputs, writes inside [0, numel) of the outputs
 * and num_out, and the call completes.
 * The WORKSPACE holds a second copy of the rows (numel keys and numel values; with value_size 4 a third array of numel
 * keys, which stands in for keys_out when the arg form passes none), a byte per row, rounded up to whole tiles, 32
 * bytes per tile, and for the counts form 8 bytes per segment: a segment that crosses a tile boundary ping-pongs
 * between the outputs and that copy.
 * Launches: for the counts form the three of clo_hip_expand that write the ends; a memset of the row bytes; one thread
 * per segment that marks the first row of every non-empty segment and writes num_out; one work-group per tile of
 * clo_hip_segsort_tile rows that sorts them on chip by (segment, key, row) and writes them, which finishes every segment
 * that lies inside one tile; ceil(log2(tiles)) merge passes, one work-group per output tile, each of which leaves at
 * once unless a segment of its tile has the middle of a pair of blocks of that pass inside it. No work-group waits for another and there are no global atomics; asynchronous on
 * `stream`; nothing is allocated and the host never waits, so the call can be captured into a graph.
 * clo_hip_segsort_tile: T, or 0 for sizes not built. clo_hip_segsort_workspace_bytes is monotone in the two counts, 0
 * for (0, 0, ., .) and a multiple of CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_SEGSORT_COUNTS 0
#define CLO_HIP_SEGSORT_OFFSETS 1
size_t clo_hip_segsort_tile(int key_size, int value_size);
size_t clo_hip_segsort_workspace_bytes(size_t numel_seg, size_t numel, int key_size, int value_size);
int clo_hip_segsort(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, uint64_t* num_out, size_t numel_seg, size_t numel, int key_type, int value_size,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- running sum, min and max within segments (new functionality: CloSegScan, include/clo_segscan.h) ----
 * m = min(numel_seg, *num_in), the forms (CLO_HIP_SEGSCAN_COUNTS, CLO_HIP_SEGSCAN_OFFSETS), the inclusive ends e_r,
 * count_size and num_out = e_(m-1) unclamped are clo_hip_expand's above. With n = numel rows of values_in, e_(-1) = 0,
 * ct = min(e_(m-1), n) and b(i) the first row of the clipped segment [min(e_(r-1), n), min(e_r, n)) that holds row i:
 * for every i < ct, data_out[i] = op over j in [b(i), i] of (sum type) values_in[j] when inclusive is 1, over [b(i), i)
 * when it is 0, the identity at i = b(i) (0 for sum, the sum type's largest number for min, its smallest for max). op,
 * the cast, value_type and sum_type (CloType numbers: int, uint, long or ulong, the sum at least as wide as the value)
 * are clo_hip_reduce_by_key's. Rows i >= ct of data_out are not written.
 * CLO_HIP_EARGS before anything is enqueued: an op, inclusive or form out of range, numel_seg or numel >= 2^32,
 * counts_or_offsets NULL with numel_seg > 0 (offsets: always), values_in or data_out NULL with numel > 0, num_out NULL or
 * misaligned, num_in misaligned, a pointer not aligned to its element, a missing or misaligned workspace with
 * numel_seg > 0. Types and count sizes not built: CLO_HIP_EUNSUPPORTED. A workspace below
 * clo_hip_segscan_workspace_bytes(numel_seg, numel): CLO_HIP_EWORKSPACE. data_out may be exactly values_in when the two
 * types are equally wide; no other overlap of an output with an input, num_in or the other output is allowed (not
 * checked here: the driver does). numel_seg 0 needs no workspace and writes *num_out = 0 alone. Whatever the arrays
 * hold, reads stay inside the inputs, writes inside data_out[0, numel) and num_out, and the call completes.
 * Launches: for the counts form the three of clo_hip_expand that write the ends into the workspace; one thread per tile
 * boundary of the MERGE of the m clipped ends with the n row indices, which finds its split by a halving and writes
 * num_out; one work-group per tile of clo_hip_segscan_tile merge steps that reduces the rows the tile takes after its
 * last close; one work-group that scans the tiles' states; one work-group per tile that scans its steps from the
 * tile's carry and writes its rows as one stretch. values_in is read once plus those open tails. No work-group waits
 * for another and there are no global atomics; asynchronous on `stream`; nothing is allocated and the host never waits,
 * so the call can be captured into a graph. clo_hip_segscan_tile: 0 for sizes not built.
 * clo_hip_segscan_workspace_bytes is monotone in both arguments, 0 for (0, 0) and a multiple of
 * CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_SEGSCAN_COUNTS 0
#define CLO_HIP_SEGSCAN_OFFSETS 1
size_t clo_hip_segscan_tile(int value_size, int sum_size);
size_t clo_hip_segscan_workspace_bytes(size_t numel_seg, size_t numel);
int clo_hip_segscan(int op, int inclusive, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* data_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- arg-min and arg-max per segment (new functionality: CloSegArg, include/clo_segarg.h) ----
 * m = min(numel_seg, *num_in), the forms (CLO_HIP_SEGARG_COUNTS, CLO_HIP_SEGARG_OFFSETS), the inclusive ends e_r,
 * count_size and num_out = e_(m-1) unclamped are clo_hip_expand's above. value_type is a CloType number: int, uint, long,
 * ulong, float or double. With n = numel rows of values_in, e_(-1) = 0 and x(i) the order key of values_in[i] (two's
 * complement with the sign bit flipped, IEEE total order; complemented for CLO_HIP_SEGARG_ARGMAX), for every r < m whose
 * range [min(e_(r-1), n), min(e_r, n)) holds a row: idx_out[r] = the row i of the range with the smallest x(i), among
 * equal ones the smallest i (CLO_HIP_SEGARG_FIRST) or the largest (CLO_HIP_SEGARG_LAST), and val_out[r] = values_in[i]
 * bit for bit. A range without a row: idx_out[r] = 0xffffffff and val_out[r] = the value whose key is all ones. Whether a
 * range has a row is read from its ends. val_out may be NULL. Rows r >= m are not written.
 * CLO_HIP_EARGS: an op, tie or form that is none of the numbers below, numel_seg or numel >= 2^32, a missing
 * counts_or_offsets (numel_seg > 0, or the offsets form), values_in (numel > 0) or idx_out (numel_seg > 0), num_out NULL
 * or misaligned, num_in misaligned, a pointer not aligned to its element, a missing or misaligned workspace with
 * numel_seg > 0. Types and count sizes not built: CLO_HIP_EUNSUPPORTED. A workspace below
 * clo_hip_segarg_workspace_bytes(numel_seg, numel): CLO_HIP_EWORKSPACE. No output may overlap an input, num_in or
 * another output (not checked here: the driver does). numel_seg 0 needs no workspace and writes *num_out = 0 alone.
 * Whatever the arrays hold, reads stay inside the inputs, writes inside idx_out[0, numel_seg), val_out[0, numel_seg)
 * and num_out, and the call completes.
 * Launches: clo_hip_segreduce's five stages with the aggregate (order key, index): the three that write the ends of the
 * counts form; one thread per tile boundary of the merge of ends and rows; one work-group per tile of
 * clo_hip_segarg_tile merge steps, which writes idx_out and val_out of every segment that closes in it and leaves its
 * open aggregate, and what it holds of its first closing segment, in the workspace; one work-group that scans the
 * tiles' open aggregates, clo_hip_segarg_carry_tiles of them per trip; one thread per tile that writes the tile's first
 * closing segment from the carry and the tile's part. values_in is read once; val_out is decoded from the winning key,
 * not gathered. No work-group waits for another and there are no global atomics; asynchronous on `stream`; nothing is
 * allocated and the host never waits, so the call can be captured into a graph. clo_hip_segarg_tile: 0 for sizes not
 * built. clo_hip_segarg_workspace_bytes is monotone in both arguments, 0 for (0, 0) and a multiple of
 * CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_SEGARG_ARGMIN 0
#define CLO_HIP_SEGARG_ARGMAX 1
#define CLO_HIP_SEGARG_FIRST 0
#define CLO_HIP_SEGARG_LAST 1
#define CLO_HIP_SEGARG_COUNTS 0
#define CLO_HIP_SEGARG_OFFSETS 1
size_t clo_hip_segarg_tile(int value_size);
size_t clo_hip_segarg_carry_tiles(void);
size_t clo_hip_segarg_workspace_bytes(size_t numel_seg, size_t numel);
int clo_hip_segarg(int op, int tie, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	uint32_t* idx_out, void* val_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- the k smallest or largest rows of every segment (new functionality: CloSegTopK, include/clo_segtopk.h) ----
 * m = min(numel_seg, *num_in), the forms (CLO_HIP_SEGTOPK_COUNTS, CLO_HIP_SEGTOPK_OFFSETS), the inclusive ends e_r,
 * count_size and num_out = e_(m-1) unclamped are clo_hip_expand's above; key_type, value_size and the arg form
 * (value_size 4, values_in NULL, keys_out optional) are clo_hip_segsort's. With n = numel rows, e_(-1) = 0 and x(i) the
 * order key of keys_in[i] (complemented for CLO_HIP_SEGTOPK_LARGEST), for every r < m: counts_out[r] = c_r = min(k, the
 * rows of [min(e_(r-1), n), min(e_r, n))), and keys_out[r * k + j], values_out[r * k + j] for j < c_r are the range's
 * j-th row in the stable sort by x: ascending x, equal x by ascending row. Keys keep their bits; the arg form writes
 * the global row as uint. Slots j >= c_r, rows r >= m and counts_out[r >= m] are not written. k is a host argument.
 * CLO_HIP_EARGS: a which or form that is none of the numbers below, numel_seg or numel >= 2^32, k above
 * clo_hip_segtopk_k_max, numel_seg * k >= 2^32, clo_hip_segsort's missing pointers, counts_out NULL with numel_seg > 0
 * and k > 0, num_out NULL or misaligned, num_in misaligned, a pointer not aligned to its element, a missing or
 * misaligned workspace with numel_seg > 0. Key types, value and count sizes not built: CLO_HIP_EUNSUPPORTED. A
 * workspace below clo_hip_segtopk_workspace_bytes(numel_seg, numel, k, key_size, value_size): CLO_HIP_EWORKSPACE. No
 * output may overlap an input, num_in or another output (not checked here: the driver does). numel_seg 0 needs no
 * workspace and writes *num_out = 0 alone; k 0 writes num_out alone. Whatever the arrays hold, reads stay inside the
 * inputs, writes inside [0, numel_seg * k) of keys_out and values_out, counts_out[0, numel_seg) and num_out, and the
 * call completes.
 * The workspace holds the segment ends of the counts form, a byte and a segment number per row, 32 bytes per tile and
 * per tile two candidate lists of k (order key, row) pairs.
 * Launches: for the counts form the three of clo_hip_expand that write the ends; a memset of the row bytes; one thread
 * per segment and per tile that marks and numbers the first row of every non-empty segment, writes counts_out, num_out
 * and the tile's two boundary segments; one work-group per tile of clo_hip_segtopk_tile rows that sorts them on chip by
 * (segment, x, row) — clo_hip_segsort's network — and writes the first k of every segment inside the tile to the
 * outputs and of the two that cross its boundaries to the candidate lists; ceil(log2(tiles)) combine levels, one
 * work-group per tile, each of which leaves at once unless a list of its tile takes in the list 2^level tiles further
 * on. No work-group waits for another and there are no global atomics; asynchronous on `stream`; nothing is allocated
 * and the host never waits, so the call can be captured into a graph.
 * clo_hip_segtopk_tile: T, clo_hip_segtopk_k_max: the largest k (T / 2); both 0 for sizes not built.
 * clo_hip_segtopk_workspace_bytes is monotone in the two counts and in k, 0 for (0, 0, ., ., .) and a multiple of
 * CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_SEGTOPK_SMALLEST 0
#define CLO_HIP_SEGTOPK_LARGEST 1
#define CLO_HIP_SEGTOPK_COUNTS 0
#define CLO_HIP_SEGTOPK_OFFSETS 1
size_t clo_hip_segtopk_tile(int key_size, int value_size);
size_t clo_hip_segtopk_k_max(int key_size, int value_size);
size_t clo_hip_segtopk_workspace_bytes(size_t numel_seg, size_t numel, size_t k, int key_size, int value_size);
int clo_hip_segtopk(int which, int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* keys_in, const void* values_in,
	void* keys_out, void* values_out, uint32_t* counts_out, uint64_t* num_out, size_t numel_seg, size_t numel, size_t k, int key_type, int value_size,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- floating-point sums per segment in a fixed order (new functionality: CloSegFSum, include/clo_segfsum.h) ----
 * m = min(numel_seg, *num_in), the forms (CLO_HIP_SEGFSUM_COUNTS, CLO_HIP_SEGFSUM_OFFSETS), the inclusive ends e_r,
 * count_size and num_out = e_(m-1) unclamped are clo_hip_expand's above. value_type and sum_type are CloType numbers,
 * one of the pairs half -> float, float -> float, float -> double, double -> double. With n = numel rows of values_in
 * and e_(-1) = 0, for every r < m: sums_out[r] = the sum over i in [min(e_(r-1), n), min(e_r, n)) of (sum type)
 * values_in[i], +0 where that range is empty; every addition is one IEEE addition in the sum type, in the order
 * include/clo_segfsum.h states, which m, n and the clipped ends alone determine. Rows r >= m are not written.
 * CLO_HIP_EARGS: a form that is neither number below, numel_seg or numel >= 2^32, counts_or_offsets NULL with
 * numel_seg > 0 (offsets: always), values_in NULL with numel > 0, sums_out NULL with numel_seg > 0, num_out NULL or
 * misaligned, num_in misaligned, a pointer not aligned to its element, a missing or misaligned workspace with
 * numel_seg > 0. Type pairs and count sizes not built: CLO_HIP_EUNSUPPORTED. A workspace below
 * clo_hip_segfsum_workspace_bytes(numel_seg, numel): CLO_HIP_EWORKSPACE. Neither output may overlap an input, num_in
 * or the other output (not checked here: the driver does). numel_seg 0 needs no workspace and writes *num_out = 0 alone.
 * Whatever the arrays hold, reads stay inside the inputs, writes inside sums_out[0, numel_seg) and num_out, and the
 * call completes.
 * Launches: clo_hip_segreduce's five stages with a floating-point aggregate that crosses lanes and lies in the
 * workspace as its bits. values_in is read once. No work-group waits for another and there are no global atomics;
 * asynchronous on `stream`; nothing is allocated and the host never waits, so the call can be captured into a graph.
 * clo_hip_segfsum_tile: T = 4352 merge steps for the four pairs' sizes (2, 4), (4, 4), (4, 8), (8, 8), 0 otherwise.
 * clo_hip_segfsum_workspace_bytes is monotone in both arguments, 0 for (0, 0) and a multiple of
 * CLO_HIP_WORKSPACE_ALIGN. */
#define CLO_HIP_SEGFSUM_COUNTS 0
#define CLO_HIP_SEGFSUM_OFFSETS 1
size_t clo_hip_segfsum_tile(int value_size, int sum_size);
size_t clo_hip_segfsum_workspace_bytes(size_t numel_seg, size_t numel);
int clo_hip_segfsum(int form, const void* counts_or_offsets, int count_size, const uint64_t* num_in, const void* values_in,
	void* sums_out, uint64_t* num_out, size_t numel_seg, size_t numel, int value_type, int sum_type,
	void* workspace, size_t workspace_bytes, void* stream);

/* ---- LSD radix sort (replaces the per-digit loop of
 *      sort/clo_sort_satradix.c:264-313: satradix_localsort, satradix_histogram,
 *      clo_scan_with_device_data, satradix_scatter — sort/clo_sort_satradix.cl:34-258) ----
 * Stable ascending sort of `numel` elements of elem_size bytes by the key
 * field  key = (elem >> key_shift) & ((1<<key_bits)-1), digits of
 * `digit_bits` bits (1..8; radix = 1<<digit_bits), least significant first.
 * key_kind: 0 = unsigned (raw bit order, what upstream's kernels do for every
 * type), 1 = two's complement, 2 = IEEE-754 (key_bits 16/32/64; -0 < +0, NaNs
 * at the ends by sign) — kinds 1 and 2 go through an order-preserving
 * transform on the first read and back on the last write, so negative keys
 * land where upstream's own check (benchmarks/clo_bench.c:26-65) wants them.
 * src is read, the sorted result is written to dst; tmp is scratch of the same
 * size. dst may equal src (in place); tmp must be distinct from both. src is
 * left untouched when dst != src. Asynchronous on `stream`. */
/* Loads the code objects of the radix passes that a small first sort does not reach (HIP loads one at the first launch
 * that needs it; upstream builds and loads every kernel in clo_sort_new, sort/clo_sort_abstract.c:144-179). */
int clo_hip_radix_preload(void);
size_t clo_hip_radix_workspace_bytes(size_t numel, int elem_size, int key_bits, int digit_bits);
/* 1 if the kernels of such a sort wait for other work-groups (the single-sweep
 * passes hand digit counts from tile to tile; every spin is bounded and a give-up
 * raises the workspace's status word: clo_hip_check_status), 0 if none does (the
 * chain-free passes). */
int clo_hip_radix_polls(size_t numel, int elem_size, int digit_bits);
int clo_hip_radix_sort(const void* src, void* dst, void* tmp, size_t numel,
	int elem_size, int key_shift, int key_bits, int key_kind, int digit_bits,
	void* workspace, size_t workspace_bytes, void* stream);
/* The same sort FED by whoever produced the keys: first_digits[i] = the low 8 bits of element i's key field,
 * (elem[i] >> key_shift) & 0xff (device memory, numel bytes at any byte address, read before anything is written —
 * it may live in `tmp`). The one re-read of the keys the sort has left is its first histogram; a producer that touches every
 * key anyway (a key extractor, a generator, the pass before in a pipeline) writes those bytes for nearly nothing
 * and the histogram reads numel bytes instead of numel elements. clo_hip_radix_takes_first_digits says whether a
 * sort of this shape reads them (1: the chain-free passes on 16 384-element tiles, radix 16 or 256, unsigned
 * keys) — otherwise they are ignored, NULL is always allowed. */
int clo_hip_radix_takes_first_digits(size_t numel, int elem_size, int key_kind, int digit_bits);
int clo_hip_radix_sort_fed(const void* src, void* dst, void* tmp, size_t numel,
	int elem_size, int key_shift, int key_bits, int key_kind, int digit_bits, const unsigned char* first_digits,
	void* workspace, size_t workspace_bytes, void* stream);
/* Key-value sort (new functionality: clo_sort_by_key_with_device_data, include/clo_sort.h): the stable order of the
 * key field as above, of `numel` elements of key_size (1, 2, 4) bytes in keys_in, carried over to 4-byte values:
 * keys_out[j] = keys_in[order[j]], values_out[j] = values_in[order[j]]. values_in NULL: the values are 0 .. numel - 1
 * (argsort); keys_out NULL: no keys are written; values_out is required. keys_out may equal keys_in and values_out
 * values_in (in place). What is sorted are 8-byte pairs (element << 32 | value); pairs_a and pairs_b are scratch of
 * numel * 8 bytes each, distinct from each other and from the four arrays. Where clo_hip_radix_sort would run the
 * chain-free radix-16 / 256 passes on 8-byte elements, the first pass (and its histogram) reads the two arrays and
 * the last one writes them; elsewhere a pack and an unpack kernel go around the pair sort. Its kernels poll exactly
 * when those of an 8-byte sort do: clo_hip_radix_polls(numel, 8, digit_bits). Asynchronous on `stream`. */
size_t clo_hip_radix_kv_workspace_bytes(size_t numel, int key_size, int key_bits, int digit_bits);
int clo_hip_radix_sort_kv(const void* keys_in, const void* values_in, void* keys_out, void* values_out, void* pairs_a, void* pairs_b,
	size_t numel, int key_size, int key_shift, int key_bits, int key_kind, int digit_bits,
	void* workspace, size_t workspace_bytes, void* stream);
/* Diagnostic: a device buffer of 8 x tiles uint64 that the LAST single-sweep pass of a sort fills with per-tile
 * s_memtime stamps (tile drawn ... stored) until it is taken away again with NULL. Process-wide, off by default. */
int clo_hip_radix_debug_stamps(void* buffer, size_t tiles);

/* Segmented sort (new functionality, the local step of the sharded sort): `nseg` (1..256) segments of ONE array —
 * seg_counts[i] elements each, host memory, summing to numel — are sorted independently, each stably by the key
 * field [key_shift, key_shift + key_bits), in SHARED launches: a launch's tiles and counter-scan chunks are
 * numbered through all segments and one small table lookup tells a work-group which segment it works for.
 * Sub-buckets that share their top key bits (what an MSD partition leaves) are thereby sorted on the REMAINING
 * bits at the rate of one large sort, where sorting them one by one would be launch-bound.
 * Where the segments lie: the RESULT holds them back to back in order (segment k at the sum of the counts before
 * it). The SOURCE `src` either holds them the same way (npieces = 0) or in up to 256 PIECES anywhere in it
 * (offsets below 2^32 elements): piece i = piece_counts[i] elements from piece_offsets[i], belonging to segment
 * piece_segment[i], pieces listed in segment order (what a rank of the sharded sort receives: one piece per
 * source rank and sub-bucket); the first pass then gathers a segment's pieces, in the order listed, as a
 * by-product. The first pass reads `src` and writes `b` (numel elements), the later ones go b -> a -> b ...: the
 * result is in `b` when *result_in_b comes back 1 (an odd number of 8-bit passes, ceil(key_bits / 8)), else in
 * `a`. `src` may be `a` itself (the first pass is the only one to read it); otherwise it is left untouched.
 * digit_bits 4 or 8 (radix 16 / 256), elem_size 4 or 8, unsigned keys. Asynchronous; the host arrays are read
 * before the call returns. */
size_t clo_hip_radix_seg_workspace_bytes(size_t numel, int nseg, int elem_size, int digit_bits);
int clo_hip_radix_sort_segmented(const void* src, void* a, void* b, size_t numel, const size_t* seg_counts, int nseg,
	const size_t* piece_counts, const size_t* piece_offsets, const int* piece_segment, int npieces,
	int elem_size, int key_shift, int key_bits, int digit_bits, void* workspace, size_t workspace_bytes, void* stream,
	int* result_in_b);
/* The same with the pieces in TWO sources: piece i lies in `src2` when piece_source[i] is 1 (piece_source NULL: all in
 * `src`), its offset counted from that source's start. What it is for: the piece of a sub-bucket that a rank of the
 * sharded sort keeps for itself never needs to move — it is gathered straight out of the partitioned shard, and the
 * rank's own share of every exchange (1 / G of the bytes; all of them on one rank) is not copied at all. `src2` is
 * only read, by the first pass; it must not be `b`. */
int clo_hip_radix_sort_segmented2(const void* src, const void* src2, void* a, void* b, size_t numel, const size_t* seg_counts, int nseg,
	const size_t* piece_counts, const size_t* piece_offsets, const int* piece_segment, const int* piece_source, int npieces,
	int elem_size, int key_shift, int key_bits, int digit_bits, void* workspace, size_t workspace_bytes, void* stream,
	int* result_in_b);

/* MSD bucket partition used by the multi-GPU exchange (new
 * functionality): stable split of src into 1<<bucket_bits buckets by the top
 * bucket_bits of the key field; dst gets the buckets back to back in bucket
 * order. counts_dev (device, 1<<bucket_bits uint64; may be NULL for the
 * partition) receives the bucket sizes — the partition produces them as a
 * by-product, clo_hip_msd_histogram computes them alone. bucket_bits: 1..8 for
 * the partition (the sharded sort splits on 8: ranks x sub-buckets per rank = 256,
 * include/clo_shard.h), 1..3 for the histogram alone. */
int clo_hip_msd_histogram(const void* src, size_t numel, int elem_size,
	int key_shift, int key_bits, int bucket_bits,
	uint64_t* counts_dev, void* stream);
int clo_hip_msd_partition(const void* src, void* dst, size_t numel, int elem_size,
	int key_shift, int key_bits, int bucket_bits, uint64_t* counts_dev,
	void* workspace, size_t workspace_bytes, void* stream);
size_t clo_hip_msd_workspace_bytes(size_t numel, int elem_size, int bucket_bits);

/* ---- RCCL over xGMI: the two collectives of the sharded sort (include/clo_shard.h;
 *      new functionality, the reference is single-device). One communicator per
 *      process = per GPU; the 128-byte id is made by one rank and handed to the
 *      others by whatever side channel the launcher has. Both calls are ordered on
 *      `stream`. all_to_all_v: rank r's bytes [send_offset[p], +send_bytes[p]) go to
 *      peer p and land at its [recv_offset[r], +recv_bytes[r]); ONE group of
 *      ncclSend / ncclRecv pairs, every pair on its own xGMI link. ---- */
#define CLO_HIP_RCCL_ID_BYTES 128
int clo_hip_rccl_unique_id(void* id_out);
int clo_hip_rccl_comm_create(void** comm, const void* id_in, int rank, int world);
int clo_hip_rccl_comm_destroy(void* comm);
/* ncclCommAbort: ends the communicator NOW; operations of it that are pending on any
 * rank's streams fail instead of waiting for this rank for ever. What a rank that
 * cannot take part in a collective its peers have already entered calls before it
 * returns its error. The handle is gone afterwards (no clo_hip_rccl_comm_destroy). */
int clo_hip_rccl_comm_abort(void* comm);
/* ncclCommGetAsyncError: 0 while the communicator is healthy, the RCCL status of an asynchronous failure (a peer that
 * died, a network error) once there is one. Never blocks. */
int clo_hip_rccl_comm_async_error(void* comm);
int clo_hip_rccl_all_gather_u64(void* comm, const uint64_t* send_dev, uint64_t* recv_dev, size_t count, void* stream);
int clo_hip_rccl_all_to_all_v(void* comm, int rank, int world,
	const void* send_dev, const size_t* send_bytes, const size_t* send_offset_bytes,
	void* recv_dev, const size_t* recv_bytes, const size_t* recv_offset_bytes, void* stream);

/* ---- bitonic sorts (replace the launch loops of
 *      sort/clo_sort_sbitonic.c:102-118 / sort/clo_sort_sbitonic.cl:38-69 and
 *      sort/clo_sort_abitonic.c:401-432 / sort/clo_sort_abitonic.cl:234-1067) ----
 * In-place bitonic network over nlpo2(numel) slots (numel need not be a power
 * of two: the caller provides a buffer of clo_hip_bitonic_padded_numel(numel)
 * elements and the call pads the tail so that it sorts to the end, i.e.
 * data[0..numel) comes out sorted). The key is the low key_bits bits of
 * (KEY_TYPE)(elem >> key_shift), KEY_TYPE being key_size bytes wide;
 * key_kind: 0 unsigned, 1 signed, 2 float (then key_bits = 8*key_size).
 * descending: CLO_SORT_COMPARE "((a) < (b))".
 * clo_hip_bitonic_simple: one launch per (stage, step) — the sbitonic schedule.
 * clo_hip_bitonic_tiled: LDS/register-tiled schedule — the abitonic replacement.
 * *launches (may be NULL) receives the number of kernel launches made. */
size_t clo_hip_bitonic_padded_numel(size_t numel);
int clo_hip_bitonic_simple(void* data, size_t numel, int elem_size,
	int key_shift, int key_bits, int key_size, int key_kind, int descending,
	int* launches, void* stream);
/* In place, ANY numel and any key: the flip form of the network (every comparator ascending, comparators that reach
 * past numel skipped), one launch per step. What the drivers use for a numel that is not a power of two when the key
 * is only part of the element (for whole-element keys they pad and run the fast schedules). */
int clo_hip_bitonic_any(void* data, size_t numel, int elem_size,
	int key_shift, int key_bits, int key_size, int key_kind, int descending, int* launches, void* stream);
int clo_hip_bitonic_tiled(void* data, size_t numel, int elem_size,
	int key_shift, int key_bits, int key_size, int key_kind, int descending,
	int* launches, void* stream);

/* ---- gselect (replaces the launch of sort/clo_sort_gselect.c:60-118 /
 *      sort/clo_sort_gselect.cl:38-58): O(n^2) rank sort, stable, out of place
 *      (dst != src); key description as for the bitonic sorts. ---- */
int clo_hip_gselect(const void* src, void* dst, size_t numel, int elem_size,
	int key_shift, int key_bits, int key_size, int key_kind, int descending, void* stream);

/* ---- bitonic sorts specialised at run time (hiprtc) for arbitrary compare /
 *      get_key expressions — what upstream does for every sorter by OpenCL JIT
 *      (sort/clo_sort_abstract.c:144-179). elem_type / key_type: CloType numbers.
 *      compare: body of CLO_SORT_COMPARE(a, b) (NULL: "((a) > (b))"); get_key:
 *      body of CLO_SORT_KEY_GET(x) (NULL: "(x)"). compiler_opts (may be NULL): the
 *      caller's options for the compiler, white-space separated, as upstream hands
 *      them to the OpenCL JIT (sort/clo_sort_abstract.c:177-178) — -DNAME[=value] /
 *      -UNAME / -Idir reach hiprtc (also spelled "-D NAME"), OpenCL's own -cl-...
 *      switches are dropped, anything else is the compiler's to accept or refuse. On a
 *      compile error returns CLO_HIP_EARGS and, if log != NULL, a malloc'd build log
 *      (caller frees). ----
 */
int clo_hip_bitonic_jit_create(int elem_type, int key_type, const char* compare, const char* get_key, const char* compiler_opts,
	void** handle, char** log);
void clo_hip_bitonic_jit_destroy(void* handle);
/* In place, numel a power of two. tiled: 0 = sbitonic schedule, 1 = abitonic. */
/* gselect (upstream's O(n^2) rank sort, sort/clo_sort_gselect.cl:38-58) through the same compiled module:
 * src -> dst (distinct), ties by index. */
int clo_hip_bitonic_jit_gselect(void* handle, const void* src, void* dst, size_t numel, void* stream);
int clo_hip_bitonic_jit_sort(void* handle, void* data, size_t numel, int tiled, int* launches, void* stream);
/* Static LDS bytes per work-group of the kernels that call would launch (0: one launch per step, registers only). */
size_t clo_hip_bitonic_jit_lds_bytes(void* handle, size_t numel, int tiled);

/* ---- satradix specialised at run time (hiprtc) for a get_key expression
 *      outside the ahead-of-time family: the key is materialised as
 *      (ordered key bits << 32 | index) pairs by a compiled kernel, the pairs are
 *      radix-sorted, the elements gathered. 8-byte keys take two such rounds
 *      (low half of the key, then the high half in the first round's order).
 *      pairs / pairs_tmp: numel * 8 bytes each; workspace as for
 *      clo_hip_radix_workspace_bytes(numel, 8, 32, digit_bits). ---- */
int clo_hip_radix_jit_create(int elem_type, int key_type, const char* get_key, const char* compiler_opts, void** handle, char** log);
void clo_hip_radix_jit_destroy(void* handle);
int clo_hip_radix_jit_sort(void* handle, const void* src, void* dst, void* pairs, void* pairs_tmp, size_t numel,
	int digit_bits, void* workspace, size_t workspace_bytes, void* stream);

/* ---- status word of the bounded spins ----
 * The scan is the one kernel that polls other work-groups' state (decoupled
 * look-back); it bounds every spin (CLO_MAX_SPINS polls; the environment
 * variable of that name overrides the bound) and on give-up sets a word in its
 * workspace and finishes with wrong output. This reads the word back
 * (synchronises `stream`). Returns 0, CLO_HIP_ETIMEOUT or a hip error; after
 * CLO_HIP_ETIMEOUT the workspace must be initialised again. The host drivers
 * check it wherever they synchronise anyway (clo_scan_with_host_data,
 * ccl_queue_finish, ccl_event_wait). Meaningful for the workspaces of the scan
 * and of clo_hip_msd_partition (always 0 there: no kernel of the sorts waits on
 * another work-group) and of clo_hip_radix_sort when clo_hip_radix_polls() says
 * its kernels poll — the caller clears the first 512 bytes of that workspace once
 * after allocating it, the sorts never clear the word themselves. */
int clo_hip_check_status(void* workspace, void* stream);

/* ---- launch observer: per-kernel events for profiling queues ----
 * Upstream names every kernel launch it enqueues (ccl_event_set_name at
 * sort/clo_sort_satradix.c:282,295,312, scan/clo_scan_blelloch.c:158,183,193) and
 * CCLProf reports per name. The C-ABI calls below launch several kernels each;
 * while an observer is installed (per calling thread), it is told about every
 * launch: phase 0 right before (label = the kernel family: "radix_hist",
 * "radix_offsets", "radix_pass", "radix_small", "scan", "bitonic_step", ...),
 * phase 1 right after (label NULL), with the stream the launch went to. The
 * host drivers use it to record one CCLEvent per kernel when the queue was
 * created with CL_QUEUE_PROFILING_ENABLE. NULL removes it. */
typedef void (*clo_hip_launch_observer)(void* user, const char* label, int phase, void* stream);
int clo_hip_set_launch_observer(clo_hip_launch_observer fn, void* user);

/* ---- per-kernel device timing (measurement only; bench.py's roofline leg) ----
 * While enabled, every kernel launch made by this library is bracketed by a
 * pair of HIP events recorded on the stream the kernel runs on.
 * clo_hip_timing_read sums the elapsed time of the launches recorded under
 * `label` since the last reset ("radix_pass", "radix_hist", "radix_offsets",
 * "radix_small", "msd_partition", "scan", "reduce", "bitonic_presort",
 * "bitonic_tile", "bitonic_strided", "bitonic_step", "gselect"). */
int clo_hip_timing_enable(int on);
int clo_hip_timing_enabled(void);
int clo_hip_timing_reset(void);
int clo_hip_timing_read(const char* label, unsigned* count, float* total_ms);

/* Static LDS bytes per work-group of the kernel families, for the
 * get_localmem_usage introspection calls (sort/clo_sort_satradix.c:626-658,
 * scan/clo_scan_blelloch.c:307-319). family: "radix_hist", "radix_pass",
 * "scan", "bitonic_tile", "bitonic_strided", "bitonic_step". */
size_t clo_hip_kernel_lds_bytes(const char* family, int elem_size, int param);
/* Static LDS bytes per work-group of the kernels the bitonic schedules launch for `numel` elements: tiled = 1 the tiled
 * schedule (clo_hip_bitonic_tiled: 0 below 32 elements, the run-time-schedule tile kernel up to one tile, the
 * compile-time-schedule kernels on 2^14-element tiles — 2^13 of 8 bytes — above), tiled = 0 one launch per step (0). */
size_t clo_hip_bitonic_lds_bytes(size_t numel, int elem_size, int tiled);

/* ---- CloRng (include/clo_rng.h; upstream: rng/clo_rng.c, rng/clo_rng_*.cl) ----
 * gen: the generator's place in CLO_RNG_IMPLS (0 lcg, 1 xorshift64, 2 xorshift128, 3 mwc64x, 4 parkmiller,
 * 5 tauslcg); `states`: device memory of `count` states of that generator's seed size.
 * clo_hip_rng_device_source: the text of include/clo_rng/clo_rng_device.hpp, fixed when the library was built.
 * clo_hip_rng_init: states[g] = from_ulong(hash(g + main_seed)) for g < count (clo_rng_init.cl); hash 0 none,
 * 1 KNUTH, 2 XS1. Asynchronous on `stream`.
 * clo_hip_rng_init_jit: the same with `hash` the body of #define CLO_RNG_HASH(x), compiled with hiprtc; returns when
 * the kernel has run. CLO_HIP_EARGS with the compiler's log in *log (malloc'd; the caller frees it) when the hash
 * does not compile.
 * clo_hip_rng_fill: out[i] = f(draw i / count of state i % count) for i < numel, f(x) = x >> (32 - bits), or
 * x % maxint when maxint != 0 (bits 1..32 either way); the states advance by their number of draws. One launch,
 * asynchronous on `stream`. layout: 0 the library's choice (one state per lane), 1 one state per lane, 4 four
 * consecutive states per lane, one 16-byte store per draw (count % 4 == 0 and `out` 16-byte aligned, else
 * CLO_HIP_EARGS; measured slower, for comparison). */
const char* clo_hip_rng_device_source(void);
int clo_hip_rng_init(int gen, void* states, size_t count, uint64_t main_seed, int hash, void* stream);
int clo_hip_rng_init_jit(int gen, const char* hash, void* states, size_t count, uint64_t main_seed, void* stream, char** log);
int clo_hip_rng_fill(int gen, void* states, size_t count, unsigned* out, size_t numel, unsigned bits, unsigned maxint,
	int layout, void* stream);

#ifdef __cplusplus
}
#endif
#endif
