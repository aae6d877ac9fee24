/*
 * clo_internal.h — helpers shared by the host drivers (not installed).
 */
#ifndef CLO_INTERNAL_H
#define CLO_INTERNAL_H

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>

#include "clo_common.h"
#include "clo_hip.h"

#ifdef CLO_USE_GLIB
#define clo_return_if_fail g_return_if_fail
#define clo_return_val_if_fail g_return_val_if_fail
#define clo_gerror_set g_set_error
#define clo_gerror_propagate g_propagate_error
#else
/* g_return_*_if_fail: a soft assertion — complain on stderr, return a default. */
#define clo_return_if_fail(expr) \
	do { if (!(expr)) { fprintf(stderr, "cl_ops-CRITICAL: %s: assertion '%s' failed\n", __func__, #expr); return; } } while (0)
#define clo_return_val_if_fail(expr, val) \
	do { if (!(expr)) { fprintf(stderr, "cl_ops-CRITICAL: %s: assertion '%s' failed\n", __func__, #expr); return (val); } } while (0)
#endif

/* CLO_DEBUG=1 in the environment turns on the g_debug-style trace upstream
 * emits under log domain "cl_ops" (e.g. clo_sort_satradix.c:171,192). */
/* Helpers shared by the host drivers: not part of the library's interface (the headers under include/ are), so not exported either. */
#define CLO_INTERNAL __attribute__((visibility("hidden")))

CLO_INTERNAL int clo_debug_enabled(void);
#define clo_debug(...) do { if (clo_debug_enabled()) { fprintf(stderr, "cl_ops-DEBUG: " __VA_ARGS__); fputc('\n', stderr); } } while (0)

/* Environment switches of the host drivers: read when an object is made, never per call. CLO_NO_WARMUP (no
 * dummy sorts / scans at the first object of a kind), and the 0 / 1 switches CLO_SORT_HOST_PIPELINE (satradix's
 * clo_sort_with_host_data: pipelined or blocking whatever the queue) and CLO_SBITONIC_STEPS (sbitonic with one
 * launch per step). */
CLO_INTERNAL int clo_env_no_warmup(void);
CLO_INTERNAL int clo_env_flag(const char* name);

/* A grow-only device allocation cached inside a sorter/scanner object, so the
 * hot path never calls hipMalloc after the first use (upstream allocates and
 * frees its aux buffers on every call: clo_sort_satradix.c:242-257,327-330). */
typedef struct {
	void* ptr;
	size_t bytes;
} clo_devbuf;

/* Returns 0 or a clo_hip status. Contents are NOT preserved when it grows. */
CLO_INTERNAL int clo_devbuf_reserve(clo_devbuf* b, size_t bytes);
CLO_INTERNAL void clo_devbuf_release(clo_devbuf* b);

/* Buffers cached in a sorter / scanner belong to one queue at a time. When a
 * call arrives on another queue than the previous one, its work must come after
 * the previous call's. The guard remembers the QUEUE of the last call (holding
 * its struct, clo_queue_hold), not a stream handle: the queue may have been
 * destroyed meanwhile (clo_*_with_host_data makes and destroys a queue of its own
 * when the caller passes none; round 1 kept the raw handle and called
 * hipStreamSynchronize on it later: undefined behaviour, observed as an abort
 * inside the HIP runtime) — a destroyed queue was synchronised when it went, so
 * nothing is left to wait for; a live one gets an event recorded on it now, and
 * the new queue's stream waits for that. Calls that stay on one queue pay
 * nothing (an event per call cost 3.5 us of device time between two kernels). */
typedef struct {
	CCLQueue* cq;    /* the queue of the last call (held), or NULL */
	void* evt;       /* created the first time two live queues alternate */
} clo_stream_guard;
CLO_INTERNAL int clo_stream_guard_enter(clo_stream_guard* g, CCLQueue* cq);   /* before the call's first enqueue; 0 or a clo_hip status */
CLO_INTERNAL void clo_stream_guard_release(clo_stream_guard* g);

/* A launch sequence that depends only on its arguments (buffers, size,
 * stream), cached as an executable hipGraph: the FIRST call with a given key
 * launches normally, a second consecutive call with the same key captures the
 * sequence and replays it, later ones replay. Any other key drops the graph.
 * Never used while per-kernel timing is on (its event pairs need real
 * launches). `enqueue` puts the whole sequence on `stream` and returns a
 * clo_hip status. */
typedef struct {
	void* exec;
	const void* k0;
	const void* k1;
	void* stream;
	size_t n;
	int variant, seen;
} clo_graph_cache;
typedef int (*clo_enqueue_fn)(void* user, void* stream);
CLO_INTERNAL int clo_graph_cache_run(clo_graph_cache* gc, int allowed, const void* k0, const void* k1, size_t n, int variant,
	void* stream, clo_enqueue_fn enqueue, void* user);
CLO_INTERNAL void clo_graph_cache_release(clo_graph_cache* gc);

/* Extensions of a scan implementation that are NOT part of the public
 * CloScanImplDef (whose layout is upstream's, clo_scan_abstract.in.h:41-103: a
 * plugin compiled against upstream's header must stay valid). Looked up by
 * implementation name; an implementation without an entry simply has none.
 *  scan_chunk: scans `numel` elements at raw device pointers as one chunk of a
 *    longer array: *carry_in_dev (device uint64, NULL = 0) is added to every
 *    output, *carry_out_dev receives the next chunk's carry. Enqueued on cq_exec
 *    as one command (a profiling queue sees it like any scan). Used by the
 *    pipelined clo_scan_with_host_data.
 *  check_status: after cq has been synchronised, fails with CLO_ERROR_LIBRARY if
 *    a kernel of this scanner gave up a bounded spin (wrong output). */
struct clo_scan;
typedef struct {
	const char* name;
	cl_bool (*scan_chunk)(struct clo_scan* scanner, CCLQueue* cq_exec, const void* in_dev, void* out_dev, size_t numel,
		const void* carry_in_dev, void* carry_out_dev, GError** err);
	cl_bool (*check_status)(struct clo_scan* scanner, CCLQueue* cq, GError** err);
} clo_scan_impl_ext;
CLO_INTERNAL const clo_scan_impl_ext* clo_scan_impl_ext_find(const char* name);
CLO_INTERNAL extern const clo_scan_impl_ext clo_scan_blelloch_ext;

/* The same for sort implementations (CloSortImplDef keeps upstream's layout,
 * clo_sort_abstract.in.h:43-110).
 *  check_status: after the sort's result has been waited for, fails with
 *    CLO_ERROR_LIBRARY if a kernel of this sorter gave up a bounded spin (the
 *    single-sweep radix passes poll other work-groups). clo_sort_with_host_data
 *    calls it whatever queues the caller passed. */
struct clo_sort;
typedef struct {
	const char* name;
	cl_bool (*check_status)(struct clo_sort* sorter, CCLQueue* cq, GError** err);
	/* host_pipeline: clo_sort_with_host_data with the transfers overlapped with the sort (SURVEY.md
	 * §8f-2). Sets *handled = 0 and touches nothing when this sort is not one it pipelines (the caller
	 * then takes upstream's blocking path, sort/clo_sort_abstract.c:348-395); otherwise *handled = 1
	 * and the return value is the call's. */
	cl_bool (*host_pipeline)(struct clo_sort* sorter, CCLQueue* cq_exec, CCLQueue* cq_comm, const void* data_in, void* data_out,
		size_t numel, int* handled, GError** err);
	/* reserve: grows the sorter's cached buffers for a sort of numel elements on cq_exec NOW. A caller about to
	 * enqueue several sorts of different sizes back to back (the slices of the sharded sort) asks for every size
	 * first: growing a buffer between two of them would free memory the earlier one is still using — hipFree
	 * waits for the device, and the overlap the slices exist for is gone. */
	cl_bool (*reserve)(struct clo_sort* sorter, CCLQueue* cq_exec, size_t numel, GError** err);
	/* sort_segments: `nseg` segments of one device range of `numel` elements, each sorted on its own by the key bits
	 * [key_shift, key_shift + key_bits), in shared launches (clo_hip_radix_sort_segmented, include/clo_hip.h: where the
	 * segments and the optional pieces lie; the result is in b_dev when *result_in_b, else in a_dev; a_dev is overwritten).
	 * *handled = 0 and nothing enqueued when this sorter cannot (another radix than 16 / 256, element size, key kind) —
	 * the caller then sorts the range some other way. reserve_segments grows the buffers it needs for that size NOW. */
	/* (src2_dev / piece_source: pieces that lie in a second device range, clo_hip_radix_sort_segmented2; NULL / NULL: none) */
	CCLEvent* (*sort_segments)(struct clo_sort* sorter, CCLQueue* cq_exec, void* a_dev, void* b_dev, size_t numel,
		const size_t* seg_counts, int nseg, const size_t* piece_counts, const size_t* piece_offsets, const int* piece_segment, int npieces,
		const void* src2_dev, const int* piece_source,
		int key_shift, int key_bits, int* result_in_b, int* handled, GError** err);
	cl_bool (*reserve_segments)(struct clo_sort* sorter, CCLQueue* cq_exec, size_t numel, int nseg, int* handled, GError** err);
	/* sort_by_key: clo_sort_by_key_with_device_data (include/clo_sort.h) once clo_sort_abstract.c has checked what every
	 * by-key sort refuses (the sorter, its element size, a run-time compiled get_key, values_out, numel). NULL: this sorter
	 * has none. values_in / keys_out may be NULL. */
	CCLEvent* (*sort_by_key)(struct clo_sort* sorter, CCLQueue* cq_exec, CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out,
		CCLBuffer* values_out, size_t numel, GError** err);
} clo_sort_impl_ext;
CLO_INTERNAL const clo_sort_impl_ext* clo_sort_impl_ext_find(const char* name);
CLO_INTERNAL extern const clo_sort_impl_ext clo_sort_satradix_ext;

/* Per-kernel events on a profiling queue. Upstream enqueues every kernel itself
 * and names its event (clo_sort_satradix.c:282,295,312; clo_scan_blelloch.c:158,
 * 183,193; clo_sort_sbitonic.c:115), and CCLProf consumers see those names. Here
 * one C-ABI call launches all the kernels of a sort, so while such a call runs
 * the driver has the C-ABI report every launch (clo_hip_set_launch_observer) and
 * opens / closes one CCLEvent per kernel, named through `map` (kernel family ->
 * upstream's event name; families not listed get `other`). Only used when the
 * queue profiles: event pairs between back-to-back kernels cost a few percent. */
typedef struct { const char* label; const char* name; } clo_kname;
typedef struct {
	CCLQueue* cq;
	const clo_kname* map;
	size_t nmap;
	const char* other;
	CCLEvent* open;
	CCLEvent* last;
	int failed;
} clo_kernel_events;
CLO_INTERNAL void clo_kernel_events_install(clo_kernel_events* ke, CCLQueue* cq, const clo_kname* map, size_t nmap, const char* other);
/* Removes the observer; returns the last kernel's event (NULL if there was no
 * launch) and reports a failed event operation through err. */
CLO_INTERNAL CCLEvent* clo_kernel_events_remove(clo_kernel_events* ke, GError** err);

/* Set *err from a clo_hip_* status (domain CCL_HIP_ERROR); returns 1 if st != 0. */
CLO_INTERNAL int clo_hip_failed(int st, GError** err, const char* what);

/* Parse one "key=value" option list the way upstream does
 * (g_strsplit_set on "," then "="; clo_sort_abitonic.c:486-543,
 * clo_sort_satradix.c:366-421). Calls cb(key, value, token, user) per non-empty
 * token; a token without exactly one '=' makes it return 0 and set *bad to a
 * malloc'd copy of the token. cb returns 0 to abort. */
typedef int (*clo_option_cb)(const char* key, const char* value, const char* token, void* user, GError** err);
CLO_INTERNAL int clo_parse_options(const char* options, clo_option_cb cb, void* user, const char* algo, GError** err);

/* ---- The host layer the operation drivers share (clo_op_host.c): clo_histogram.c, clo_reduce_by_key.c,
 * clo_scan_by_key.c, clo_merge.c, clo_search.c, clo_setop.c, clo_select.c and clo_topk.c keep only what is particular
 * to their operation (options, refusals and their wording, size tables, the one thin-ABI call, getters). ---- */

/* 0 unsigned, 1 signed, 2 IEEE total order: the key kinds of clo_sort_by_key_* */
CLO_INTERNAL int clo_type_key_kind(CloType t);
/* int, uint, long or ulong: the value and sum types of the aggregating operations */
CLO_INTERNAL int clo_type_is_int32_or_64(CloType t);
/* The position of name among names[0 .. count), or -1 (for NULL too). */
CLO_INTERNAL int clo_name_index(const char* name, const char* const* names, int count);

/* A range of addresses, of the device or of the host: nothing is dereferenced. A NULL or empty range overlaps nothing. */
typedef struct { const void* p; size_t bytes; } clo_range;
CLO_INTERNAL int clo_ranges_overlap(clo_range a, clo_range b);
/* 0, or why the outputs cannot be written: output by output, CLO_RANGES_OUT_IN when it overlaps an input, else
 * CLO_RANGES_OUT_OUT when it overlaps an earlier output. */
enum { CLO_RANGES_OUT_IN = 1, CLO_RANGES_OUT_OUT = 2 };
CLO_INTERNAL int clo_ranges_conflict(const clo_range* in, int nin, const clo_range* out, int nout);

/* What every operation object starts with (its FIRST member, so that the object's address is the head's). */
typedef struct {
	CCLContext* ctx;
	clo_devbuf workspace;    /* what the operation's clo_hip_*_workspace_bytes asks for; grows, never shrinks */
	clo_stream_guard guard;  /* the workspace belongs to one queue at a time */
} clo_op_head;
/* A zeroed object of `size` bytes holding a reference to ctx, or NULL with CLO_ERROR_LIBRARY; and its end. */
CLO_INTERNAL void* clo_op_new(size_t size, CCLContext* ctx, GError** err);
CLO_INTERNAL void clo_op_destroy(void* op);
/* Before a call on cq that needs ws bytes of workspace: orders the call after the workspace's last user, grows the
 * workspace. `what` names the allocation in the error. 1, or 0 with *err set. */
CLO_INTERNAL int clo_op_reserve(clo_op_head* op, CCLQueue* cq, size_t ws, const char* what, GError** err);

/* p[i]: the device pointer of buf[i], NULL for NULL. */
CLO_INTERNAL void clo_buffers_device_ptrs(CCLBuffer* const* buf, void** p, int n);
/* 1 if every buffer that is not NULL holds need[i] bytes. */
CLO_INTERNAL int clo_buffers_hold(CCLBuffer* const* buf, const size_t* need, int n);
/* Closes the command evt of cq (ccl_queue_begin_command) around the thin-ABI call `what` that returned st: the event,
 * or NULL with *err set and the command taken back. */
CLO_INTERNAL CCLEvent* clo_op_end_command(CCLQueue* cq, CCLEvent* evt, int st, const char* what, GError** err);

/* The device side of a *_with_host_data call: a queue of its own when the caller gave none, one device buffer per
 * slot, blocking transfers on cq_comm. The first failure is kept in `err` and every later step does nothing, so a
 * driver writes the steps one after the other and asks once, at clo_stage_close. In between it makes its device call
 * itself: `if (clo_stage_ok(&st)) st.evt = clo_x_with_device_data(..., st.cq_exec, st.cq_comm, st.dev[..], &st.err);`
 * — the first read-back then waits for st.evt. A slot whose host pointer is NULL or that holds 0 bytes stays NULL.
 * write_name / read_name (NULL after clo_stage_open; the sorts and the scan of clo_sort_abstract.c and
 * clo_scan_abstract.c set them): the uploads / the read-backs are enqueued non-blocking, their events carry that name
 * for a CCLProf consumer, and they are waited for with ccl_event_wait, which also asks the queue's give-up watch. */
#define CLO_STAGE_SLOTS 8
typedef struct {
	CCLContext* ctx;
	CCLQueue* cq_exec;
	CCLQueue* cq_comm;
	CCLQueue* own_queue;     /* made here because the caller passed no cq_exec; destroyed by clo_stage_close */
	CCLBuffer* dev[CLO_STAGE_SLOTS];
	CCLEvent* evt;           /* the device call's event, until the first read has waited for it */
	CCLEventWaitList ewl;
	const char* write_name;
	const char* read_name;
	GError* err;
} clo_stage;
CLO_INTERNAL void clo_stage_open(clo_stage* st, CCLContext* ctx, CCLQueue* cq_exec, CCLQueue* cq_comm);
#define clo_stage_ok(st) ((st)->err == NULL)
CLO_INTERNAL void clo_stage_in(clo_stage* st, int slot, const void* host, size_t bytes);    /* allocates and uploads */
CLO_INTERNAL void clo_stage_out(clo_stage* st, int slot, const void* host, size_t bytes);   /* allocates */
CLO_INTERNAL void clo_stage_read(clo_stage* st, int slot, void* host, size_t bytes);        /* the first bytes of the slot */
/* Moves the failure, if any, to *err; releases the buffers and the queue made here. CL_TRUE if nothing failed. */
CLO_INTERNAL cl_bool clo_stage_close(clo_stage* st, GError** err);

/* ---- What the pipelined host-data paths share (clo_host_pipe.c): scan_with_host_data_pipelined of clo_scan_abstract.c
 * and clo_sort_satradix_host_pipeline of clo_sort_satradix.c keep the arithmetic that says where item k lies. ---- */

/* The copy-out helper. A copy to pageable host memory holds the calling thread for its duration, so the items of a
 * pipeline (the chunks of a scan, the buckets of a sort) go back to the host on a thread of their own. It waits until
 * item k is posted, calls copy(user, k) — which brings item k to the host and returns a clo_hip status — and counts the
 * item completed. The first failure is kept and ends the helper; an item that was never posted is never copied. A
 * zeroed clo_drain is one that was never started. */
typedef struct {
	pthread_t thread;
	pthread_mutex_t mtx;
	pthread_cond_t cv;
	int (*copy)(void* user, size_t k);
	void* user;
	size_t count, posted, completed;   /* items in all / handed to / finished by the helper */
	int device, started, abort, status;
} clo_drain;
#define CLO_DRAIN_START "pthread_create"   /* what a failed clo_drain_start is called in the caller's error */
/* Reads the current device for the helper and creates it: 0 or a clo_hip status. */
CLO_INTERNAL int clo_drain_start(clo_drain* d, size_t count, int (*copy)(void* user, size_t k), void* user);
/* Items 0 .. k - 1 may be copied now. */
CLO_INTERNAL void clo_drain_post(clo_drain* d, size_t k);
/* Returns once k items are completed, or as soon as one has failed: 0, or the first failure's status. */
CLO_INTERNAL int clo_drain_wait(clo_drain* d, size_t k);
/* Ends and joins the helper (items posted by then are still copied). Does nothing after a failed or missing start, or
 * when called again. */
CLO_INTERNAL void clo_drain_stop(clo_drain* d);

/* The runtime calls of one item going out — wait for `ready`, copy `bytes` (if any) on s_out, wait for s_out — and of one
 * chunk coming in: copy on s_in, record `arrived` there, make s_exec wait for it. 0 or a clo_hip status. */
CLO_INTERNAL int clo_pipe_copy_out(void* ready, void* host, const void* dev, size_t bytes, void* s_out);
CLO_INTERNAL int clo_pipe_upload(void* dev, const void* host, size_t bytes, void* s_in, void* arrived, void* s_exec);
/* The stream the chunks come in on: cq_comm's, or `own` when the caller gave one queue for everything. */
CLO_INTERNAL void* clo_pipe_transfer_stream(CCLQueue* cq_comm, void* s_exec, void* own);

#endif
