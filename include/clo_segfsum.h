/*
 * clo_segfsum.h — CloSegFSum: the floating-point sum of every segment of an array, the segments given by counts or by
 * CSR offsets, REPRODUCIBLE BIT FOR BIT because the order of the additions is part of this contract. NOT upstream (the
 * reference has sort, scan and rng only). Beside CloSegReduce (clo_segreduce.h), which takes integers only: segment
 * sums of features, weights and probabilities, the row sums of a CSR matrix. As there, a segment without a row keeps
 * its output row: sums_out[r] always speaks of segment r.
 *
 * form is one of CLO_SEGREDUCE_FORMS (clo_segreduce.h); count_type is uint or ulong for both forms. The segments are
 * clo_segreduce.h's, word for word: with m_h = numel_seg and m = min(m_h, *num_in) when num_in is given (one cl_ulong
 * of device memory, 8-byte aligned; the host form: a host size_t), else m_h:
 *
 *   form "counts"   counts_or_offsets holds m_h counts c_r. e_r = c_0 + .. + c_r in 64-bit arithmetic, s_r = e_(r-1),
 *                   s_0 = 0, total = e_(m-1), 0 for m = 0. Entries at r >= m are not part of the sum.
 *   form "offsets"  counts_or_offsets holds m_h + 1 offsets, ascending (the precondition); entries [0, m] are read.
 *                   With base = offsets[0]: s_r = offsets[r] - base, e_r = offsets[r + 1] - base, total = offsets[m] -
 *                   base: the offsets are rebased on offsets[0].
 *
 * With n = numel, the rows of values_in, for every r < m:
 *     sums_out[r] = the sum over i in [min(s_r, n), min(e_r, n)) of (sum_type) values_in[i]
 * The ends are clipped at n. Rows r >= m of sums_out (which holds m_h rows) are NOT written. num_out (one cl_ulong of
 * device memory, 8-byte aligned, required) receives total UNCLAMPED. m = 0 writes num_out = 0 and nothing else (the
 * host form returns then without a device).
 *
 * TYPES. value -> sum is one of half -> float, float -> float, float -> double, double -> double. Every row is
 * converted to the sum type by the C cast, which is exact for these four pairs. Every addition is ONE IEEE 754
 * addition in the sum type, round to nearest even, nothing flushed (subnormals are numbers); no fast-math, no
 * reassociation. Every partial sum starts from +0: a segment without a row gets +0, a segment of -0.0 rows sums to +0,
 * and no partial sum is ever -0 — which is why adding +0 for a step that takes no row changes no bit. NaNs and
 * infinities propagate as IEEE addition propagates them; a NaN result is "a NaN", with no promise about its sign or
 * payload.
 *
 * THE ORDER IS THE CONTRACT. The sum of segment r is the value of one fixed expression tree over its rows. The tree is
 * determined by m, n and the clipped ends c_r = min(e_r, n) alone. The result does NOT depend on timing, on the stream,
 * on earlier calls on the object, on the alignment of the arrays, on the form (counts or offsets), on the count type,
 * or on whether num_in is given (for the same m). The result MAY depend on where the segment lies among the other
 * segments and rows: the same rows in a segment that starts elsewhere, or behind other segments, may be added in
 * another order and give other low bits. The fixed order is a property of the whole call, not of one segment.
 * tests/segfsum_model.py restates the tree in numpy, and the GPU is held to it bit for bit. The tree, with the
 * library's constants T = 4352 (clo_hip_segfsum_tile), I = 17 steps per lane, 64 lanes per wave, 4 waves per tile,
 * J = 16 tile states per thread and 4096 tiles per trip of the carry scan:
 *
 *   merge        the m clipped ends are merged with the row indices 0 .. n - 1, an end going first when c_r <= j: m + n
 *                steps. Row j is taken at step j + #{r < m : c_r <= j}; segment r closes at step c_r + r.
 *   tiles, lanes tile t owns the steps [t T, (t + 1) T), lane l of the tile (l < 256) its steps [17 l, 17 l + 17).
 *   first walk   a lane adds the rows of its steps left to right, starting from +0 and starting over from +0 after
 *                every close: its state is (whether it closed, the sum since its last close).
 *   wave         the 64 lane states of a wave go through the segmented network: lanes take the state 1, 2, 4 and 8
 *                lanes below them inside rows of 16 lanes (four steps, each on the results of the step before); then
 *                every lane of rows 1 and 3 takes lane 15 of the row below; then every lane of rows 2 and 3 takes lane
 *                31. Taking a state l from the left into a state r: r.closed ? r.sum : l.sum + r.sum.
 *   waves        the four wave totals are combined left to right, from (no close, +0).
 *   second walk  a lane starts from (the waves before it, left to right) combined with (the lanes below it in its wave:
 *                the network's result one lane down) and adds its rows one by one; at a close the running sum is the
 *                segment's sum as far as this tile knows, and the lane starts over from +0.
 *   carry        the tiles' states (whether a segment closed in the tile, the sum that is open at its end) are scanned
 *                by one work-group in trips of 4096 tiles: a thread combines its 16 states left to right from (no close,
 *                +0); the 64 thread states of a wave go through the same network; the running state of the trips before
 *                comes first, then the four waves left to right; a thread then walks its 16 tiles from (running, waves
 *                before, lanes below). Tile t's carry is the open sum of the tiles before it.
 *   fix-up       the first segment that closes in a tile receives sums_out[r] = sums_out[r] + carry.
 *
 * D(tiles), the largest number of additions any row passes through (those of +0 counted), with tiles =
 * ceil((m + n) / T), I = 17, N = 6 steps of the network, W = 4 waves, J = 16 and trips = ceil(tiles / 4096):
 *     a row whose segment closes in its tile:  I (first walk) + N + (W - 1) (the waves before) + 1 (the lanes below)
 *                                              + (I - 1) (second walk)                                        = 43
 *     a row into its tile's open sum:          I + N + W                                                       = 27
 *     an open sum through the carry scan:      J + N + (W - 1) + 1 + (J - 1) = 41 within one trip; across trips
 *                                              J + N + W into the running state, W in every trip it passes through,
 *                                              (W - 1) + 1 + (J - 1) in the last:   45 + 4 (trips - 2)
 *     the fix-up:                              1
 *     D(tiles) = 43 for tiles <= 1;  27 + 41 + 1 = 69 for trips = 1;  27 + 45 + 4 (trips - 2) + 1 otherwise
 *     (73 from 4097 tiles, 77 from 8193; tests/segfsum_model.py: depth).
 * The classical bound follows: |sum - exact| <= gamma_D * (the sum of |x_i| over the segment), gamma_D = D u /
 * (1 - D u), u = 2^-24 for float and 2^-53 for double sums. (A serial sum of a segment of L rows has D = L - 1.)
 *
 * Refused with CLO_ERROR_ARGS before any device call (err may be NULL, the context may be offline; nothing is written):
 * an unknown form; options other than NULL or ""; an integer value or sum type (that is CloSegReduce); a sum type of
 * half or narrower; a sum type narrower than the value type; half -> double, which is not built; a count_type other
 * than uint or ulong; numel_seg or numel >= 2^32; NULL counts_or_offsets with numel_seg > 0, and in the offsets form
 * always; NULL values_in with numel > 0; NULL sums_out with numel_seg > 0; num_out NULL (device form: misaligned, or
 * below 8 bytes); num_in misaligned or below 8 bytes (device form); a buffer too small (counts_or_offsets for m_h counts
 * or m_h + 1 offsets, values_in for numel rows, sums_out for m_h rows); sums_out or num_out overlapping an input, num_in
 * or each other.
 *
 * Whatever the arrays hold — offsets that do not ascend, sums of counts that wrap 2^64, a *num_in above m_h — every
 * read stays inside the inputs, every write stays inside sums_out[0, m_h) and num_out, and the call completes; the
 * contents are then unspecified.
 *
 * Out of scope: means; float min and max (that is CloSegArg's val_out, clo_segarg.h); half sums;
 * bfloat16; compensated or exact summation; several value columns per call; numel >= 2^32; float aggregates in reduce
 * by key, scan by key and the segmented scan.
 */
#ifndef CLO_SEGFSUM_H
#define CLO_SEGFSUM_H

#include "clo_common.h"
#include "clo_segreduce.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct clo_segfsum CloSegFSum;

/* Works on a context without a device (ccl_context_new_offline). */
CloSegFSum* clo_segfsum_new(const char* form, const char* options, CCLContext* ctx,
	CloType value_type, CloType sum_type, CloType count_type, GError** err);
void clo_segfsum_destroy(CloSegFSum* sf);

/* Asynchronous on cq_exec; never synchronises the device. cq_comm is not used. The object's workspace (the segment
 * ends of the counts form, a few words per tile) belongs to one queue at a time and only grows. */
CCLEvent* clo_segfsum_with_device_data(CloSegFSum* sf, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* counts_or_offsets, CCLBuffer* num_in, CCLBuffer* values_in,
	CCLBuffer* sums_out, CCLBuffer* num_out, size_t numel_seg, size_t numel, GError** err);
/* Blocking: copy in, run, copy the m = min(numel_seg, *num_in) rows of sums_out and total back. cq_exec NULL: a queue
 * of its own; cq_comm NULL: cq_exec. */
cl_bool clo_segfsum_with_host_data(CloSegFSum* sf, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* counts_or_offsets, const size_t* num_in, const void* values_in,
	void* sums_out, size_t* num_out, size_t numel_seg, size_t numel, GError** err);

CCLContext* clo_segfsum_get_context(CloSegFSum* sf);
const char* clo_segfsum_get_form(CloSegFSum* sf);
CloType clo_segfsum_get_value_type(CloSegFSum* sf);
size_t clo_segfsum_get_value_size(CloSegFSum* sf);
CloType clo_segfsum_get_sum_type(CloSegFSum* sf);
size_t clo_segfsum_get_sum_size(CloSegFSum* sf);
CloType clo_segfsum_get_count_type(CloSegFSum* sf);
size_t clo_segfsum_get_count_size(CloSegFSum* sf);

#ifdef __cplusplus
}
#endif
#endif
