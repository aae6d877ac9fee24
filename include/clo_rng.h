/*
 * clo_rng.h — CloRng, device random number generators, as exported by the reference's
 * src/cl_ops/rng/clo_rng.in.h:44-111 (names, values and meaning), implemented over HIP
 * (cl_ops_amd/csrc/clo_rng.c, cl_ops_amd/csrc/hip/clo_hip_rng.hip). Generators: CLO_RNG_IMPLS.
 *
 * Divergences (deliberate):
 *  - clo_rng_get_source() returns HIP C++ (include/clo_rng/clo_rng_device.hpp), not OpenCL C: a client compiles
 *    it in front of its own kernels with hiprtc.
 *  - clo_rng_infos is a macro over clo_rng_get_infos(): `clo_rng_infos[i].name` reads as upstream's, and the
 *    library exports functions only. Its `src` members are the line that selects a generator in front of the
 *    device header's text ("#define CLO_RNG_LCG 1\n", ...).
 *  - clo_rng_fill() is new: the bulk fill, the library's own kernel.
 * An CloRng is not re-entrant: one thread and one queue at a time per object.
 */
#ifndef CLO_RNG_H
#define CLO_RNG_H

#include "clo_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* clo_rng.in.h:45 */
#define CLO_RNG_IMPLS "lcg, xorshift64, xorshift128, mwc64x, parkmiller, tauslcg"

/* clo_rng.in.h:51-62: name, source, seed size in bytes. The list ends with a NULL name. */
struct clo_rng_info {
	const char* name;
	const char* src;
	const size_t seed_size;
};

const struct clo_rng_info* clo_rng_get_infos(void);
#define clo_rng_infos (clo_rng_get_infos())

/* clo_rng.in.h:77-91 */
typedef enum clo_rng_seed_type {
	/* Seeds made on the device from the work-item's global id: hash(gid + main_seed). */
	CLO_RNG_SEED_DEV_GID = 0,
	/* Seeds made on the host by Mersenne Twister (GLib's g_rand_new_with_seed((guint32) main_seed)). */
	CLO_RNG_SEED_HOST_MT = 1,
	/* The client's seeds, already on the device: `seeds` is a CCLBuffer*, which the RNG uses but does not own. */
	CLO_RNG_SEED_EXT_DEV = 2,
	/* The client's seeds, in host memory: copied to the device. */
	CLO_RNG_SEED_EXT_HOST = 3
} CloRngSeedType;

/* clo_rng.c:262-412. type: one of CLO_RNG_IMPLS; hash (DEV_GID only): the body of #define CLO_RNG_HASH(x),
 * applied as the statement CLO_RNG_HASH(seed); NULL or "" = no hash, "KNUTH(x)" and "XS1(x)" the two built in,
 * anything else is compiled at run time. */
CloRng* clo_rng_new(const char* type, CloRngSeedType seed_type, void* seeds, size_t seeds_count, cl_ulong main_seed,
	const char* hash, CCLContext* ctx, CCLQueue* cq, GError** err);
void clo_rng_destroy(CloRng* rng);
const char* clo_rng_get_source(CloRng* rng);
CCLBuffer* clo_rng_get_device_seeds(CloRng* rng);
size_t clo_rng_get_size(CloRng* rng);

/* Not upstream: the bulk fill.
 * out[i] = f(draw floor(i / S) of state i % S), S = seeds_count; f = x >> (32 - bits), or x % maxint when
 * maxint != 0 (bits 1..32 either way). Same values and final states as ceil(numel / S) launches of upstream's
 * clo_rng_bench kernel with global size S (the last one with global size numel % S when that is not 0). Enqueued on
 * cq; returns its event. out holds at least numel uint32 values. */
CCLEvent* clo_rng_fill(CloRng* rng, CCLQueue* cq, CCLBuffer* out, size_t numel, cl_uint bits, cl_uint maxint, GError** err);

#ifdef __cplusplus
}
#endif
#endif
