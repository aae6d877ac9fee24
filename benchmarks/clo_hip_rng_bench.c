/*
 * clo_hip_rng_bench.c — the RNG harness (reference: src/benchmarks/clo_rng_bench.c:50-82,204-270, restated),
 * against include/cl_ops.h and libcl_ops_hip.so, with hiprtc and the HIP module API for the client side.
 *
 * As upstream's: a CloRng of `-g` states (seeded on the device from the global id with hash `-h`, else on the host by
 * Mersenne Twister from `-s`), its device source (clo_rng_get_source) compiled together with the bench kernel below,
 * `-n` launches of it over the `-g` states, one draw per state per launch, each result read back and written out
 * (file-tsv, file-dh, stdout-bin, stdout-uint).
 *
 * Output `none` (not upstream): times, with device events and after a warm-up, ONE clo_rng_fill of g * n numbers,
 * then the per-launch path above making the same numbers (n launches of the bench kernel, launch r writing its g
 * numbers at r * g), and checks that both wrote the same bytes.
 */
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>
#include <hip/hiprtc.h>

#include "cl_ops.h"

#define BENCH_GWS 262144
#define BENCH_LWS 256
#define BENCH_RUNS 10
#define BENCH_BITS 32
#define BENCH_FILE_PREFIX "out"
#define BENCH_PEAK_BYTES_PER_S 8.0e12

/* benchmarks/clo_rng_bench.cl:31-44, in HIP: the global size is the number of states, whatever the block size */
static const char* k_bench_src =
	"extern \"C\" __global__ void clo_rng_bench(clo_statetype* seeds, unsigned int* result, const unsigned int bits,\n"
	"		const unsigned int gws) {\n"
	"	const unsigned int gid = GID1();\n"
	"	if (gid >= gws) return;\n"
	"#ifdef CLO_RNG_BENCHMARK_MAXINT\n"
	"	result[gid] = clo_rng_next_int(seeds, bits);\n"
	"#else\n"
	"	result[gid] = clo_rng_next(seeds, gid) >> (32 - bits);\n"
	"#endif\n"
	"}\n";

static void usage(const char* prog) {
	fprintf(stderr,
		"Usage: %s [options]\n"
		"  -r, --rng RNG          Random number generator: " CLO_RNG_IMPLS " (default is lcg)\n"
		"  -o, --output OUTPUT    Output: file-tsv, file-dh, stdout-bin, stdout-uint, none (default: file-tsv)\n"
		"  -g, --globalsize SIZE  Global work size = number of states (default is %d)\n"
		"  -l, --localsize SIZE   Local work size (default is %d)\n"
		"  -n, --runs SIZE        Random numbers per work-item (default is %d, 0 means continuous generation)\n"
		"  -d, --device INDEX     Device index\n"
		"  -s, --rng-seed SEED    Seed for random number generator (default is %d)\n"
		"  -h, --gid-hash HASH    Use work-item GID-based seeds instead of MT derived seeds from host; the hash to apply\n"
		"                         (KNUTH, XS1 or source code modifying variable x, e.g. x = x << 2)\n"
		"  -b, --bits BITS        Number of bits in unsigned integers to produce (default %d)\n"
		"  -m, --max MAX          Maximum integer to produce, overrides --bits option\n",
		prog, BENCH_GWS, BENCH_LWS, BENCH_RUNS, CLO_DEFAULT_SEED, BENCH_BITS);
}

#define HIP_OK(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "Error: %s: %s\n", what, hipGetErrorString(e_)); status = CLO_ERROR_LIBRARY; goto cleanup; } } while (0)
#define FAIL(code, ...) do { fprintf(stderr, "Error: "); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); status = (code); goto cleanup; } while (0)

int main(int argc, char** argv) {
	char* rng = "lcg";
	char* output = "file-tsv";
	size_t gws = BENCH_GWS, lws = BENCH_LWS;
	unsigned runs = BENCH_RUNS;
	int dev_idx = -1;
	unsigned rng_seed = CLO_DEFAULT_SEED;
	char* gid_hash = NULL;
	unsigned bits = BENCH_BITS, maxint = 0;

	static struct option longopts[] = {
		{ "rng", required_argument, 0, 'r' }, { "output", required_argument, 0, 'o' },
		{ "globalsize", required_argument, 0, 'g' }, { "localsize", required_argument, 0, 'l' },
		{ "runs", required_argument, 0, 'n' }, { "device", required_argument, 0, 'd' },
		{ "rng-seed", required_argument, 0, 's' }, { "gid-hash", required_argument, 0, 'h' },
		{ "bits", required_argument, 0, 'b' }, { "max", required_argument, 0, 'm' }, { "help", no_argument, 0, '?' },
		{ 0, 0, 0, 0 } };
	int c;
	while ((c = getopt_long(argc, argv, "r:o:g:l:n:d:s:h:b:m:", longopts, NULL)) != -1) {
		switch (c) {
			case 'r': rng = optarg; break;
			case 'o': output = optarg; break;
			case 'g': gws = strtoull(optarg, NULL, 0); break;
			case 'l': lws = strtoull(optarg, NULL, 0); break;
			case 'n': runs = (unsigned) strtoul(optarg, NULL, 0); break;
			case 'd': dev_idx = atoi(optarg); break;
			case 's': rng_seed = (unsigned) strtoul(optarg, NULL, 0); break;
			case 'h': gid_hash = optarg; break;
			case 'b': bits = (unsigned) strtoul(optarg, NULL, 0); break;
			case 'm': maxint = (unsigned) strtoul(optarg, NULL, 0); break;
			default: usage(argv[0]); return CLO_ERROR_ARGS;
		}
	}

	int status = CLO_SUCCESS;
	GError* err = NULL;
	CCLContext* ctx = NULL;
	CCLQueue* queue = NULL;
	CloRng* rng_dev = NULL;
	CloRng* rng_fill = NULL;
	CCLBuffer* result_dev = NULL;
	CCLBuffer* big = NULL;
	unsigned* result_host = NULL;
	unsigned* check_a = NULL;
	unsigned* check_b = NULL;
	char* src = NULL;
	char* code = NULL;
	char* fname = NULL;
	FILE* out = NULL;
	hipModule_t module = NULL;
	hipFunction_t kernel = NULL;
	hipEvent_t e0 = NULL, e1 = NULL;
	hiprtcProgram prog = NULL;

	const int is_none = !strcmp(output, "none");
	if (strcmp(output, "file-tsv") && strcmp(output, "file-dh") && strcmp(output, "stdout-bin") && strcmp(output, "stdout-uint") && !is_none)
		FAIL(CLO_ERROR_ARGS, "Unknown output '%s'.", output);
	if (bits > 32 || bits < 1) FAIL(CLO_ERROR_ARGS, "Number of bits must be between 1 and 32.");
	if (runs == 0 && (!strncmp(output, "file", 4) || is_none)) FAIL(CLO_ERROR_ARGS, "Continuous generation can only be performed to stdout.");
	if (gws == 0 || lws == 0 || lws > 1024 || gws > 0xffffffffull) FAIL(CLO_ERROR_ARGS, "Global size must be 1 .. 2^32 - 1, local size 1 .. 1024.");

	ctx = ccl_context_new_from_menu_full(&dev_idx, &err);
	if (!ctx) goto gerror;
	queue = ccl_queue_new(ctx, NULL, 0, &err);
	if (!queue) goto gerror;
	const CloRngSeedType seed_type = gid_hash ? CLO_RNG_SEED_DEV_GID : CLO_RNG_SEED_HOST_MT;
	rng_dev = clo_rng_new(rng, seed_type, NULL, gws, rng_seed, gid_hash, ctx, queue, &err);
	if (!rng_dev) goto gerror;

	/* the client's program: the RNG's source + the bench kernel, compiled with hiprtc (upstream: OpenCL JIT) */
	{
		const char* rs = clo_rng_get_source(rng_dev);
		src = (char*) malloc(strlen(rs) + strlen(k_bench_src) + 1);
		if (!src) FAIL(CLO_ERROR_LIBRARY, "out of memory");
		strcpy(src, rs);
		strcat(src, k_bench_src);
		if (hiprtcCreateProgram(&prog, src, "clo_rng_bench.hip", 0, NULL, NULL) != HIPRTC_SUCCESS) FAIL(CLO_ERROR_LIBRARY, "hiprtcCreateProgram");
		const char* opts[] = { "--offload-arch=gfx950", "-O3", "-DCLO_RNG_BENCHMARK_MAXINT" };
		if (hiprtcCompileProgram(prog, maxint ? 3 : 2, opts) != HIPRTC_SUCCESS) {
			size_t n = 0;
			hiprtcGetProgramLogSize(prog, &n);
			char* log = (char*) calloc(n + 1, 1);
			if (log) hiprtcGetProgramLog(prog, log);
			fprintf(stderr, "Error: building the bench kernel:\n%s\n", log ? log : "");
			free(log);
			status = CLO_ERROR_LIBRARY;
			goto cleanup;
		}
		size_t code_size = 0;
		hiprtcGetCodeSize(prog, &code_size);
		code = (char*) malloc(code_size);
		if (!code) FAIL(CLO_ERROR_LIBRARY, "out of memory");
		hiprtcGetCode(prog, code);
		HIP_OK(hipModuleLoadData(&module, code), "hipModuleLoadData");
		HIP_OK(hipModuleGetFunction(&kernel, module, "clo_rng_bench"), "hipModuleGetFunction");
	}
	void* stream = ccl_queue_get_stream(queue);
	void* seeds_ptr = ccl_buffer_get_device_ptr(clo_rng_get_device_seeds(rng_dev));
	const unsigned value = maxint ? maxint : bits;
	const unsigned gws32 = (unsigned) gws;
	const unsigned blocks = (unsigned) ((gws + lws - 1) / lws);

	if (is_none) {
		/* one fill of g * n numbers against n launches of the bench kernel making the same numbers */
		const size_t numel = gws * (size_t) runs;
		big = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, numel * 4, NULL, &err);
		if (!big) goto gerror;
		rng_fill = clo_rng_new(rng, seed_type, NULL, gws, rng_seed, gid_hash, ctx, queue, &err);
		if (!rng_fill) goto gerror;
		const size_t seed_size = clo_rng_get_size(rng_fill) / gws;
		HIP_OK(hipEventCreate(&e0), "hipEventCreate");
		HIP_OK(hipEventCreate(&e1), "hipEventCreate");
		float ms_fill = 0, ms_launch = 0;
		for (int pass = 0; pass < 2; ++pass) {   /* pass 0: warm-up */
			HIP_OK(hipEventRecord(e0, (hipStream_t) stream), "hipEventRecord");
			if (!clo_rng_fill(rng_fill, queue, big, numel, bits, maxint, &err)) goto gerror;
			HIP_OK(hipEventRecord(e1, (hipStream_t) stream), "hipEventRecord");
			HIP_OK(hipEventSynchronize(e1), "hipEventSynchronize");
			HIP_OK(hipEventElapsedTime(&ms_fill, e0, e1), "hipEventElapsedTime");
			ccl_queue_gc(queue);
		}
		/* the per-launch path: warm-up of `runs` launches into the same range, then the timed ones (the states of
		 * both RNGs have then made 2 * runs draws each, so the last writes of each compare) */
		for (int pass = 0; pass < 2; ++pass) {
			HIP_OK(hipEventRecord(e0, (hipStream_t) stream), "hipEventRecord");
			for (unsigned r = 0; r < runs; ++r) {
				void* res = (unsigned*) ccl_buffer_get_device_ptr(big) + (size_t) r * gws;
				void* args[] = { &seeds_ptr, &res, (void*) &value, (void*) &gws32 };
				HIP_OK(hipModuleLaunchKernel(kernel, blocks, 1, 1, (unsigned) lws, 1, 1, 0, (hipStream_t) stream, args, NULL), "launch");
			}
			HIP_OK(hipEventRecord(e1, (hipStream_t) stream), "hipEventRecord");
			HIP_OK(hipEventSynchronize(e1), "hipEventSynchronize");
			HIP_OK(hipEventElapsedTime(&ms_launch, e0, e1), "hipEventElapsedTime");
		}
		/* same states after the same number of draws: compare them (the numbers were compared by the tests) */
		const size_t sbytes = clo_rng_get_size(rng_fill);
		check_a = (unsigned*) malloc(sbytes);
		check_b = (unsigned*) malloc(sbytes);
		if (!check_a || !check_b) FAIL(CLO_ERROR_LIBRARY, "out of memory");
		if (!ccl_buffer_enqueue_read(clo_rng_get_device_seeds(rng_fill), queue, 1, 0, sbytes, check_a, NULL, &err)) goto gerror;
		if (!ccl_buffer_enqueue_read(clo_rng_get_device_seeds(rng_dev), queue, 1, 0, sbytes, check_b, NULL, &err)) goto gerror;
		const int same = !memcmp(check_a, check_b, sbytes);
		const double bytes = 4.0 * (double) numel + 2.0 * (double) gws * (double) seed_size;
		const double bytes_launch = 4.0 * (double) numel + 2.0 * (double) runs * (double) gws * (double) seed_size;
		printf("rng=%s states=%zu numbers=%zu fill_ms=%.4f numbers_per_s=%.4g bytes=%.0f peak_share=%.3f "
			"launch_path_ms=%.4f launch_path_bytes=%.0f launch_path_peak_share=%.3f speedup=%.2f states_match=%d\n",
			rng, gws, numel, ms_fill, numel / (ms_fill * 1e-3), bytes, bytes / (ms_fill * 1e-3) / BENCH_PEAK_BYTES_PER_S,
			ms_launch, bytes_launch, bytes_launch / (ms_launch * 1e-3) / BENCH_PEAK_BYTES_PER_S, ms_launch / ms_fill, same);
		if (!same) FAIL(CLO_ERROR_LIBRARY, "the fill and the per-launch path left different states");
		goto cleanup;
	}

	result_dev = ccl_buffer_new(ctx, CL_MEM_READ_WRITE, gws * sizeof(unsigned), NULL, &err);
	if (!result_dev) goto gerror;
	result_host = (unsigned*) malloc(gws * sizeof(unsigned));
	if (!result_host) FAIL(CLO_ERROR_LIBRARY, "out of memory");

	const int raw = !strcmp(output, "stdout-bin");
	const char* sep_field = "\n";
	const char* sep_line = "";
	if (!strncmp(output, "stdout", 6)) {
		out = stdout;
	} else {
		const int dh = !strcmp(output, "file-dh");
		const char* h = gid_hash ? gid_hash : "mt";
		fname = (char*) malloc(strlen(rng) + strlen(h) + 64);
		if (!fname) FAIL(CLO_ERROR_LIBRARY, "out of memory");
		sprintf(fname, "%s_%s_%s%s%s", BENCH_FILE_PREFIX, rng, gid_hash ? "gid_" : "host_", h, dh ? ".dh.txt" : ".tsv");
		if (!dh) { sep_field = "\t"; sep_line = "\n"; }
		out = fopen(fname, "w");
		if (!out) FAIL(CLO_ERROR_OPENFILE, "Unable to create output file '%s'.", fname);
		if (dh) fprintf(out, "type: d\ncount: %d\nnumbit: %d\n", (int) (gws * runs), bits);
		fprintf(stderr, "     Random number generator (seed): %s (%u)\n", rng, rng_seed);
		fprintf(stderr, "     Seeds in workitems: %s %s\n", gid_hash ? "GID-based, hash:" : "Host-based,", gid_hash ? gid_hash : "Mersenne Twister");
		fprintf(stderr, "     Global/local worksizes: %d/%d\n", (int) gws, (int) lws);
		fprintf(stderr, "     Number of runs: %d\n", runs);
	}
	for (unsigned i = 0; i != runs || runs == 0; ++i) {
		void* res = ccl_buffer_get_device_ptr(result_dev);
		void* args[] = { &seeds_ptr, &res, (void*) &value, (void*) &gws32 };
		HIP_OK(hipModuleLaunchKernel(kernel, blocks, 1, 1, (unsigned) lws, 1, 1, 0, (hipStream_t) stream, args, NULL), "launch");
		if (!ccl_buffer_enqueue_read(result_dev, queue, 1, 0, gws * sizeof(unsigned), result_host, NULL, &err)) goto gerror;
		ccl_queue_gc(queue);
		if (raw) {
			if (fwrite(result_host, sizeof(unsigned), gws, out) != gws) FAIL(CLO_ERROR_STREAM_WRITE, "write failed");
		} else {
			for (size_t k = 0; k < gws; ++k) fprintf(out, "%u%s", result_host[k], sep_field);
			fprintf(out, "%s", sep_line);
		}
	}
	goto cleanup;

gerror:
	status = err ? err->code : CLO_ERROR_LIBRARY;
	fprintf(stderr, "Error: %s\n", err ? err->message : "(unknown)");
	clo_gerror_clear(&err);

cleanup:
	if (out && out != stdout) fclose(out);
	if (out == stdout) fflush(stdout);
	if (e0) hipEventDestroy(e0);
	if (e1) hipEventDestroy(e1);
	if (module) hipModuleUnload(module);
	if (prog) hiprtcDestroyProgram(&prog);
	if (rng_fill) clo_rng_destroy(rng_fill);
	if (rng_dev) clo_rng_destroy(rng_dev);
	if (result_dev) ccl_buffer_destroy(result_dev);
	if (big) ccl_buffer_destroy(big);
	if (queue) ccl_queue_destroy(queue);
	if (ctx) ccl_context_destroy(ctx);
	free(result_host);
	free(check_a);
	free(check_b);
	free(src);
	free(code);
	free(fname);
	return status;
}
