// clo_hip_rng.hip — CloRng on gfx950: seed initialisation (upstream: rng/clo_rng.c:100-155 + clo_rng_init.cl) and
// the bulk fill (new: clo_rng_fill, include/clo_rng.h). The generators themselves are the device header
// include/clo_rng/clo_rng_device.hpp, whose text clo_hip_rng_device_source() also returns.
//
// Fill: out[i] = f(draw floor(i / S) of state i % S). Each lane loads its state(s) ONCE, makes every draw of it in
// registers and stores it once; upstream's bench kernel sends the state through memory on every draw and needs a
// launch per draw. The stores of one draw are consecutive along the state index, so a wave writes one contiguous
// run per store instruction: 256 B with one state per lane (the library's choice), 1 KiB with four states per lane
// (one 16-byte store each, when S is a multiple of 4 and `out` 16-byte aligned; 15-22 % slower on the MI355X at
// 2^20 states and 2^28 numbers, kept selectable through the thin ABI for measurement).
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "clo_hip.h"
#include "clo_hip_internal.h"
#include "clo_hip_jit_opts.h"
#include "clo_rng/clo_rng_device.hpp"

namespace {

// The header's text, made into a string literal by the Makefile (clo_rng_device_src.inc).
const char k_device_src[] =
#include "clo_rng_device_src.inc"
	;

// Generators in upstream's order (clo_rng.c:60-68); the index is the thin ABI's `gen`.
const char* const k_gen_macro[] = { "CLO_RNG_LCG", "CLO_RNG_XORSHIFT64", "CLO_RNG_XORSHIFT128", "CLO_RNG_MWC64X",
	"CLO_RNG_PARKMILLER", "CLO_RNG_TAUSLCG" };
const int k_ngen = 6;

constexpr int k_threads = 256;

// ---- seeds: seed = gid + main_seed, hashed, converted (clo_rng_init.cl) ----
template <class G, int HASH>
__global__ __launch_bounds__(k_threads) void rng_init_kernel(typename G::state_t* __restrict__ states, size_t count,
	unsigned long long main_seed) {
	const size_t gid = (size_t) blockIdx.x * k_threads + threadIdx.x;
	if (gid >= count) return;
	unsigned long long seed = (unsigned long long) gid + main_seed;
	if (HASH == 1) {
		KNUTH(seed);
	} else if (HASH == 2) {
		XS1(seed);
	}
	states[gid] = G::from_ulong(seed);
}

// The same with the client's hash text compiled in (hiprtc): upstream pastes it as the body of
// #define CLO_RNG_HASH(x) and applies it as the statement CLO_RNG_HASH(seed); (clo_rng.c:100-108).
const char k_init_jit_src[] = R"CLORNGINIT(
extern "C" __global__ void clo_rng_init(clo_statetype* states, unsigned long long count, unsigned long long main_seed) {
	const unsigned long long gid = (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x;
	if (gid >= count) return;
	unsigned long long seed = gid + main_seed;
	CLO_RNG_HASH(seed);
	states[gid] = clo_ulong2statetype(seed);
}
)CLORNGINIT";

template <class G>
int launch_init(void* states, size_t count, unsigned long long main_seed, int hash, hipStream_t s) {
	typedef typename G::state_t T;
	const dim3 grid((unsigned) ((count + k_threads - 1) / k_threads));
	switch (hash) {
		case 0: hipLaunchKernelGGL((rng_init_kernel<G, 0>), grid, dim3(k_threads), 0, s, (T*) states, count, main_seed); break;
		case 1: hipLaunchKernelGGL((rng_init_kernel<G, 1>), grid, dim3(k_threads), 0, s, (T*) states, count, main_seed); break;
		case 2: hipLaunchKernelGGL((rng_init_kernel<G, 2>), grid, dim3(k_threads), 0, s, (T*) states, count, main_seed); break;
		default: return CLO_HIP_EARGS;
	}
	return (int) hipGetLastError();
}

// ---- fill ----
// f: x >> shift (shift = 32 - bits) or, MOD, x % maxint.
template <bool MOD>
__device__ __forceinline__ unsigned rng_out(unsigned x, unsigned shift, unsigned maxint) {
	return MOD ? x % maxint : x >> shift;
}

// One state per lane: state i makes q + (i < r) draws, draw d goes to out[d * S + i].
template <class G, bool MOD>
__global__ __launch_bounds__(k_threads) void rng_fill1_kernel(typename G::state_t* __restrict__ states, size_t S,
	unsigned* __restrict__ out, size_t q, size_t r, unsigned shift, unsigned maxint) {
	const size_t i = (size_t) blockIdx.x * k_threads + threadIdx.x;
	if (i >= S) return;
	const size_t draws = q + (i < r ? 1 : 0);
	if (draws == 0) return;
	typename G::state_t st = states[i];
	unsigned* p = out + i;
#pragma unroll 4
	for (size_t d = 0; d < draws; ++d) {
		*p = rng_out<MOD>(G::next(st), shift, maxint);
		p += S;
	}
	states[i] = st;
}

// Four consecutive states per lane (S % 4 == 0, out 16-byte aligned): every full draw of the four is one 16-byte
// store at out[d * S + 4j]; the last draw, which only the states below r make, is stored element by element.
template <class G, bool MOD>
__global__ __launch_bounds__(k_threads) void rng_fill4_kernel(typename G::state_t* __restrict__ states, size_t S,
	unsigned* __restrict__ out, size_t q, size_t r, unsigned shift, unsigned maxint) {
	const size_t j = (size_t) blockIdx.x * k_threads + threadIdx.x;
	const size_t i0 = 4 * j;
	if (i0 >= S) return;
	if (q == 0 && i0 >= r) return;
	typename G::state_t s0 = states[i0], s1 = states[i0 + 1], s2 = states[i0 + 2], s3 = states[i0 + 3];
	uint4* p = (uint4*) (out + i0);
	const size_t step = S / 4;
#pragma unroll 2
	for (size_t d = 0; d < q; ++d) {
		uint4 v;
		v.x = rng_out<MOD>(G::next(s0), shift, maxint);
		v.y = rng_out<MOD>(G::next(s1), shift, maxint);
		v.z = rng_out<MOD>(G::next(s2), shift, maxint);
		v.w = rng_out<MOD>(G::next(s3), shift, maxint);
		*p = v;
		p += step;
	}
	if (i0 < r) {
		unsigned* t = (unsigned*) p;
		t[0] = rng_out<MOD>(G::next(s0), shift, maxint);
		if (i0 + 1 < r) t[1] = rng_out<MOD>(G::next(s1), shift, maxint);
		if (i0 + 2 < r) t[2] = rng_out<MOD>(G::next(s2), shift, maxint);
		if (i0 + 3 < r) t[3] = rng_out<MOD>(G::next(s3), shift, maxint);
	}
	states[i0] = s0;
	states[i0 + 1] = s1;
	states[i0 + 2] = s2;
	states[i0 + 3] = s3;
}

template <class G, bool MOD>
int launch_fill(void* states, size_t S, unsigned* out, size_t numel, unsigned shift, unsigned maxint, int four, hipStream_t s) {
	typedef typename G::state_t T;
	const size_t q = numel / S, r = numel % S;
	const size_t lanes = four ? S / 4 : S;
	const size_t blocks = (lanes + k_threads - 1) / k_threads;
	if (blocks > 0x7fffffff) return CLO_HIP_EARGS;
	if (four)
		hipLaunchKernelGGL((rng_fill4_kernel<G, MOD>), dim3((unsigned) blocks), dim3(k_threads), 0, s, (T*) states, S, out, q, r, shift, maxint);
	else
		hipLaunchKernelGGL((rng_fill1_kernel<G, MOD>), dim3((unsigned) blocks), dim3(k_threads), 0, s, (T*) states, S, out, q, r, shift, maxint);
	return (int) hipGetLastError();
}

template <class G>
int fill_gen(void* states, size_t S, unsigned* out, size_t numel, unsigned bits, unsigned maxint, int four, hipStream_t s) {
	if (maxint) return launch_fill<G, true>(states, S, out, numel, 0, maxint, four, s);
	return launch_fill<G, false>(states, S, out, numel, 32 - bits, 0, four, s);
}

void set_log(char** log, const std::string& text) {
	if (!log) return;
	*log = (char*) malloc(text.size() + 1);
	if (*log) memcpy(*log, text.c_str(), text.size() + 1);
}

}  // namespace

extern "C" {

const char* clo_hip_rng_device_source(void) { return k_device_src; }

int clo_hip_rng_init(int gen, void* states, size_t count, uint64_t main_seed, int hash, void* stream) {
	if (count == 0) return 0;
	if (!states || (count + k_threads - 1) / k_threads > 0x7fffffff) return CLO_HIP_EARGS;
	hipStream_t s = (hipStream_t) stream;
	clo_timing_scope timing("rng_init", s);
	switch (gen) {
		case 0: return launch_init<clo_rng::lcg>(states, count, main_seed, hash, s);
		case 1: return launch_init<clo_rng::xorshift64>(states, count, main_seed, hash, s);
		case 2: return launch_init<clo_rng::xorshift128>(states, count, main_seed, hash, s);
		case 3: return launch_init<clo_rng::mwc64x>(states, count, main_seed, hash, s);
		case 4: return launch_init<clo_rng::parkmiller>(states, count, main_seed, hash, s);
		case 5: return launch_init<clo_rng::tauslcg>(states, count, main_seed, hash, s);
		default: return CLO_HIP_EARGS;
	}
}

int clo_hip_rng_init_jit(int gen, const char* hash, void* states, size_t count, uint64_t main_seed, void* stream, char** log) {
	if (log) *log = nullptr;
	if (gen < 0 || gen >= k_ngen || !hash || !states || (count + k_threads - 1) / k_threads > 0x7fffffff) return CLO_HIP_EARGS;
	std::string src = std::string("#define ") + k_gen_macro[gen] + " 1\n#define CLO_RNG_HASH(x) " + hash + "\n";
	src += k_device_src;
	src += k_init_jit_src;

	hiprtcProgram prog = nullptr;
	if (hiprtcCreateProgram(&prog, src.c_str(), "clo_rng_init.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
		set_log(log, "hiprtcCreateProgram failed");
		return CLO_HIP_EUNSUPPORTED;
	}
	const std::vector<std::string> optv = clo_jit_options(nullptr);
	std::vector<const char*> opts;
	for (const std::string& o : optv) opts.push_back(o.c_str());
	if (hiprtcCompileProgram(prog, (int) opts.size(), opts.data()) != HIPRTC_SUCCESS) {
		size_t n = 0;
		hiprtcGetProgramLogSize(prog, &n);
		std::string text(n ? n : 1, '\0');
		if (n) hiprtcGetProgramLog(prog, &text[0]);
		set_log(log, text);
		hiprtcDestroyProgram(&prog);
		return CLO_HIP_EARGS;   // the client's hash does not compile
	}
	size_t code_size = 0;
	hiprtcGetCodeSize(prog, &code_size);
	std::vector<char> code(code_size);
	hiprtcGetCode(prog, code.data());
	hiprtcDestroyProgram(&prog);
	if (count == 0) return 0;

	hipModule_t module = nullptr;
	hipFunction_t fn = nullptr;
	hipStream_t s = (hipStream_t) stream;
	hipError_t e = hipModuleLoadData(&module, code.data());
	if (e == hipSuccess) e = hipModuleGetFunction(&fn, module, "clo_rng_init");
	if (e == hipSuccess) {
		unsigned long long n = count, ms = main_seed;
		void* args[] = { &states, &n, &ms };
		clo_timing_scope timing("rng_init", s);
		e = hipModuleLaunchKernel(fn, (unsigned) ((count + k_threads - 1) / k_threads), 1, 1, k_threads, 1, 1, 0, s, args, nullptr);
	}
	// the module goes once its one launch has run (this is clo_rng_new, not the hot path)
	if (e == hipSuccess) e = hipStreamSynchronize(s);
	if (e != hipSuccess) set_log(log, std::string("running the compiled seed kernel failed: ") + hipGetErrorString(e));
	if (module) (void) hipModuleUnload(module);
	return (int) e;
}

int clo_hip_rng_fill(int gen, void* states, size_t count, unsigned* out, size_t numel, unsigned bits, unsigned maxint,
	int layout, void* stream) {
	if (numel == 0) return 0;
	if (!states || !out || count == 0 || bits < 1 || bits > 32) return CLO_HIP_EARGS;
	const int four_ok = count % 4 == 0 && ((uintptr_t) out % 16) == 0;
	if (layout == 4 && !four_ok) return CLO_HIP_EARGS;
	if (layout != 0 && layout != 1 && layout != 4) return CLO_HIP_EARGS;
	const int four = layout == 4;   // the library's choice is one state per lane: measured faster
	hipStream_t s = (hipStream_t) stream;
	clo_timing_scope timing("rng_fill", s);
	switch (gen) {
		case 0: return fill_gen<clo_rng::lcg>(states, count, out, numel, bits, maxint, four, s);
		case 1: return fill_gen<clo_rng::xorshift64>(states, count, out, numel, bits, maxint, four, s);
		case 2: return fill_gen<clo_rng::xorshift128>(states, count, out, numel, bits, maxint, four, s);
		case 3: return fill_gen<clo_rng::mwc64x>(states, count, out, numel, bits, maxint, four, s);
		case 4: return fill_gen<clo_rng::parkmiller>(states, count, out, numel, bits, maxint, four, s);
		case 5: return fill_gen<clo_rng::tauslcg>(states, count, out, numel, bits, maxint, four, s);
		default: return CLO_HIP_EARGS;
	}
}

}  // extern "C"
