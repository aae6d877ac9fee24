// clo_rng_device.hpp — the device code of CloRng, HIP C++ (upstream: rng/clo_rng_{workitem,lcg,xorshift64,
// xorshift128,mwc64x,parkmiller,tauslcg,api,init}.cl, OpenCL C).
//
// Written once and used twice: the library's ahead-of-time kernels (cl_ops_amd/csrc/hip/clo_hip_rng.hip) include
// it, and clo_rng_get_source() returns this very text, made into a string when the library is built, behind one
// line that selects the generator (#define CLO_RNG_LCG 1, ... as upstream concatenates one generator's source).
// A client pastes it in front of its own kernels and compiles them with hiprtc, as upstream's clients do with the
// OpenCL JIT. It needs nothing but the HIP built-ins (hiprtc provides them without an #include).
//
// Each generator matches upstream's arithmetic bit for bit, quirks included. One of them: a state of all zeros
// stays all zeros for xorshift64, xorshift128 and parkmiller (for instance xorshift64 seeded from DEV_GID with main
// seed 0 at gid 0), as upstream's do.
#ifndef CLO_RNG_DEVICE_HPP
#define CLO_RNG_DEVICE_HPP

#define CLO_RNG_FN __device__ __forceinline__

namespace clo_rng {

typedef unsigned int u32;
typedef unsigned long long u64;

// Each generator: state_t, from_ulong (upstream's clo_ulong2statetype) and next (one step; returns the output).

// clo_rng_lcg.cl: java.util.Random's 48-bit LCG, output the top 32 of the 48 bits.
struct lcg {
	typedef u64 state_t;
	static CLO_RNG_FN state_t from_ulong(u64 seed) { return seed; }
	static CLO_RNG_FN u32 next(state_t& s) {
		s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
		return (u32) (s >> 16);
	}
};

// clo_rng_xorshift64.cl: output the low 32 bits of the new state.
struct xorshift64 {
	typedef u64 state_t;
	static CLO_RNG_FN state_t from_ulong(u64 seed) { return seed; }
	static CLO_RNG_FN u32 next(state_t& s) {
		s ^= s << 21;
		s ^= s >> 35;
		s ^= s << 4;
		return (u32) s;
	}
};

// clo_rng_xorshift128.cl: Marsaglia's xor128; the seed's words overlap (shifts 0, 16, 32, 46), as upstream's.
struct xorshift128 {
	typedef uint4 state_t;
	static CLO_RNG_FN state_t from_ulong(u64 seed) {
		return make_uint4((u32) seed, (u32) (seed >> 16), (u32) (seed >> 32), (u32) (seed >> 46));
	}
	static CLO_RNG_FN u32 next(state_t& s) {
		const u32 t = s.x ^ (s.x << 11);
		s.x = s.y;
		s.y = s.z;
		s.z = s.w;
		s.w = s.w ^ (s.w >> 19) ^ (t ^ (t >> 8));
		return s.w;
	}
};

// clo_rng_mwc64x.cl: x = low word, c = high word of the seed; the output is taken BEFORE the step.
struct mwc64x {
	typedef uint2 state_t;
	static CLO_RNG_FN state_t from_ulong(u64 seed) { return make_uint2((u32) seed, (u32) (seed >> 32)); }
	static CLO_RNG_FN u32 next(state_t& s) {
		const u32 A = 4294883355U;
		u32 x = s.x, c = s.y;
		const u32 res = x ^ c;
		const u32 hi = (u32) (((u64) x * A) >> 32);   // mul_hi(x, A)
		x = x * A + c;
		c = hi + (x < c);
		s = make_uint2(x, c);
		return res;
	}
};

// clo_rng_parkmiller.cl: s = (long) s * 16807 % 2147483647 with C's truncating remainder, negative states too
// (a seed's low word is taken as it is, so half of all seeds start negative and stay so); output (uint) s << 1.
// The 64-bit signed remainder is computed exactly without a division: |p| < 2^46, and since 2^31 = 1 (mod m),
// |p| = hi * 2^31 + lo leaves hi + lo < 2^31 + 2^15 < 2m, one conditional subtraction from the remainder, which
// then takes p's sign. Exact over the whole int32 domain (tests/test_gpu_rng.py checks all 2^32 states).
struct parkmiller {
	typedef int state_t;
	static CLO_RNG_FN state_t from_ulong(u64 seed) { return (int) (u32) seed; }
	static CLO_RNG_FN u32 next(state_t& s) {
		const long long p = (long long) s * 16807;
		const u64 a = (u64) (p < 0 ? -p : p);
		u64 r = (a & 0x7FFFFFFFULL) + (a >> 31);
		r = r >= 0x7FFFFFFFULL ? r - 0x7FFFFFFFULL : r;
		s = p < 0 ? -(int) r : (int) r;
		return (u32) s << 1;
	}
};

// clo_rng_tauslcg.cl: three Tausworthe steps and an LCG, the components rotating one place per step; the seed is
// (lo, hi, lo, hi); the output is the new x.
struct tauslcg {
	typedef uint4 state_t;
	static CLO_RNG_FN state_t from_ulong(u64 seed) {
		return make_uint4((u32) seed, (u32) (seed >> 32), (u32) seed, (u32) (seed >> 32));
	}
	static CLO_RNG_FN u32 taus_step(u32 z, int s1, int s2, int s3, u32 m) {
		const u32 b = ((z << s1) ^ z) >> s2;
		return ((z & m) << s3) ^ b;
	}
	static CLO_RNG_FN u32 next(state_t& s) {
		const u32 x = s.x;
		s.x = taus_step(s.y, 13, 19, 12, 4294967294U);
		s.y = taus_step(s.z, 2, 25, 4, 4294967288U);
		s.z = taus_step(s.w, 3, 11, 17, 4294967294U);
		s.w = 1664525U * x + 1013904223U;
		return s.x;
	}
};

}  // namespace clo_rng

// Seed hashes of the DEV_GID seed type (clo_rng_init.cl): statements on an unsigned 64-bit variable, named in
// clo_rng_new's `hash` as "KNUTH(x)" / "XS1(x)".
#define KNUTH(x) x = ((x * 2654435761ULL) % 0x100000000ULL)
#define XS1(x) \
	x = ((x >> 16) ^ x) * 0x45d9f3b; \
	x = ((x >> 16) ^ x) * 0x45d9f3b; \
	x = ((x >> 16) ^ x);

// ---- upstream's device API for one generator, chosen by the line in front of this text ----
#if defined(CLO_RNG_LCG)
typedef clo_rng::lcg clo_rng_impl;
#elif defined(CLO_RNG_XORSHIFT64)
typedef clo_rng::xorshift64 clo_rng_impl;
#elif defined(CLO_RNG_XORSHIFT128)
typedef clo_rng::xorshift128 clo_rng_impl;
#elif defined(CLO_RNG_MWC64X)
typedef clo_rng::mwc64x clo_rng_impl;
#elif defined(CLO_RNG_PARKMILLER)
typedef clo_rng::parkmiller clo_rng_impl;
#elif defined(CLO_RNG_TAUSLCG)
typedef clo_rng::tauslcg clo_rng_impl;
#endif

#if defined(CLO_RNG_LCG) || defined(CLO_RNG_XORSHIFT64) || defined(CLO_RNG_XORSHIFT128) || \
	defined(CLO_RNG_MWC64X) || defined(CLO_RNG_PARKMILLER) || defined(CLO_RNG_TAUSLCG)

typedef clo_rng_impl::state_t clo_statetype;

#define clo_ulong2statetype(seed) (clo_rng_impl::from_ulong(seed))

// clo_rng_workitem.cl. The global size is the grid's thread count, gridDim.x * blockDim.x.
#define GLOBAL_SIZE() ((unsigned int) (gridDim.x * blockDim.x))
#define GID1() ((unsigned int) (blockIdx.x * blockDim.x + threadIdx.x))
#define GID2() make_uint2(GID1(), GLOBAL_SIZE() + GID1())
#define GID4() make_uint4(GID1(), GLOBAL_SIZE() + GID1(), GLOBAL_SIZE() * 2 + GID1(), GLOBAL_SIZE() * 3 + GID1())
#define GID8() clo_uint8_make(GID1(), GLOBAL_SIZE())

// OpenCL's uint8 (HIP has no 8-wide vector type); s[k] is upstream's .sk.
struct clo_uint8 {
	unsigned int s[8];
};
CLO_RNG_FN clo_uint8 clo_uint8_make(unsigned int gid, unsigned int gsize) {
	clo_uint8 r;
	for (int k = 0; k < 8; ++k) r.s[k] = gsize * k + gid;
	return r;
}

// One step of the state at `index`, through memory as upstream's (the library's own fill keeps states in
// registers instead).
CLO_RNG_FN unsigned int clo_rng_next(clo_statetype* states, unsigned int index) {
	clo_statetype s = states[index];
	const unsigned int r = clo_rng_impl::next(s);
	states[index] = s;
	return r;
}

// clo_rng_api.cl: random integers from 0 to n - 1, from the states GID1 / GID2 / GID4 / GID8 name.
CLO_RNG_FN unsigned int clo_rng_next_int(clo_statetype* states, unsigned int n) {
	return clo_rng_next(states, GID1()) % n;
}
CLO_RNG_FN uint2 clo_rng_next_int2(clo_statetype* states, unsigned int n) {
	const uint2 i = GID2();
	const unsigned int a = clo_rng_next(states, i.x) % n;
	const unsigned int b = clo_rng_next(states, i.y) % n;
	return make_uint2(a, b);
}
CLO_RNG_FN uint4 clo_rng_next_int4(clo_statetype* states, unsigned int n) {
	const uint4 i = GID4();
	const unsigned int a = clo_rng_next(states, i.x) % n;
	const unsigned int b = clo_rng_next(states, i.y) % n;
	const unsigned int c = clo_rng_next(states, i.z) % n;
	const unsigned int d = clo_rng_next(states, i.w) % n;
	return make_uint4(a, b, c, d);
}
CLO_RNG_FN clo_uint8 clo_rng_next_int8(clo_statetype* states, unsigned int n) {
	const clo_uint8 i = GID8();
	clo_uint8 r;
	for (int k = 0; k < 8; ++k) r.s[k] = clo_rng_next(states, i.s[k]) % n;
	return r;
}

#endif  // a generator is selected

#endif  // CLO_RNG_DEVICE_HPP
