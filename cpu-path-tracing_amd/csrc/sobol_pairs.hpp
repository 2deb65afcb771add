// sobol_pairs.hpp -- PTG_FLAG_STRATIFIED's sampler (include/ptgpu.h
// "Stratified sampling"): pairs of 24-bit integers from an Owen-scrambled,
// index-shuffled Sobol' (0,2)-sequence in a path's sample index.
//
// Integer arithmetic on uint32 throughout (the seed mix is 64-bit), the same
// on host and device: the render kernels, the reference-arithmetic mode
// (ref64.hpp), ptg_sampler_pairs_device and the host check
// (tests/sobol_check.cpp) all include this file.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTG_SOBOL_HD __host__ __device__ inline
#else
#define PTG_SOBOL_HD inline
#endif

namespace ptg {
namespace sobol {

constexpr int kPairs = 4;  // 0 sub-pixel jitter, 1 lens, 2 first diffuse bounce, 3 first light sample

#if defined(__has_builtin)
#if __has_builtin(__builtin_bitreverse32)
#define PTG_SOBOL_HAS_BITREVERSE 1
#endif
#endif

PTG_SOBOL_HD uint32_t brev(uint32_t x)
{
#ifdef PTG_SOBOL_HAS_BITREVERSE
    return __builtin_bitreverse32(x);  // device: v_bfrev_b32
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// Laine-Karras style hash: every output bit depends only on the input bits
// below it, so brev(lk(brev(v), seed)) is a nested uniform (Owen) scramble of v
PTG_SOBOL_HD uint32_t lk(uint32_t x, uint32_t seed)
{
    x += seed;
    x ^= x * 0x6c50b47cu;
    x ^= x * 0xb82f1e52u;
    x ^= x * 0xc7afe638u;
    x ^= x * 0x8d22f6e6u;
    return x;
}

// brev of the second Sobol' dimension of index i (direction numbers
// v = 1 << 31; v ^= v >> 1 per index bit): a prefix xor over the index bits
PTG_SOBOL_HD uint32_t P(uint32_t i)
{
    i ^= (i >> 1) & 0x55555555u;
    i ^= (i >> 2) & 0x33333333u;
    i ^= (i >> 4) & 0x0F0F0F0Fu;
    i ^= (i >> 8) & 0x00FF00FFu;
    i ^= (i >> 16) & 0x0000FFFFu;
    return i;
}

// splitmix64's finaliser (pt_device.hpp mix64: the same function)
PTG_SOBOL_HD uint64_t seed_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The three seeds of pair j of a sub-pixel, key = key_hash(seed, pixel_sub):
// they depend on (sub-pixel, pair) only, never on the sample
struct Seeds {
    uint32_t sa, sb, sc;
};
PTG_SOBOL_HD Seeds seeds_of(uint64_t key, int j)
{
    const uint64_t h = seed_mix64(key ^ ((uint64_t)(j + 1) * 0xD1B54A32D192ED03ull));
    return Seeds{(uint32_t)(h >> 32), (uint32_t)h, (uint32_t)(seed_mix64(h) >> 32)};
}

// Pair j of sample s from brs = brev(s) (shared by a sample's pairs): two
// 24-bit integers m, used where a draw_bits() result is: u = m 2^-24
PTG_SOBOL_HD void pair_brev(const Seeds sd, uint32_t brs, uint32_t &m0, uint32_t &m1)
{
    const uint32_t i = brev(lk(brs, sd.sa));  // the shuffled index
    m0 = brev(lk(i, sd.sb)) >> 8;             // van der Corput, scrambled
    m1 = brev(lk(P(i), sd.sc)) >> 8;          // Sobol' dimension 2, scrambled
}
PTG_SOBOL_HD void pair(const Seeds sd, uint32_t s, uint32_t &m0, uint32_t &m1) { pair_brev(sd, brev(s), m0, m1); }

}  // namespace sobol
}  // namespace ptg
