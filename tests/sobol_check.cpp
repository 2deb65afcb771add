// sobol_check.cpp -- host check of csrc/sobol_pairs.hpp, PTG_FLAG_STRATIFIED's
// sampler (tests/test_sobol_pairs.py builds and runs it, once plainly and once
// with -fsanitize=address,undefined).
//
//  1. P(i) is the bit reversal of the second Sobol' dimension of i, formed
//     here bit by bit from its direction numbers (v = 1 << 31; v ^= v >> 1
//     per index bit): every i < 2^16 and 2^16 scattered 32-bit values.
//  2. The scrambled, shuffled pairs are a (0,2)-sequence: for m = 1..8 every
//     aligned block of 2^m samples has exactly one point in each elementary
//     interval 2^-a x 2^-(m-a), a = 0..m -- 64 keys, all four pair numbers,
//     samples [0, 1024) and the 1024 samples from 2^20 on.
//  3. Pairs of different pair numbers for the same samples differ: every two
//     of the four pair numbers, in m0 and in m1.
// Then "vec seed pixel_sub pair sample m0 m1" lines, which tests/strat_ref.py's
// numpy restatement must reproduce.  Exit status 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../cpu-path-tracing_amd/csrc/sobol_pairs.hpp"

using namespace ptg::sobol;

static uint64_t key_hash(uint64_t seed, uint64_t pixel_sub) { return seed_mix64(seed ^ seed_mix64(pixel_sub + 1ull)); }

static uint32_t sobol_dim2(uint32_t i)
{
    uint32_t v = 1u << 31, r = 0;
    for (int b = 0; b < 32; ++b) {
        if ((i >> b) & 1u)
            r ^= v;
        v ^= v >> 1;
    }
    return r;
}

int main()
{
    long bad_p = 0, bad_cell = 0, bad_range = 0, same = 0, blocks = 0;
    for (uint32_t k = 0; k < (1u << 17); ++k) {
        const uint32_t i = k < (1u << 16) ? k : (k * 2654435761u) ^ (k << 13);
        if (P(i) != brev(sobol_dim2(i)))
            ++bad_p;
    }
    std::vector<uint32_t> m0(1024), m1(1024);
    std::vector<uint32_t> all0[kPairs], all1[kPairs];  // the pairs of the pair numbers before j, same key and samples
    std::vector<int> seen;
    for (int kk = 0; kk < 64; ++kk) {
        const uint64_t key = key_hash(12345ull + (uint64_t)(kk / 8), (uint64_t)kk * 977ull);
        for (int base = 0; base < 2; ++base) {
            const uint32_t s0 = base ? 1u << 20 : 0u;
            for (int j = 0; j < kPairs; ++j) {
                const Seeds sd = seeds_of(key, j);
                for (uint32_t s = 0; s < 1024; ++s) {
                    pair(sd, s0 + s, m0[s], m1[s]);
                    if ((m0[s] | m1[s]) >> 24)
                        ++bad_range;
                }
                for (int i = 0; i < j; ++i) {  // against every earlier pair number, m0 and m1
                    long eq0 = 0, eq1 = 0;
                    for (uint32_t s = 0; s < 1024; ++s) {
                        eq0 += m0[s] == all0[i][s];
                        eq1 += m1[s] == all1[i][s];
                    }
                    same += (eq0 > 2) + (eq1 > 2);  // (24-bit values: equal by chance about 6e-5 of the time)
                }
                all0[j] = m0;
                all1[j] = m1;
                for (int m = 1; m <= 8; ++m)
                    for (uint32_t b = 0; b < 1024; b += 1u << m)
                        for (int a = 0; a <= m; ++a) {
                            ++blocks;
                            seen.assign((size_t)1 << m, 0);
                            for (uint32_t s = b; s < b + (1u << m); ++s) {
                                const uint32_t cx = a ? m0[s] >> (24 - a) : 0u;
                                const uint32_t cy = m - a ? m1[s] >> (24 - (m - a)) : 0u;
                                seen[(cx << (m - a)) | cy] += 1;
                            }
                            for (int c : seen)
                                bad_cell += c != 1;
                        }
            }
        }
    }
    std::printf("P_mismatches %ld cells_off %ld out_of_range %ld equal_pairs %ld blocks %ld\n", bad_p, bad_cell, bad_range,
                same, blocks);
    const uint64_t seeds[2] = {1ull, 0x9E3779B97F4A7C15ull};
    const uint64_t subs[3] = {0ull, 5ull, 123456789ull};
    const uint32_t samples[6] = {0u, 1u, 2u, 7u, 1000u, 0x12345678u};
    for (uint64_t seed : seeds)
        for (uint64_t ps : subs)
            for (int j = 0; j < kPairs; ++j)
                for (uint32_t s : samples) {
                    uint32_t a, b;
                    pair(seeds_of(key_hash(seed, ps), j), s, a, b);
                    std::printf("vec %llu %llu %d %u %u %u\n", (unsigned long long)seed, (unsigned long long)ps, j, s, a, b);
                }
    return (bad_p || bad_cell || bad_range || same) ? 1 : 0;
}
