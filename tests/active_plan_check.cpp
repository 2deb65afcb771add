// Host-side check of plan_active (cpu-path-tracing_amd/csrc/launch_plan.hpp),
// the plan of an adaptive pass, built and run on the CPU by
// tests/test_adaptive_host.py with AddressSanitizer/UBSan.  For unit counts 0,
// 1 and large, every add_samples in [1, 65536] and several chunk_samples, for
// the linear and the BVH kernel:
//   * every chunk is in [1, kMaxChunk] (divmod_nv's exact range) and
//     chunk_samples is honoured where it is within add_samples and kMaxChunk;
//   * decoded as gather_kernel decodes them (unit = units * c + u, local
//     samples [c * chunk, min(add, (c + 1) * chunk))), units x chunks cover
//     every sample of every unit exactly once and no chunk is empty;
//   * n_units = units * n_chunks and the grid = ceil(n_units / waves per
//     workgroup), computed in 64 bits: a plan past 2^31 - 1 workgroups is
//     refused, not truncated.
// Then it prints the layout of the adaptive structs of include/ptgpu.h, which
// the test compares with the ctypes mirrors.  Exits non-zero on a violation.
#include <cinttypes>
#include <cstddef>
#include <cstdio>

#include "../cpu-path-tracing_amd/csrc/kernel_args.hpp"
#include "../cpu-path-tracing_amd/csrc/launch_plan.hpp"

static int fails = 0;
#define CHECK(c, ...)                                                                              \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            std::fprintf(stderr, "units %lld add %d chunk_samples %d bvh %d: ", units, add, cs, (int)bvh); \
            std::fprintf(stderr, __VA_ARGS__);                                                     \
            std::fprintf(stderr, "\n");                                                            \
            ++fails;                                                                               \
            return;                                                                                \
        }                                                                                          \
    } while (0)

static long long refused = 0, planned = 0;

static void check(bool bvh, int wave_slots, long long units, int add, int cs)
{
    ActivePlan P;
    const int rc = plan_active(bvh, wave_slots, units, add, cs, P);
    const int wpb = (bvh ? PTG_BVH_BLOCK : kBlock) / 64;
    if (units <= 0 || add <= 0) {
        CHECK(rc == PTG_OK && P.grid == 0 && P.n_units == 0 && P.n_chunks == 0, "an empty plan launches nothing");
        return;
    }
    CHECK(P.chunk >= 1 && P.chunk <= kMaxChunk && P.chunk <= add, "chunk %d", P.chunk);
    if (cs > 0)
        CHECK(P.chunk == (cs < add ? (cs < kMaxChunk ? cs : kMaxChunk) : add), "chunk_samples not honoured: %d", P.chunk);
    // the chunks cover [0, add) exactly once, none empty
    CHECK((long long)(P.n_chunks - 1) * P.chunk < add && (long long)P.n_chunks * P.chunk >= add, "n_chunks %d of %d",
          P.n_chunks, P.chunk);
    long long covered = 0;
    for (int c : {0, P.n_chunks / 2, P.n_chunks - 1}) {  // as the kernel forms them
        const long long s0 = (long long)c * P.chunk;
        long long cnt = add - s0;
        cnt = cnt < P.chunk ? cnt : P.chunk;
        CHECK(s0 < add && cnt >= 1 && cnt <= P.chunk, "chunk %d: s0 %lld cnt %lld", c, s0, cnt);
    }
    covered = (long long)(P.n_chunks - 1) * P.chunk + (add - (long long)(P.n_chunks - 1) * P.chunk);
    CHECK(covered == add, "covered %lld", covered);
    const long long want_units = units * (long long)P.n_chunks;
    const long long want_grid = (want_units + wpb - 1) / wpb;
    if (want_grid > 0x7FFFFFFFLL) {
        CHECK(rc == PTG_ERR_UNSUPPORTED && P.grid == 0, "a grid of %lld workgroups must be refused (rc %d grid %d)",
              want_grid, rc, P.grid);
        ++refused;
        return;
    }
    CHECK(rc == PTG_OK, "rc %d", rc);
    CHECK(P.n_units == want_units && (long long)P.grid == want_grid, "n_units %lld grid %d", P.n_units, P.grid);
    // unit -> (chunk, list unit) and back, at the ends of the grid
    for (long long unit : {0LL, want_units / 2, want_units - 1}) {
        const long long c = unit / units, u = unit - c * units;
        CHECK(c >= 0 && c < P.n_chunks && u >= 0 && u < units && c * units + u == unit, "unit %lld -> chunk %lld unit %lld",
              unit, c, u);
    }
    CHECK((long long)P.grid * wpb >= want_units && ((long long)P.grid - 1) * wpb < want_units, "grid %d", P.grid);
    ++planned;
}

int main()
{
    const int wave_slots = 256 * 32;
    for (int bvh = 0; bvh < 2; ++bvh)
        for (long long units : {0LL, 1LL, 7LL, 129600LL, 1LL << 28})
            for (int cs : {0, 1, 3, 100000})
                for (int add = 1; add <= 65536; ++add)
                    check(bvh != 0, wave_slots, units, add, cs);
    for (int bvh = 0; bvh < 2; ++bvh) {
        check(bvh != 0, wave_slots, 5, 0, 0);
        check(bvh != 0, wave_slots, 129600, 1 << 30, 0);  // the largest add: chunks of kMaxChunk
        check(bvh != 0, wave_slots, 1LL << 28, 1 << 30, 1);
    }
    std::printf("plans ok %lld, refused (too many work units) %lld, failures %d\n", planned, refused, fails);
    std::printf("ptg_adaptive_target size %zu rel_error %zu floor %zu max_fraction %zu min_samples %zu dilate %zu\n",
                sizeof(ptg_adaptive_target), offsetof(ptg_adaptive_target, rel_error), offsetof(ptg_adaptive_target, floor),
                offsetof(ptg_adaptive_target, max_fraction), offsetof(ptg_adaptive_target, min_samples),
                offsetof(ptg_adaptive_target, dilate));
    std::printf("ptg_adaptive_report size %zu passes %zu converged %zu max_samples %zu pixels %zu pixels_over %zu "
                "max_rho %zu mean_rho %zu total_samples %zu counters %zu pass_added %zu pass_over %zu pass_active %zu\n",
                sizeof(ptg_adaptive_report), offsetof(ptg_adaptive_report, passes), offsetof(ptg_adaptive_report, converged),
                offsetof(ptg_adaptive_report, max_samples), offsetof(ptg_adaptive_report, pixels),
                offsetof(ptg_adaptive_report, pixels_over), offsetof(ptg_adaptive_report, max_rho),
                offsetof(ptg_adaptive_report, mean_rho), offsetof(ptg_adaptive_report, total_samples),
                offsetof(ptg_adaptive_report, counters), offsetof(ptg_adaptive_report, pass_added),
                offsetof(ptg_adaptive_report, pass_over), offsetof(ptg_adaptive_report, pass_active));
    return fails ? 1 : 0;
}
