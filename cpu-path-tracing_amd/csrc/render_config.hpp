// render_config.hpp -- the render kernels' compile-time tunables, each with
// the measurement that set its value, and the debug-statistics switches with
// their macros.  Included by ptg_render.hip inside its unnamed namespace,
// first of the device headers; needs kLinearMax (kernel_args.hpp).  Owns
// PTG_MAX_LDS_SPHERES, PTG_REFILL_BATCH, PTG_LEAF_FRAC, PTG_LEAF_SPLIT,
// PTG_LONG_LEAF, PTG_BVH_STACK, PTG_READY_FRAC, PTG_MIN_WAVES_PER_EU and the
// debug builds' PTG_BLOCK_STATS, PTG_UNIT_TRACE and PTG_WAVE_STATS (their
// device arrays are read by ptg_render.hip's ptg_debug_stats_ /
// ptg_unit_trace_).
#pragma once

#ifndef PTG_MAX_LDS_SPHERES
#define PTG_MAX_LDS_SPHERES 64
#endif
// scenes up to 64 spheres keep geometry (32 B) and shading (64 B) records in
// dynamically sized LDS: box_scene needs 17.4 KB + 768 B per workgroup, so 8
// workgroups fit a CU (measured: shading in LDS +1.3 % over geometry-only
// staging, which itself beat scalar loads by 1.5 %)
constexpr int kMaxLdsSpheres = PTG_MAX_LDS_SPHERES;
static_assert(kLinearMax <= kMaxLdsSpheres, "linear scenes must fit in LDS");
#ifndef PTG_REFILL_BATCH
#define PTG_REFILL_BATCH 40  // measured: 40 beats 32 by 0.35 % (box) / 0.6 % (box_mirror), ties 48-56; 24 is 1.2 % slower
#endif
#ifndef PTG_LEAF_FRAC
#define PTG_LEAF_FRAC 4  // BVH: leaf phase once 4/8 of the walking lanes hold a leaf (re-swept after the walk clean-up: 4 and 3 beat 5 by 0.6 %, 6 +1.5 %)
#endif
#ifndef PTG_LEAF_SPLIT
#define PTG_LEAF_SPLIT 2  // BVH leaf phase: lanes without a leaf test part of another lane's leaf (1: one helper per leaf, 2: up to two)
#endif
#ifndef PTG_LONG_LEAF
#define PTG_LONG_LEAF 5  // BVH leaf phase: leaves of at least this many spheres get helpers first (and a second one; 5 beats 4 by 0.9 %, 3 and 6 worse)
#endif
#ifndef PTG_BVH_STACK
#define PTG_BVH_STACK 3  // wide walk: per-lane stack entries before the continuation fallback (3: C5 -0.7 % vs 2, A/B 258.3 vs 260.1 ms)
#endif
#ifndef PTG_READY_FRAC
#define PTG_READY_FRAC 6  // BVH: stop walking and shade once 6/8 of the active lanes have finished their scan
                          // (measured with octant layouts + SAH: 6 beats 4 by 7 %, 5 and 7 by 1-2 %)
#endif
#ifndef PTG_BLOCK_STATS
#define PTG_BLOCK_STATS 0  // debug builds only: wave-level execution counts of the linear kernel's blocks (ptg_dbg_stats)
#endif
#if PTG_BLOCK_STATS
// [0] main-loop iterations, [1] scans, [2] small-sphere root parts, [3] extra box-mode walls,
// [4] diffuse/dielectric blocks, [5] mirror blocks, [6] refill batches, [7] small-sphere pre-tests
__device__ unsigned long long ptg_dbg_stats[256 * 16];
// PTG_BLOCK_STATS == 3: wave cycles inside the linear kernel's refill batch --
// [0] batches, [1] flush + park of finished paths, [2] camera rays (ray_of),
// [3] begin / store_pre
__device__ unsigned long long ptg_dbg_stats2[256 * 16];
#define PTG_SUB_T(var) const unsigned long long var = clock64()
#define PTG_SUB_ADD(i, v)                                                                              \
    do {                                                                                               \
        if (__lane_id() == __ffsll((long long)__ballot(1)) - 1)                                        \
            atomicAdd(&ptg_dbg_stats2[(blockIdx.x & 255) * 16 + (i)], (v));                           \
    } while (0)
#define PTG_STAT(i)                                                                                    \
    do {                                                                                               \
        if (__lane_id() == __ffsll((long long)__ballot(1)) - 1)                                        \
            atomicAdd(&ptg_dbg_stats[(blockIdx.x & 255) * 16 + (i)], 1ull);                            \
    } while (0)
// BVH kernel, PTG_BLOCK_STATS=2: wave cycles (s_memtime) per phase of the
// main loop in [8..13]: scan starts, node steps, leaf phases, shading,
// refills, loop control
#if PTG_BLOCK_STATS == 2
#define PTG_PHASE(i)                                                                                   \
    do {                                                                                               \
        if constexpr (kBvh) {                                                                          \
            const unsigned long long t_ = clock64();                                                   \
            ph_cyc[i] += t_ - ph_t;                                                                    \
            ph_t = t_;                                                                                 \
        }                                                                                              \
    } while (0)
#else
#define PTG_PHASE(i) ((void)0)
#endif
#else
#define PTG_STAT(i) ((void)0)
#define PTG_PHASE(i) ((void)0)
#endif
#ifndef PTG_UNIT_TRACE
#define PTG_UNIT_TRACE 0  // debug builds only: per-unit start / end wall clock and hardware id (tools/unit_trace.py)
#endif
#if PTG_UNIT_TRACE
constexpr int kTraceUnits = 1 << 19;
// unit u: [3u] start, [3u + 1] end (s_memrealtime, 100 MHz), [3u + 2] XCC id << 32 | HW_ID
__device__ unsigned long long ptg_unit_trace[3 * kTraceUnits];
#define PTG_TRACE_END()                                                                                \
    do {                                                                                               \
        if (__lane_id() == 0 && unit < kTraceUnits) {                                                  \
            ptg_unit_trace[3 * unit] = trace_t0;                                                       \
            ptg_unit_trace[3 * unit + 1] = wall_clock64();                                             \
            ptg_unit_trace[3 * unit + 2] = ((unsigned long long)__builtin_amdgcn_s_getreg(0xF814) << 32) | \
                                           (unsigned long long)__builtin_amdgcn_s_getreg(0xF804);     \
        }                                                                                              \
    } while (0)
#else
#define PTG_TRACE_END() ((void)0)
#endif
#ifndef PTG_WAVE_STATS
#define PTG_WAVE_STATS 0  // debug builds only: count wave-level BVH iterations instead of per-lane tests
#endif
#ifndef PTG_MIN_WAVES_PER_EU
#define PTG_MIN_WAVES_PER_EU 8  // 8 waves per SIMD: <= 64 VGPRs and <= 80 SGPRs (8 blocks of 256 per CU)
#endif
