// ptg_render.hip -- the MI355X render-loop megakernel and its C ABI (include/ptgpu.h).
//
// Replaces the reference's per-pixel hot path (src/main.cpp:214-236 and
// below).  Mapping onto CDNA4:
//  * one lane per (pixel, sub-pixel): lanes 4p..4p+3 of a wave are the
//    2x2 sub-pixels of pixel p (main.cpp:226-232), 16 pixels per wave64;
//  * each lane runs its `samples` paths back to back in ONE flat loop whose
//    iteration is one bounce segment: a lane whose path ends (miss, Russian
//    roulette, depth cap) accumulates it and immediately starts its next
//    sample (per-lane path regeneration), so the wave keeps ~all lanes busy
//    despite the geometric path-length tail;
//  * sphere geometry records are staged in LDS once per workgroup and read
//    with uniform-address (broadcast) LDS loads in the scan (up to 256
//    spheres; measured 1.5 % faster than scalar loads, 7 % faster than
//    software-prefetched scalar loads); larger scenes use wave-uniform scalar
//    loads (s_load into SGPRs) from L2/HBM;
//  * per-wave segment counts via ballot popcount, one atomic per wave;
//  * sub-pixel combine by in-register cross-lane reads, then coalesced
//    192-B stores (three lanes of each pixel write R, G, B).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ptgpu.h"
#include "bvh_build.hpp"
#include "frame_passes.hpp"  // add_image: the ADD into the caller's image
#include "kernel_args.hpp"  // KArgs and the constants shared with the host side
#include "launch_plan.hpp"  // check_params, fill_launch and their tunables
#include "pt_device.hpp"
#include "ptg_error.hpp"
#include "ref64.hpp"
#include "scene_prep.hpp"  // scene records, scan order, box mode, the uploads
#include "sobol_pairs.hpp"  // PTG_FLAG_STRATIFIED: the scrambled Sobol' pairs

using namespace ptg;

namespace {

#define PTG_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(PTG_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)

constexpr int kTraceBlock = 256;  // parity probe kernel
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
template <bool kBvh>
constexpr int kBlockOf = kBvh ? PTG_BVH_BLOCK : kBlock;
struct Lane {
    int x, y, sx, sy;
    uint64_t key;
};

// camera constants as 4 float4: {pos, lens}, {base, sub_len}, {X, 1/W},
// {Y, 1/H}.  The render kernel stages them in LDS and reads them in each
// refill (camera_ray runs only there): kept in registers for the whole unit
// they took 16 VGPRs, half of them spilled to scratch (measured).
struct CamC {
    float4 p, b, X, Y;
};

__host__ __device__ inline CamC cam_of(const KArgs &A)
{
    return CamC{make_float4(A.pos_x, A.pos_y, A.pos_z, A.lens), make_float4(A.base_x, A.base_y, A.base_z, A.sub_len),
                make_float4(A.X_x, A.X_y, A.X_z, A.invW), make_float4(A.Y_x, A.Y_y, A.Y_z, A.invH)};
}

// kStrat (PTG_FLAG_STRATIFIED): the jitter is pair 0 and the lens disk's first
// try pair 1 of the sample (cq = {pair 0, pair 1}); neither advances the
// xorshift state, which the retries and everything after draw from.
template <bool kStrat = false>
__device__ __forceinline__ void camera_ray(const CamC &C, const Lane &L, uint32_t sample, uint32_t &st, f3 &o,
                                           f3 &d, [[maybe_unused]] const uint4 cq = uint4{})
{
    st = sample_state(L.key, sample);
    // main.cpp:186-190: jitter inside the sub-pixel cell
    float u1, u2;
    if constexpr (kStrat) {
        u1 = (float)cq.x * 0x1p-24f;
        u2 = (float)cq.y * 0x1p-24f;
    } else {
        u1 = draw(st);
        u2 = draw(st);
    }
    float xin = __builtin_fmaf(C.b.w, u1, (float)L.x + (float)L.sx * C.b.w);
    float yin = __builtin_fmaf(C.b.w, u2, (float)L.y + (float)L.sy * C.b.w);
    float fs = xin * C.X.w;  // main.cpp:190 x/W as x * (1/W)
    float ft = yin * C.Y.w;
    // camera.cpp:19-30: rejection sample of the unit disk (2 draws per try)
    float px, py;
    if constexpr (kStrat) {
        px = __builtin_fmaf(2.0f, (float)cq.z * 0x1p-24f, -1.0f);
        py = __builtin_fmaf(2.0f, (float)cq.w * 0x1p-24f, -1.0f);
        while (__builtin_fmaf(py, py, px * px) >= 1.0f) {
            px = __builtin_fmaf(2.0f, draw(st), -1.0f);
            py = __builtin_fmaf(2.0f, draw(st), -1.0f);
        }
    } else
    do {
        px = __builtin_fmaf(2.0f, draw(st), -1.0f);
        py = __builtin_fmaf(2.0f, draw(st), -1.0f);
    } while (__builtin_fmaf(py, py, px * px) >= 1.0f);
    // camera.cpp:34-37 (offset = rd*s + rd*t, the reference's lens quirk)
    float sst = fs + ft;
    float ox = (px * C.p.w) * sst;
    float oy = (py * C.p.w) * sst;
    o = mk3(C.p.x + ox, C.p.y + oy, C.p.z);
    d = mk3(__builtin_fmaf(C.Y.x, ft, __builtin_fmaf(C.X.x, fs, C.b.x)) - ox,
            __builtin_fmaf(C.Y.y, ft, __builtin_fmaf(C.X.y, fs, C.b.y)) - oy,
            __builtin_fmaf(C.Y.z, ft, __builtin_fmaf(C.X.z, fs, C.b.z)));
}

// main.cpp:30-42 + sphere.cpp:6-30: closest root >= eps over all spheres,
// strict < so the first record in scan order wins exact ties.  Sphere records
// are read from LDS at wave-uniform addresses (broadcast reads).
// Scan order groups the records by kind (host: prepare_scan_order), so every
// loop below runs one straight-line test: huge spheres whose anchor normal is
// a coordinate axis (the box walls) need e_k and d_k instead of two dot
// products (-6 VALU per wall); the oracle's generic form gives the same bits
// (a dot product with +-e_k is exactly +-x_k).
// Roots: with qq = sq + |hb| they are c/-qq (hb >= 0) or c/qq (near) and
// qq/a (far) (hb < 0); the far root matters only when the near one is < eps.
// Roots stay fractions num/den (den > 0): "root < eps" is num < eps*den,
// "nearer" is num*bq < bn*den, and one division per segment turns the winner
// into t.  The test is straight-line code (selects, no per-lane branches):
// the oracle's two culls (hb >= 0 && c >= 0; near root provably not nearer,
// DESIGN.md "scene scan") are exact early-outs that never let a wave skip the
// sqrt in practice, so they are left out here (-15 % frame time, same bits).
constexpr float kCullMargin = 0x1.00001p+0f;  // 1 + 2^-20 (BVH leaf test)
constexpr float kPlaneMargin = 0x1.ffep-1f;    // 1 - 2^-12: box mode's wall skip test

enum : int { kAxX = 0, kAxY = 1, kAxZ = 2, kBig = 3, kSmall = 4, kAxAny = 5, kAxSel = 6, kAxAnyOut = 7 };

__device__ __forceinline__ float comp(f3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// Returns the winner's record, or the sentinel recs + n (no hit).
// Tests a scan executed (counting kernels only).  BVH scenes: sphere tests
// (huge + leaf spheres) and box tests of the walk; linear scenes: sphere
// tests executed (walls + small spheres, each lane's own -- box mode tests
// one wall for most rays, not all of them) and, of those, the wall tests.
struct ScanCount {
    uint32_t spheres = 0, boxes = 0;
};

template <bool kExact, bool kCount = false>
__device__ __forceinline__ const LinRec *scene_scan(const KArgs &A, const LinRec *recs, f3 o, f3 d, float &tbest,
                                                   ScanCount &cnt)
{
    // the nearest root is kept as a fraction bn/bq (bq > 0); candidates are
    // compared by cross-multiplication, only the winner is divided
    float a = dot3(d, d);
    float bn = kInf, bq = 1.0f;
    // the winner as a byte offset from the sentinel (0: the sentinel, no
    // hit): no multiply by the record size per segment
    constexpr int kRecB = (int)sizeof(LinRec);
    int bi = 0;
    auto ri_of = [&](const LinRec *r) { return ((int)(r - recs) - A.n) * kRecB; };
    // r: the record's index relative to the sentinel
    auto test_geo = [&](const auto r, const float4 g0, const float4 g1, auto kind_tag, const float un = 0.0f,
                        const float vn = 0.0f, const bool valid = true, const int ks = 0) {
        constexpr int kKind = decltype(kind_tag)::value;
        if constexpr (kCount) {
            cnt.spheres += valid ? 1u : 0u;
            if constexpr (kKind != kSmall)
                cnt.boxes += valid ? 1u : 0u;  // (linear scenes: the wall tests)
        }
        // r is wave-uniform, except for a pair's walls / box mode
        f3 e = mk3(o.x - g0.x, o.y - g0.y, o.z - g0.z);
        float ed = dot3(e, d);
        float ee = dot3(e, e);
        float hb, c;
        if constexpr (kKind <= kAxZ) {  // huge sphere anchored on axis k: g0.w = +-R, g1.w = +-2R
            hb = __builtin_fmaf(g0.w, comp(d, kKind), ed);
            c = __builtin_fmaf(g1.w, comp(e, kKind), ee);
        } else if constexpr (kKind == kAxAny || kKind == kAxAnyOut) {
            // the same, for the wall the ray moves toward on a per-lane axis
            // k: g0.w d_k = -R |d_k| = -|g0.w| vn and g1.w e_k = 2R u = |g1.w| un
            // (un: the plane distance numerator, the same subtraction as e_k
            // up to sign), the products' bits are unchanged
            hb = __builtin_fmaf(-__builtin_fabsf(g0.w), vn, ed);
            c = __builtin_fmaf(__builtin_fabsf(g1.w), un, ee);
        } else if constexpr (kKind == kAxSel) {
            // the same as kAxX..kAxZ for a per-lane axis ks (box mode's extra
            // walls).  Exact cull: with hb >= 0 the only candidate root is
            // -c / qq, qq = sq + hb >= hb, so -c < eps hb (or c >= 0) means
            // it fails "num < eps den" below -- the common case here, a lane
            // that just left this convex wall; the wave skips the root when
            // every lane is culled
            hb = __builtin_fmaf(g0.w, comp(d, ks), ed);
            c = __builtin_fmaf(g1.w, comp(e, ks), ee);
            const bool live = valid & !((hb >= 0.0f) & ((c >= 0.0f) | (-c < kEps * hb)));
#if PTG_BLOCK_STATS == 1  // [13] lanes with an extra wall in a pass, [14] of them not culled, [15] passes not skipped
            {
                const unsigned long long mv = __ballot(valid), ml = __ballot(live);
                if (__lane_id() == __ffsll((long long)__ballot(1)) - 1) {
                    unsigned long long *st = &ptg_dbg_stats[(blockIdx.x & 255) * 16];
                    atomicAdd(st + 13, (unsigned long long)__popcll(mv));
                    atomicAdd(st + 14, (unsigned long long)__popcll(ml));
                    atomicAdd(st + 15, ml ? 1ull : 0ull);
                }
            }
#endif
            if (__ballot(live) == 0ull)
                return;
        } else if constexpr (kKind == kBig) {  // general anchored form
            hb = __builtin_fmaf(g0.w, dot3(mk3(g1.x, g1.y, g1.z), d), ed);
            c = __builtin_fmaf(g1.w, dot3(e, mk3(g1.x, g1.y, g1.z)), ee);
        } else {
            hb = ed;
            // fast mode: -R^2 folded into the first product of e.e (one add
            // fewer; another rounding order of the same sum)
            if constexpr (!kExact)
                c = __builtin_fmaf(e.z, e.z, __builtin_fmaf(e.y, e.y, __builtin_fmaf(e.x, e.x, g0.w)));
            else
            c = ee + g0.w;  // g0.w = g1.w = -R^2
        }
        float disc;
        if constexpr (kKind == kSmall) {
            // Lagrange's identity: hb^2 - a c = a R^2 - |e x d|^2.  hb^2 - a c
            // cancels to ~1e-3 relative for a sphere of radius r at distance
            // D >> r (two terms of size a D^2 for a difference of size a r^2);
            // this form keeps the rounding at the scale of a r^2 (DESIGN.md
            // "error budget": box_mirror 1920x1080x1024 RMSE vs fp64 1.9e-3 ->
            // 5e-5).  Huge spheres keep hb^2 - a c: there the anchored hb, c
            // are accurate and a R^2 would be ~1e12.
            const f3 x = cross3(e, d);
            disc = __builtin_fmaf(a, -g0.w, -dot3(x, x));
        } else {
            disc = __builtin_fmaf(hb, hb, -(a * c));
        }
        // a small sphere no lane's ray line meets cannot win: the wave skips
        // the root (exact: "win" below requires disc >= 0)
        if constexpr (kKind == kSmall) {
            PTG_STAT(7);
            if (__ballot(!(disc < 0.0f)) == 0ull)
                return;
            PTG_STAT(2);
        }
        // disc < 0 is rejected below whatever sq is: no clamp
        const float sq = Math<kExact>::sqrt(disc);
        const bool neg = hb < 0.0f;
        // sq - hb (hb < 0) and hb + sq (hb >= 0) are the same IEEE add
        const float qq = sq + __builtin_fabsf(hb);
        float num, den;
        if constexpr (kKind == kAxAnyOut) {
            // a box wall, origin outside it (box_walls_out): the near root
            // c/qq (hb < 0) or nothing (hb >= 0: -c/qq <= 0 fails the eps
            // test; `win` below requires hb < 0).  The far root qq/a -- the
            // wall sphere's other side, ~2R away -- is dropped: the
            // reference takes it only for an origin within eps of the wall
            // moving toward it (a surface touching the wall); the bench
            // frame's quality rows are unchanged up to single roundings
            // (profiles/r04_kernel_ab.txt 13).  The same for the small
            // spheres moved paths there (item 12): not done.
            num = c;
            den = qq;
        } else {
            const bool near_lt = c < kEps * qq;
            num = neg ? (near_lt ? qq : c) : -c;
            den = (neg & near_lt) ? a : qq;
        }
        // one eps test covers all three cases (for the near root it repeats
        // near_lt, which is false there)
        bool win = valid & (!kExact || !(disc < 0.0f)) & !(num < kEps * den) &
                   (num * bq < bn * den);
        if constexpr (kKind == kAxAnyOut)
            win = win & neg;
        bn = win ? num : bn;
        bq = win ? den : bq;
        bi = win ? r : bi;
    };
    auto test_rec = [&](const LinRec *r, auto kind_tag, const float un = 0.0f, const float vn = 0.0f,
                        const bool valid = true, const int ks = 0) {
        test_geo(ri_of(r), r->g.g0, r->g.g1, kind_tag, un, vn, valid, ks);
    };
    auto test = [&](const int i, auto kind_tag) { test_rec(recs + i, kind_tag); };
    // scan order: axis-anchored walls (x, y, z), general huge spheres, small
    // spheres (host: prepare_scan_order)
    int i = 0;
    // a wall pair: the + wall at i, the - wall at i + 1.  A ray whose origin
    // is on the room side of both walls' tangent planes (within a margin) can
    // only hit the wall it moves toward (DESIGN.md "wall pairs"); other lanes
    // (origins outside the room, rare) test both, the one moved toward first
    auto axis_group = [&](auto kind_tag) {
        constexpr int k = decltype(kind_tag)::value;
        if (A.pairs[k]) {
            const bool pos = comp(d, k) >= 0.0f;
            test(pos ? i : i + 1, kind_tag);
            const float ok = comp(o, k);
            const bool outside = !(ok >= A.pair_lo[k]) | !(ok <= A.pair_hi[k]);
            if (__ballot(outside) != 0ull) {
                if (outside)
                    test(pos ? i + 1 : i, kind_tag);
            }
            i += 2;
        }
        for (; i < A.end_ax[k]; ++i)
            test(i, kind_tag);
    };
#ifndef PTG_ASSUME_BOX_MODE
#define PTG_ASSUME_BOX_MODE 0  // analysis builds only (tools/isa_breakdown.py): box mode on, the other scan compiled out
#endif
    // the first small sphere's geometry (the records after the huge ones;
    // always in bounds: the sentinel follows the last record)
    const float4 pf_g0 = recs[A.end_big].g.g0, pf_g1 = recs[A.end_big].g.g1;
    const float4 pf2_g0 = recs[A.end_big + 1].g.g0;  // (in bounds: the sentinel and the wall table follow)
    const float4 pf3_g0 = recs[A.end_big + 2].g.g0;  // (all three read at the start)
    // the small spheres [i, n) (i = n after)
    auto small_spheres = [&](int &i) {
        // three small spheres (the box scenes): straight-line code on one LDS
        // base address (the records at constant offsets), no loop control
        if (A.n - i == 3) {
            // the three records' geometry read at the scan's start (pf_g0,
            // pf2_g0, pf3_g0: their LDS latency behind the walls' tests)
            test_geo(-3 * kRecB, pf_g0, pf_g1, std::integral_constant<int, kSmall>{});
            const float4 a2 = pf3_g0;
            test_geo(-2 * kRecB, pf2_g0, pf_g1, std::integral_constant<int, kSmall>{});
            test_geo(-1 * kRecB, a2, pf_g1, std::integral_constant<int, kSmall>{});
            i = A.n;
        }
        for (; i < A.n; ++i)
            test(i, std::integral_constant<int, kSmall>{});
    };
    if (PTG_ASSUME_BOX_MODE || A.box_mode) {
        // Box mode (DESIGN.md "box mode"): per axis the wall the ray moves
        // toward and the distance u/v to its tangent plane; the wall of the
        // nearest plane is tested first.  Every wall lies beyond its tangent
        // plane, so another wall can only win if its plane is nearer than the
        // winner's root (checked with a 2^-12 margin, far above the roots'
        // rounding): those walls are tested only where that check fails
        // (rare: rays hitting near an edge); a wall the ray moves away from
        // only from beyond its tangent plane (below).
        // wall table after the sentinel: byte offsets of the records of axis
        // k's + wall (2k) and - wall (2k + 1), -1 where missing
        [[maybe_unused]] const int *walls = reinterpret_cast<const int *>(recs + A.n + 1);
        float u[3], v[3];
        bool posk[3];
        float umin = 0.0f;  // the smallest of the six plane distances (room bound check below)
        for (int k = 0; k < 3; ++k) {
            // the uniform plane / record values stay in SGPRs: select values,
            // not kernel-argument addresses (that became per-lane loads)
            float pp = A.plane_plus[k], pm = A.plane_minus[k];
            asm volatile("" : "+s"(pp), "+s"(pm));
            const float dk = comp(d, k);
            const bool pos = dk >= 0.0f;

            // (o - pm) is the same IEEE subtraction as -(pm - o).  A missing
            // wall's plane is at +-inf: u = inf is never the nearest (inf * v
            // is inf or NaN, and NaN compares false) and never needed below
            const float up = pp - comp(o, k), um = comp(o, k) - pm;
            umin = k == 0 ? __builtin_fminf(up, um) : __builtin_fminf(__builtin_fminf(umin, up), um);
            u[k] = pos ? up : um;
            v[k] = __builtin_fabsf(dk);
            posk[k] = pos;
        }
        // the nearest plane, kept as the lane masks n1, n2 (axis 1, axis 2
        // nearer) and the wall table's byte offset of the selected wall (8 k,
        // + 4 for the - wall), not as an axis index re-compared and
        // re-multiplied
        float un = u[0], vn = v[0];
        int offn = posk[0] ? 0 : 4;
        const bool n1 = u[1] * vn < un * v[1];
        un = n1 ? u[1] : un;
        vn = n1 ? v[1] : vn;
        offn = n1 ? (posk[1] ? 8 : 12) : offn;
        const bool n2 = u[2] * vn < un * v[2];
        un = n2 ? u[2] : un;
        vn = n2 ? v[2] : vn;
        offn = n2 ? (posk[2] ? 16 : 20) : offn;
        [[maybe_unused]] auto rec_at = [&](int off) { return reinterpret_cast<const LinRec *>(reinterpret_cast<const char *>(recs) + off); };
        // (fast mode: box mode runs only when no ray starts inside a wall --
        // KArgs::box_walls_out -- so the outside-only roots apply)
        {
            // 32-B geometry entries, entry 2 k + side at 8 offn bytes
            const GeoRec *wg = reinterpret_cast<const GeoRec *>(recs + A.n + 2);
            const GeoRec &g = *reinterpret_cast<const GeoRec *>(reinterpret_cast<const char *>(wg) + 8 * offn);
            const float4 g0 = g.g0, g1 = g.g1;
            test_geo(__float_as_int(g1.x), g0, g1,
                     std::integral_constant<int, !kExact ? kAxAnyOut : kAxAny>{}, un, vn);
        }
        const float bqm = bq * kPlaneMargin;
        // need[k]: wall k is not the selected one and its plane is not safely
        // beyond the winner's root.  Formed as wave masks by the scalar unit
        // from the selection's masks and one compare per plane (as per-lane
        // logic, !n1 and !n2 had been emitted as two more compares).  A
        // missing wall is never needed: its u is +inf, so the compare holds
        // unless bn v is NaN, and the pass below masks a missing wall's test
        // by its NaN geometry -- the same results
        bool need[3];
        const unsigned long long b1 = __ballot(n1), b2 = __ballot(n2);
        const unsigned long long nm[3] = {__ballot(!(bn * v[0] < u[0] * bqm)) & (b1 | b2),
                                          __ballot(!(bn * v[1] < u[1] * bqm)) & (~b1 | b2),
                                          __ballot(!(bn * v[2] < u[2] * bqm)) & ~b2};
        for (int k = 0; k < 3; ++k)
            need[k] = __builtin_amdgcn_inverse_ballot_w64(nm[k]);
        // a wall the ray moves away from can be hit only from beyond its
        // tangent plane (outside the room's bound on that side -- after a
        // bounce off a curved wall far from its tangent point, frequent in
        // box_mirror's mirror tube).  in_room: inside every bound, from the
        // plane distances already formed (host room_neg_margin: it implies
        // the six bound compares; a lane for which only those hold takes the
        // pass below, which checks the exact bounds -- the same tests run)
        const bool in_room = umin >= A.room_nmr;
        if ((__ballot(!in_room) | nm[0] | nm[1] | nm[2]) != 0ull) {
            PTG_STAT(3);
#if PTG_BLOCK_STATS == 3  // debug: wave cycles of the extra-wall block in [15]
            const unsigned long long xw_t0 = clock64();
#endif
#if PTG_BLOCK_STATS == 1  // [9] waves with a lane outside the room, [10] with a lane needing a wall toward; [11], [12] such lanes
            {
                const unsigned long long mo = __ballot(!in_room), mn = __ballot(need[0] | need[1] | need[2]);
                if (__lane_id() == __ffsll((long long)__ballot(1)) - 1) {
                    unsigned long long *st = &ptg_dbg_stats[(blockIdx.x & 255) * 16];
                    atomicAdd(st + 9, mo ? 1ull : 0ull);
                    atomicAdd(st + 10, mn ? 1ull : 0ull);
                    atomicAdd(st + 11, (unsigned long long)__popcll(mo));
                    atomicAdd(st + 12, (unsigned long long)__popcll(mn));
                }
            }
#endif
            // each lane's extra walls in the order of the scan below (toward
            // x, y, z, then away x, y, z): one wall per lane per pass, so a
            // wave pays one test per pass, not one per axis any lane needs
            unsigned m = (need[0] ? 1u : 0u) | (need[1] ? 2u : 0u) | (need[2] ? 4u : 0u);
            if (__ballot(!in_room) != 0ull) {
                for (int k = 0; k < 3; ++k) {
                    float pp = A.plane_plus[k], pm = A.plane_minus[k], lo = A.pair_lo[k], hi = A.pair_hi[k];
                    asm volatile("" : "+s"(pp), "+s"(pm), "+s"(lo), "+s"(hi));
                    const float ok = comp(o, k);
                    const bool pos = comp(d, k) >= 0.0f;
                    // (the wall's existence checked by value as well: a NaN
                    // origin must not select a missing wall's record)
                    // (mask logic, not a select: the select became two exec-mask blocks)
                    const bool away = (pos & !(ok >= lo) & (pm > -HUGE_VALF)) | (!pos & !(ok <= hi) & (pp < HUGE_VALF));
                    m |= away ? 8u << k : 0u;
                }
            }
            while (__ballot(m != 0u) != 0ull) {
                const int j = __builtin_ctz(m | 64u);  // 6: none left
                m &= m - 1u;
                const int k = j < 3 ? j : (j < 6 ? j - 3 : 0);
                const bool toward = j < 3;
                // the wall's geometry entry (axis, side) of the table above:
                // one dependent LDS read; a missing wall's NaN geometry never
                // passes the cull's compares' win
                const int side = (comp(d, k) >= 0.0f) == toward ? 0 : 1;
                const GeoRec &gx = reinterpret_cast<const GeoRec *>(recs + A.n + 2)[2 * k + side];
                const float4 x0 = gx.g0, x1 = gx.g1;
                test_geo(__float_as_int(x1.x), x0, x1, std::integral_constant<int, kAxSel>{}, 0.0f, 0.0f,
                         j < 6, k);
            }
#if PTG_BLOCK_STATS == 3
            {
                const unsigned long long xw_t1 = clock64();
                if (__lane_id() == __ffsll((long long)__ballot(1)) - 1)
                    atomicAdd(&ptg_dbg_stats[(blockIdx.x & 255) * 16 + 15], xw_t1 - xw_t0);
            }
#endif
        }
        i = A.end_ax[2];
    } else {
        axis_group(std::integral_constant<int, kAxX>{});
        axis_group(std::integral_constant<int, kAxY>{});
        axis_group(std::integral_constant<int, kAxZ>{});
    }
    for (; i < A.end_big; ++i)
        test(i, std::integral_constant<int, kBig>{});
    small_spheres(i);
    tbest = bi != 0 ? Math<kExact>::div(bn, bq) : kInf;
    return reinterpret_cast<const LinRec *>(reinterpret_cast<const char *>(recs + A.n) + bi);
}

// Scenes with more than kLinearMax spheres: the huge
// spheres linearly, then a stackless walk of the BVH.  The nearest-hit rule
// here is the reference's own -- every candidate root is divided,
// t = fl(num/den), and the winner is the smallest t, lowest scene index on
// ties (main.cpp:35 strict <, in index order) -- which does not depend on the
// visiting order, so the oracle reproduces it with a linear scan.  Box tests
// only cull: boxes are padded (bvh_build.hpp) and use fast reciprocals.

// Root of one sphere under the reference's rule (the root >= eps nearest to
// the origin, t = fl(num/den)); NaN when rejected or provably not below tb
// (the two exact culls of DESIGN.md "scene scan").  kBig: anchored form with
// g0 = {P0, R}, g1 = {n0, 2R} (huge spheres); else g0 = {C, -R^2}.
constexpr float kReject = __builtin_nanf("");  // every comparison with it is false

// the cull's scaled culling distance: tb * -2 (1 + 2^-20), exact constant
constexpr float kCullScale = -2.0f * kCullMargin;

template <bool kBig, bool kExact>
__device__ __forceinline__ float root_lex(const float4 g0, const float4 g1, const f3 o, const f3 d, const float a,
                                          const float tb, const float tbm)
{
    f3 e = mk3(o.x - g0.x, o.y - g0.y, o.z - g0.z);
    float ed = dot3(e, d);
    float ee = dot3(e, e);
    float hb, c;
    if constexpr (kBig) {
        hb = __builtin_fmaf(g0.w, dot3(mk3(g1.x, g1.y, g1.z), d), ed);
        c = __builtin_fmaf(g1.w, dot3(e, mk3(g1.x, g1.y, g1.z)), ee);
    } else {
        hb = ed;
        c = ee + g0.w;  // g0.w = -R^2
    }
    // the two culls and the discriminant test as one early-out (bitwise: the
    // && chains had been evaluated as nested exec-masked blocks; C5 -1.1 %)
    // The two culls as one compare: behind (hb >= 0, c >= 0) and beyond (hb
    // < 0, near root > tb: c >= 2 |hb| tb (1 + 2^-20); the margin covers the q
    // bound's 3u and the two roundings) are c >= max(hb tbm, 0) with tbm = tb
    // * kCullScale < 0 from the caller (once per change of tb): hb tbm <= 0
    // for hb >= 0 (NaN for hb = 0, tb = inf: fmax gives 0), > 0 for hb < 0.
    // (As two sign-selected compares the choice was materialised: 5 VALU.)
    const bool culled = c >= __builtin_fmaxf(hb * tbm, 0.0f);
    float disc;
    if constexpr (kBig) {
        disc = __builtin_fmaf(hb, hb, -(a * c));
    } else {
        // Lagrange form (scene_scan), limited to hb^2 for an origin outside
        // (c >= 0: exactly disc <= hb^2), which keeps q <= 2|hb|(1 + 3u)
        // and so the cull above exact
        const f3 x = cross3(e, d);
        disc = __builtin_fmaf(a, -g0.w, -dot3(x, x));
        disc = c >= 0.0f ? __builtin_fminf(disc, hb * hb) : disc;
    }
    if (culled | (disc < 0.0f))
        return kReject;
    const float sq = Math<kExact>::sqrt(disc);  // disc >= 0 here
    // the near root c/q (hb < 0, q = sq - hb), else the far root q/a, or -c/qn
    // (hb >= 0, qn = hb + sq) -- as selects (scene_scan's form: sq - hb and
    // hb + sq are the IEEE add sq + |hb|; one eps test covers the three cases),
    // not two divergent branches that a wave with both signs ran one after
    // the other
    const bool neg = hb < 0.0f;
    const float qq = sq + __builtin_fabsf(hb);
    const bool near_lt = c < kEps * qq;
    const float num = neg ? (near_lt ? qq : c) : -c;
    const float den = (neg & near_lt) ? a : qq;
    if (num < kEps * den)
        return kReject;
    if constexpr (kExact)
        return num / den;  // IEEE: the oracle's intersect_B_lex
    else
        return Math<false>::div(num, den);
}

// The BVH scan's winner is its scene index (-1: none).  Ties of t go to the
// lowest scene index (main.cpp:35: strict < in index order), which makes the
// result independent of the visiting order: the oracle's linear scan
// (intersect_B_lex) gives the same bits.
__device__ __forceinline__ void update_lex(const float t, const int sid, float &tb, int &best)
{
    // a NaN t (rejected) fails both compares; (unsigned) -1 orders after every
    // index.  Selects, not a short-circuit && / || (exec-masked blocks)
    const bool win = (t < tb) | ((t == tb) & ((unsigned)sid < (unsigned)best));
    tb = win ? t : tb;
    best = win ? sid : best;
}

// Per-lane BVH scan state.  The render kernel keeps it across iterations of
// its main loop (resumable scan): lanes whose scan ends early shade and start
// their next segment while the wave keeps walking for the long rays -- a
// wave otherwise waits for its slowest ray (measured 93 wave-level node
// steps for 33 per ray on the 10,000-sphere scene).
// global (address space 1) pointers: kernel-argument pointers pinned in
// SGPRs lose their address space, and generic (flat) loads also wait on LDS
template <class T>
using gptr = const T __attribute__((address_space(1))) *;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // a compact node record, loadable from gptr

struct BvhTrav {
    int ni;    // binary: next node in depth-first order; wide: see below
    int pend;  // parked leaf (first | count << 24) or -1
    float tb;  // nearest root so far
    int best;  // winner's scene index or -1
    // wide walk: ni = the next position (a wide node's first record + the
    // slot to resume from, >= 0), -1 (walk finished), or -- only while a leaf
    // is parked -- kPopLater (-2: pop the stack after the leaf phase) or a
    // leaf word (parked after the leaf phase).  A two-entry stack (top first, -1 empty)
    // of positions / leaf words still to visit; when it overflows it is
    // cleared and the walk continues, once it runs dry, from the resume
    // position `res` and its continuation chain (bvh_build.hpp wide_conts:
    // everything after it in depth-first order, culled by tb), so any tree
    // depth is walked correctly with three registers.
    int s0, s1;
#if PTG_BVH_STACK >= 3
    int s2;
#endif
    int res;
};

__device__ __forceinline__ bool bvh_done(const KArgs &, const BvhTrav &tr) { return (tr.ni == -1) & (tr.pend < 0); }
__device__ __forceinline__ int bvh_pop(gptr<int> cont, BvhTrav &tr)
{
    const int v = tr.s0;
    tr.s0 = tr.s1;
#if PTG_BVH_STACK >= 3
    tr.s1 = tr.s2;
    tr.s2 = -1;
#else
    tr.s1 = -1;
#endif
    if (v != -1)
        return v;
    const int r = tr.res;  // stack dry: the resume position, then its continuation
    if (r != -1)
        tr.res = cont[r >> 2];
    return r;
}

// Start a scan: the huge spheres (tested linearly, first), then the BVH in
// the layout of the ray's direction octant.
template <bool kCount, bool kExact>
__device__ __forceinline__ void bvh_start(const KArgs &A, f3 o, f3 d, BvhTrav &tr, ScanCount &cnt)
{
    const float a = dot3(d, d);
    tr.tb = kInf;
    tr.best = -1;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(4))) f32x4 *cvec_t;
    typedef const __attribute__((address_space(4))) int *cint_t;
    const cvec_t bgeo = (cvec_t)A.big_geo;  // GeoRec k: words 2 k, 2 k + 1
    const cint_t bid = (cint_t)A.big_id;
    for (int k = 0; k < A.n_big; ++k) {
        const f32x4 v0 = bgeo[2 * k], v1 = bgeo[2 * k + 1];
        const float4 g0 = make_float4(v0.x, v0.y, v0.z, v0.w), g1 = make_float4(v1.x, v1.y, v1.z, v1.w);
        update_lex(root_lex<true, kExact>(g0, g1, o, d, a, tr.tb, tr.tb * kCullScale), bid[k], tr.tb, tr.best);
    }
    if constexpr (kCount)
        cnt.spheres += A.n_big;
    // the wide layouts store each box near-plane first for their octant:
    // all 8 layouts exist
    const unsigned oct = (__float_as_uint(d.x) >> 31) | ((__float_as_uint(d.y) >> 30) & 2u) |
                         ((__float_as_uint(d.z) >> 29) & 4u);
    tr.ni = A.n_nodes > 0 ? (int)(oct << 2) : -1;  // layout k's root: interleaved node k
    tr.s0 = -1;
    tr.s1 = -1;
#if PTG_BVH_STACK >= 3
    tr.s2 = -1;
#endif
    tr.res = -1;
    tr.pend = -1;
}

// Slab-test constants of a ray in the compact nodes' grid units (culling
// only: fast reciprocals, boxes padded and rounded outward):
// t = q * (scale / d) + (lo - o) / d.
struct SlabRay {
    float sx, sy, sz, bx, by, bz;
};
__device__ __forceinline__ SlabRay slab_ray(const KArgs &A, f3 o, f3 d)
{
    const float ix = d.x != 0.0f ? __builtin_amdgcn_rcpf(d.x) : __builtin_copysignf(1e30f, d.x);
    const float iy = d.y != 0.0f ? __builtin_amdgcn_rcpf(d.y) : __builtin_copysignf(1e30f, d.y);
    const float iz = d.z != 0.0f ? __builtin_amdgcn_rcpf(d.z) : __builtin_copysignf(1e30f, d.z);
    SlabRay r;
    r.sx = A.q_scale[0] * ix;
    r.sy = A.q_scale[1] * iy;
    r.sz = A.q_scale[2] * iz;
    r.bx = (A.q_lo[0] - o.x) * ix;
    r.by = (A.q_lo[1] - o.y) * iy;
    r.bz = (A.q_lo[2] - o.z) * iz;
    return r;
}


// Box test of a wide-layout record: binary16 planes on the wide grid, stored
// near-plane first for the ray's octant (bvh_build.hpp WideGrid), each read
// by one v_fma_mix_f32.  No slab margin: the boxes are padded far beyond the
// rounding of the slab times (bvh_build.hpp); tcap keeps the 1e-4 margin
// over the nearest root.
// binary16 halves of a word as float: folded into v_fma_mix_f32 operands.
// (A __builtin_bit_cast of the word to a 2 x _Float16 vector miscompiles
// here: every plane was read from the record's first word.)
__device__ __forceinline__ float lo_half(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu)); }
__device__ __forceinline__ float hi_half(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
__device__ __forceinline__ bool box_hit_sorted(const u32x4 q, const SlabRay &r, const float tcap)
{
    const float tnx = __builtin_fmaf(lo_half(q.x), r.sx, r.bx);
    const float tny = __builtin_fmaf(hi_half(q.x), r.sy, r.by);
    const float tnz = __builtin_fmaf(lo_half(q.y), r.sz, r.bz);
    const float tfx = __builtin_fmaf(hi_half(q.y), r.sx, r.bx);
    const float tfy = __builtin_fmaf(lo_half(q.z), r.sy, r.by);
    const float tfz = __builtin_fmaf(hi_half(q.z), r.sz, r.bz);
    const float t_in = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), __builtin_fmaxf(tnz, 0.0f));
    // tcap by its own compare: as a min operand it came from outside the
    // node step's block, so the compiler re-canonicalised it (v_max x, x) in
    // every step; the slab times are fresh v_fma_mix results
    const float t_out = __builtin_fminf(__builtin_fminf(tfx, tfy), tfz);
    return !(t_in > t_out) & !(t_in > tcap);
}

// One wide node step at position ni (node + first slot): the node's 4
// records (one 64-B line) in one go.  Slots are in near-first order for the
// layout's octant.  The nearest hit child is visited next -- or, when it is a
// leaf, parked in tr.pend and the second hit visited next; of the hits after
// that one goes on the stack as itself, several as the position of the first
// (the node is re-tested from there, with the culling distance of then).
// With no successor the stack is popped -- at most once per step, and not
// when a leaf was parked: ni = kPopLater then, and the leaf phase pops.
// Selections are branch-free (v_cndmask).
constexpr int kPopLater = -2;
__device__ __forceinline__ int bvh_pop_sel(gptr<int> cont, BvhTrav &tr, const bool need, const int keep);
template <bool kCount>
__device__ __forceinline__ void bvh_node_step(gptr<int> cont, gptr<u32x4> qnodes, const SlabRay &r_in, BvhTrav &tr,
                                              ScanCount &cnt)
{
    const int base = tr.ni & ~3;
    u32x4 q0, q1, q2, q3;
    const SlabRay &r = r_in;
    {
        // a 32-bit byte offset on the uniform base: the load's saddr form
        // (no 64-bit address arithmetic per lane)
        gptr<u32x4> q = (gptr<u32x4>)((const __attribute__((address_space(1))) char *)qnodes + ((unsigned)base << 4));
        q0 = q[0];
        q1 = q[1];
        q2 = q[2];
        q3 = q[3];
    }
    if constexpr (kCount)
        cnt.boxes += 4 - (tr.ni & 3);
    const float tcap = tr.tb * 1.0001f;
    // slots before the walk's position (ni & 3) are not tested again
    const int s = tr.ni & 3;
    const bool h0 = box_hit_sorted(q0, r, tcap) & (s == 0), h1 = box_hit_sorted(q1, r, tcap) & (s <= 1),
               h2 = box_hit_sorted(q2, r, tcap) & (s <= 2), h3 = box_hit_sorted(q3, r, tcap);
    // the words of the first three hits in slot order (-1: none) and the
    // slots of the second and third, shifted in from the last slot: every
    // step is a v_cndmask on its box test's lane mask (the hit mask with
    // lowest-set-bit lookups took 10-16 VALU more per node step: C5 +4.8 %)
    int w1 = h3 ? (int)q3.w : -1, w2 = -1, w3 = -1;
    w2 = h2 ? w1 : w2;
    w1 = h2 ? (int)q2.w : w1;
    w3 = h1 ? w2 : w3;
    w2 = h1 ? w1 : w2;
    w1 = h1 ? (int)q1.w : w1;
    w3 = h0 ? w2 : w3;
    w2 = h0 ? w1 : w2;
    w1 = h0 ? (int)q0.w : w1;
    int i2 = 3, i3 = 3;  // (meaningful only where the hit exists)
    i3 = h1 ? i2 : i3;
    i2 = h1 ? (h2 ? 2 : 3) : i2;
    i3 = h0 ? i2 : i3;
    i2 = h0 ? (h1 ? 1 : h2 ? 2 : 3) : i2;
    const bool leaf = w1 < kPopLater;  // the first hit is a leaf: parked (no hit: w1 = -1)
    int next = leaf ? (w2 != -1 ? w2 : kPopLater) : w1;
    tr.pend = leaf ? (w1 & 0x7FFFFFFF) : tr.pend;
    // the hits left after next: from the second (an inner first hit) or the
    // third (a parked leaf); one goes on the stack as its word, several as
    // the position of the first of them
    // (each select on one lane mask: a select between two conditions was
    // materialised as 5 VALU)
    const bool push = leaf ? w3 != -1 : w2 != -1;
    const int pos = base + (leaf ? i3 : i2);
    const int e = leaf ? ((h0 & h1 & h2 & h3) ? pos : w3) : (w3 != -1 ? pos : w2);
#if PTG_BVH_STACK >= 3
    const bool full = tr.s2 != -1;
    tr.res = (push & full) ? pos : tr.res;
    const int s0 = tr.s0, s1 = tr.s1;
    tr.s0 = push ? (full ? -1 : e) : s0;
    tr.s1 = push ? (full ? -1 : s0) : s1;
    tr.s2 = push ? (full ? -1 : s1) : tr.s2;
#else
    const bool full = tr.s1 != -1;
    tr.res = (push & full) ? pos : tr.res;
    const int s0 = tr.s0;
    tr.s0 = push ? (full ? -1 : e) : s0;
    tr.s1 = push ? (full ? -1 : s0) : tr.s1;
#endif
    if (next == -1) {
        next = bvh_pop(cont, tr);
        if (next < kPopLater) {  // a leaf from the stack
            tr.pend = next & 0x7FFFFFFF;
            next = kPopLater;
        }
    }
    tr.ni = next;
}

// The render kernel's leaf completion (bvh_leaf_done) and its pop, executed
// by every lane of the wave: lanes without a tested leaf (act false) keep
// their state through selects.  As nested divergent branches the update
// merged the traversal state through exec-masked copies (39 v_mov per leaf
// phase in the ISA); same values, C5 -0.5 %.
//
// Pop where need (else return keep): the stack top, or once it runs dry the
// resume position and its continuation -- the one load stays behind a branch
// (rare: the two-entry stack overflowed earlier).
__device__ __forceinline__ int bvh_pop_sel(gptr<int> cont, BvhTrav &tr, const bool need, const int keep)
{
    const int v = tr.s0, r = tr.res;
    const bool dry = v == -1;
    int nres = r;
    if (need & dry & (r != -1))
        nres = cont[r >> 2];
    tr.s0 = need ? tr.s1 : v;
#if PTG_BVH_STACK >= 3
    tr.s1 = need ? tr.s2 : tr.s1;
    tr.s2 = need ? -1 : tr.s2;
#else
    tr.s1 = need ? -1 : tr.s1;
#endif
    tr.res = nres;
    return need ? (dry ? r : v) : keep;
}

// bvh_leaf_done for the lanes whose parked leaf was tested (act)
__device__ __forceinline__ void bvh_leaf_done_sel(gptr<int> cont, BvhTrav &tr, const bool act)
{
    tr.pend = act ? -1 : tr.pend;
    int next = bvh_pop_sel(cont, tr, act & (tr.ni == kPopLater), tr.ni);
    const bool lf = act & (next < kPopLater);  // a leaf word (popped, or waiting in ni)
    tr.pend = lf ? (next & 0x7FFFFFFF) : tr.pend;
    next = lf ? kPopLater : next;
    tr.ni = act ? next : tr.ni;
}

// Spheres [f, f + cnt) of the leaf order against one ray: compact records
// {C, -R^2}; (tb, best) updated by the lex rule.
template <bool kCount, bool kExact>
__device__ __forceinline__ void leaf_spheres(const KArgs &A, int f, int cnt, f3 o, f3 d, float &tb, int &best,
                                             ScanCount &sc)
{
    const float a = dot3(d, d);
    if constexpr (kCount)
        sc.spheres += cnt;
    // 32-bit byte offsets on the uniform bases (saddr loads)
    const char *sph = (const char *)A.bvh_sph;
    const char *ids = (const char *)A.bvh_id;
    float tbm = tb * kCullScale;
    for (int j = 0; j < cnt; ++j) {
        const unsigned off = (unsigned)(f + j) << 4;
        const float4 rec = *(const float4 *)(sph + off);
        const float t = root_lex<false, kExact>(rec, float4{}, o, d, a, tb, tbm);
        if (t <= tb) {  // the scene index is read only for a candidate that wins or ties
            update_lex(t, *(const int *)(ids + (off >> 2)), tb, best);
            tbm = tb * kCullScale;
        }
    }
}

// After the parked leaf's spheres: wide walk -- a leaf word waiting in tr.ni
// is parked next, or the pop deferred by the node step happens.
__device__ __forceinline__ void bvh_leaf_done(gptr<int> cont, BvhTrav &tr)
{
    tr.pend = -1;
    if (tr.ni < -1) {  // kPopLater, or the leaf the node step moved to after parking one
        int next = tr.ni == kPopLater ? bvh_pop(cont, tr) : tr.ni;
        if (next < kPopLater) {  // a leaf: parked for the next leaf phase
            tr.pend = next & 0x7FFFFFFF;
            next = kPopLater;
        }
        tr.ni = next;
    }
}

// The parked leaf's spheres, all by this lane.
template <bool kCount, bool kExact>
__device__ __forceinline__ void bvh_leaf(const KArgs &A, gptr<int> cont, f3 o, f3 d, BvhTrav &tr, ScanCount &cnt)
{
    const int first = tr.pend & 0xFFFFFF, nl = tr.pend >> 24;
    const int take = nl;
    leaf_spheres<kCount, kExact>(A, first, take, o, d, tr.tb, tr.best, cnt);
    if (take < nl) {
        tr.pend = (first + take) | ((nl - take) << 24);
        return;
    }
    bvh_leaf_done(cont, tr);
}

// Leaf phase with helpers (PTG_LEAF_SPLIT; called by the whole wave): lanes
// with no leaf to test are assigned, by rank, to lanes holding a leaf of >= 2
// spheres -- one helper per such leaf, longest leaves (>= PTG_LONG_LEAF spheres: they set
// the wave's loop length) first, then a second helper per long leaf while
// idle lanes remain.  A helper tests its part of the leaf with the owner's
// ray and culling distance (ds_bpermute) and the owner merges the helpers'
// nearest roots by the same lex rule -- order-independent, so the result is
// the one-lane result bit for bit.  pair: 2 x 64 bytes of LDS (owner lane by
// owner rank, helper lane by helper rank).
template <bool kCount, bool kExact>
__device__ __forceinline__ void bvh_leaf_split(const KArgs &A, gptr<int> cont, f3 o, f3 d, bool has,
                                               unsigned long long mhas, BvhTrav &tr, ScanCount &cnt,
                                               uint8_t (*pair)[64])
{
    const int lane = (int)__lane_id();
    const int nl = has ? (tr.pend >> 24) : 0;
    const bool own = nl >= 2, hlp = !has;
    auto rank = [](unsigned long long m) {
        return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    };
    const bool longl = nl >= PTG_LONG_LEAF;
    // (mhas = ballot(has), the whole wave active: ballots of single compares only)
    const unsigned long long ml = __ballot(longl), ms = __ballot(own) & ~ml, mh = ~mhas;
    const int nlong = (int)__popcll(ml), nown = nlong + (int)__popcll(ms), nhelp = (int)__popcll(mh);
    const int np1 = min(nown, nhelp);  // owners (by rank) with a first helper
#if PTG_LEAF_SPLIT >= 2
    const int np2 = max(0, min(nlong, nhelp - nown));  // long-leaf owners with a second helper
#else
    const int np2 = 0;
#endif
    const int ro = longl ? rank(ml) : nlong + rank(ms);
    const int rh = rank(mh);
    const bool po = own & (ro < np1), ph = hlp & (rh < np1 + np2);
    if (po)
        pair[0][ro] = (uint8_t)lane;
    if (ph)
        pair[1][rh] = (uint8_t)lane;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int orank = rh < np1 ? rh : rh - np1;  // a helper's owner, and which helper it is
    const int part = rh < np1 ? 1 : 2;
    const int partner = po ? (int)pair[1][ro] : ph ? (int)pair[0][orank] : lane;
    const int partner2 = (po & (ro < np2)) ? (int)pair[1][np1 + ro] : lane;
    auto bpf = [](int who, float v) {
        return __int_as_float(__builtin_amdgcn_ds_bpermute(who << 2, __float_as_int(v)));
    };
    auto bpi = [](int who, int v) { return __builtin_amdgcn_ds_bpermute(who << 2, v); };
    // helpers take the owner's ray, culling distance and leaf
    const f3 po3 = mk3(bpf(partner, o.x), bpf(partner, o.y), bpf(partner, o.z));
    const f3 pd3 = mk3(bpf(partner, d.x), bpf(partner, d.y), bpf(partner, d.z));
    const float ptb = bpf(partner, tr.tb);
    const int ppend = bpi(partner, tr.pend);
    const f3 ro3 = ph ? po3 : o, rd3 = ph ? pd3 : d;
    const int pendl = ph ? ppend : tr.pend;
    const int first = pendl & 0xFFFFFF, nll = pendl >> 24;
    // the leaf's parts: one helper -> [0, ceil(n/2)), [ceil(n/2), n); two
    // helpers -> [0, n/3), [n/3, 2n/3), [2n/3, n) (n <= 12: x/3 = x*11 >> 5)
    const int k = ph ? 1 + (orank < np2) : po ? 1 + (ro < np2) : 0;
    const int b1 = k == 2 ? (nll * 11) >> 5 : (nll + 1) >> 1;
    const int b2 = k == 2 ? (2 * nll * 11) >> 5 : nll;
    const int lo = !ph ? 0 : part == 1 ? b1 : b2;
    const int hi = !ph ? (po ? b1 : (has ? nll : 0)) : part == 1 ? b2 : nll;
    const int f = first + lo, c = hi - lo;
    float tb = ph ? ptb : tr.tb;
    int best = ph ? -1 : tr.best;
#if PTG_WAVE_STATS == 1  // debug: the wave's loop length
    {
        int mx = c;
        for (int off = 32; off > 0; off >>= 1)
            mx = max(mx, __shfl_xor(mx, off, 64));
        const bool first_lane = lane == __ffsll((long long)__ballot(1)) - 1;
        cnt.spheres += first_lane ? (uint32_t)mx : 0u;
    }
#endif
    leaf_spheres<kCount && !PTG_WAVE_STATS, kExact>(A, f, c, ro3, rd3, tb, best, cnt);
    // owners merge their helpers' nearest roots
    const float htb = bpf(partner, tb), htb2 = bpf(partner2, tb);
    const int hbest = bpi(partner, best), hbest2 = bpi(partner2, best);
    if (po) {
        update_lex(htb, hbest, tb, best);
        update_lex(htb2, hbest2, tb, best);  // partner2 = lane without a second helper: a no-op
    }
    tr.tb = has ? tb : tr.tb;
    tr.best = has ? best : tr.best;
    bvh_leaf_done_sel(cont, tr, has);
}

// Whole scan of one ray (parity probe kernel): walk, testing each parked leaf
// at once.
template <bool kCount, bool kExact>
__device__ __forceinline__ int scene_scan_bvh(const KArgs &A, f3 o, f3 d, float &tbest, ScanCount &cnt)
{
    BvhTrav tr;
    bvh_start<kCount, kExact>(A, o, d, tr, cnt);
    const SlabRay sr = slab_ray(A, o, d);
    while (!bvh_done(A, tr)) {
        if (tr.pend >= 0)
            bvh_leaf<kCount, kExact>(A, (gptr<int>)A.bvh_cont, o, d, tr, cnt);
        else
            bvh_node_step<kCount>((gptr<int>)A.bvh_cont, (gptr<u32x4>)A.bvh_qnodes, sr, tr, cnt);
    }
    tbest = tr.tb;
    return tr.best;
}

// Per-lane state machine: one call = one bounce segment of radiance()
// (main.cpp:111-155).  Returns true when the path has ended; E then holds
// its radiance.
// shade(): everything after the scene scan -- sky on a miss, else hit
// record, emission, Russian roulette, BRDF sampling of the next ray.
//
// Light sampling (kLS; PTG_FLAG_LIGHT_SAMPLING, include/ptgpu.h): a diffuse
// hit may be followed by a shadow segment -- one more state of the lane.  The
// lane keeps the contribution the segment would add, the BRDF direction it
// resumes with and the light's id in LsLane; the segment's origin is the hit
// point, which o already holds.  What the lane is doing travels in LsIo: in,
// this segment is a shadow segment / this hit skips the listed emitters; out,
// the same two for the lane's next segment (the callers keep them as wave
// masks).  Without kLS both structs are unused and the code is as before.
struct LsLane {
    f3 pend, nd;
    int light;
};
struct LsIo {
    const LightRec *lights;
    int n_lights;
    int hid;                     // what the scan reported (LightRec id)
    bool shadow, skip;           // in
    bool to_shadow, skip_next;   // out
};
// kStrat (PTG_FLAG_STRATIFIED): fh holds the path's pairs 2 and 3, {phi, r,
// u1, u2} of its first hit -- read only at depth 0, on a diffuse lane
template <bool kExact, bool kLS = false, bool kStrat = false>
__device__ __forceinline__ bool shade(const ShadeRec *hit, float t, const float2 *trig, f3 &o, f3 &d, f3 &T, f3 &E,
                                      int &depth, uint32_t &st, LsLane &ls, LsIo &io, const uint4 fh = uint4{});
template <bool kExact>
__device__ __forceinline__ bool shade(const ShadeRec *hit, float t, const float2 *trig, f3 &o, f3 &d, f3 &T, f3 &E,
                                      int &depth, uint32_t &st)
{
    LsLane ls;
    LsIo io;
    return shade<kExact, false>(hit, t, trig, o, d, T, E, depth, st, ls, io);
}

template <bool kBvh, bool kExact, bool kCount = false, bool kLS = false, bool kStrat = false>
__device__ __forceinline__ bool segment(const KArgs &A, const LinRec *recs, const float2 *trig, f3 &o, f3 &d, f3 &T,
                                        f3 &E, int &depth, uint32_t &st, ScanCount &cnt, LsLane &ls, LsIo &io,
                                        [[maybe_unused]] const uint4 fh = uint4{})
{
    float t;
    const ShadeRec *hit;
    if constexpr (kBvh) {
        const int id = scene_scan_bvh<kCount, kExact>(A, o, d, t, cnt);
        hit = id >= 0 ? A.shade + id : nullptr;
        if constexpr (kLS)
            io.hid = id;
    } else {
        const LinRec *w = scene_scan<kExact, kCount>(A, recs, o, d, t, cnt);
        hit = w != recs + A.n ? &w->s : nullptr;
        if constexpr (kLS)
            io.hid = (int)(w - recs);
    }
    if constexpr (kStrat)
        return shade<kExact, kLS, true>(hit, t, trig, o, d, T, E, depth, st, ls, io, fh);
    else
    return shade<kExact, kLS>(hit, t, trig, o, d, T, E, depth, st, ls, io);
}
template <bool kBvh, bool kExact, bool kCount = false>
__device__ __forceinline__ bool segment(const KArgs &A, const LinRec *recs, const float2 *trig, f3 &o, f3 &d, f3 &T,
                                        f3 &E, int &depth, uint32_t &st, ScanCount &cnt)
{
    LsLane ls;
    LsIo io;
    return segment<kBvh, kExact, kCount, false>(A, recs, trig, o, d, T, E, depth, st, cnt, ls, io);
}

template <bool kExact, bool kLS, bool kStrat>
__device__ __forceinline__ bool shade(const ShadeRec *hit, float t, const float2 *trig, f3 &o, f3 &d, f3 &T, f3 &E,
                                      int &depth, uint32_t &st, [[maybe_unused]] LsLane &ls, [[maybe_unused]] LsIo &io,
                                      [[maybe_unused]] const uint4 fh)
{
    if constexpr (kLS) {
        // a shadow segment's "shade": the pending value when the light is
        // the nearest hit, then on with the bounce; depth is not counted
        if (io.shadow) {
            const bool lit = io.hid == ls.light;
            E = mk3(lit ? E.x + ls.pend.x : E.x, lit ? E.y + ls.pend.y : E.y, lit ? E.z + ls.pend.z : E.z);
            d = ls.nd;
            io.skip_next = true;
            return false;
        }
    }
    // the segment count first, for every lane: a sky lane's path ends here
    // (its depth is reset by the refill), so the value is only read below --
    // no per-branch copy of the loop-carried register
    depth += 1;
    // kStrat: the camera ray's own hit takes its BRDF and light-sample draws
    // from the path's pairs (io.fh) and leaves the xorshift state where it is
    [[maybe_unused]] const bool first = kStrat && depth == 1;
    if (!hit) {  // main.cpp:115-120: sky
        f3 ud = norm3m<kExact>(d);
        float tt = 0.5f * (ud.y + 1.0f);
        float it = 1.0f - tt;
        E = mk3(__builtin_fmaf(T.x, __builtin_fmaf(tt, 0.5f, it), E.x),
                __builtin_fmaf(T.y, __builtin_fmaf(tt, 0.7f, it), E.y),
                __builtin_fmaf(T.z, __builtin_fmaf(tt, 1.0f, it), E.z));
        return true;
    }
    const ShadeRec &S = *hit;
    float4 s0 = S.s0;
    const float4 s1 = S.s1;
    // hit_record.cpp:3-12
    f3 p = mk3(__builtin_fmaf(d.x, t, o.x), __builtin_fmaf(d.y, t, o.y), __builtin_fmaf(d.z, t, o.z));
    // hit_record.cpp:6 (p - C).norm() as (p - C) * (1/R): p lies on the sphere
    const bool rr = depth > kRRThreshold + 1;  // (the depth before this segment's count)
    const float4 cc = *(rr ? &S.s3 : &S.s2);  // (prepare_scene: 1/R in s2.w and s3.w)
    const float invR = cc.w;
    bool front;
    f3 on, nn;
    [[maybe_unused]] float kn = 0.0f;  // fast mode: nn.d
    if (!kExact) {
        const f3 pc = mk3(p.x - s0.x, p.y - s0.y, p.z - s0.z);
        const float sd = dot3(pc, d);
        front = sd < 0.0f;
        const float ks = front ? invR : -invR;
        nn = mk3(pc.x * ks, pc.y * ks, pc.z * ks);
        kn = sd * ks;
        on = nn;  // (unused: the mirror reflects on nn)
    } else {
        on = mk3((p.x - s0.x) * invR, (p.y - s0.y) * invR, (p.z - s0.z) * invR);
        front = dot3(on, d) < 0.0f;
        nn = front ? on : mk3(-on.x, -on.y, -on.z);
    }
    // main.cpp:126
    if constexpr (kLS) {
        // the hit after a light-sampling step: the listed emitters were
        // sampled there (their ids by wave-uniform loads) -- those met on
        // their front face.  A back face means the previous hit point lay
        // inside that light, where the step adds nothing: it counts here
        bool listed = false;
        if (io.skip & front)
            for (int k = 0; k < io.n_lights; ++k)
                listed |= io.hid == __float_as_int(io.lights[k].e.w);
        if (!listed)
            E = mk3(__builtin_fmaf(T.x, s1.x, E.x), __builtin_fmaf(T.y, s1.y, E.y), __builtin_fmaf(T.z, s1.z, E.z));
    } else
    E = mk3(__builtin_fmaf(T.x, s1.x, E.x), __builtin_fmaf(T.y, s1.y, E.y), __builtin_fmaf(T.z, s1.z, E.z));
    // main.cpp:128-139: Russian roulette after depth 4 (the colour row read
    // above by address)
    // Russian roulette without an early return: the roulette's draw advances the state of the
    // rr lanes only (a select), and a killed lane runs on with its materials
    // masked -- its next ray and state are discarded (the early return's
    // merge had cost state copies and exec-mask blocks)
    uint32_t st_rr = st;
    const uint32_t m_rr = draw_bits(st_rr);  // u = m_rr 2^-24; s0.w holds ceil(p 2^24) (prepare_scene)
    st = rr ? st_rr : st;
    const bool killed = rr & !(m_rr < __float_as_uint(s0.w));
    T = mk3(T.x * cc.x, T.y * cc.y, T.z * cc.z);
    // BRDF samplers (main.cpp:44-97).  Diffuse and dielectric lanes share the
    // three expensive ops (one rsqrt, two sqrt) through selects, so a wave
    // holding both materials issues them once; every lane's arithmetic is the
    // same as the per-material code (oracle sample_B).
    const int mat = __float_as_int(s1.w);
    const bool isD = !killed & (mat == PTG_DIFFUSE);
    const bool isG = !killed & (mat == PTG_DIELECTRIC);
    bool spec = !killed & (mat == PTG_SPECULAR);
    // every lane's first BRDF draw taken once, here: the diffuse phi, the
    // dielectric's Fresnel draw -- or, where it cannot refract, its
    // reflection's draw -- and the mirror's draw (main.cpp:46, :89, :62).
    // A dielectric lane reflected by its Fresnel draw takes the reflection's
    // draw as well: the block's shared second step below (fres_refl).
    // Each lane's draws keep their order and count; killed lanes advance a
    // state their ended path no longer reads.
    // light sampling: a diffuse lane whose path goes on takes the step's
    // draws first -- the light (only with several), then u1, u2 -- whatever
    // the geometry (include/ptgpu.h)
    [[maybe_unused]] bool ls_run = false;
    [[maybe_unused]] uint32_t ls_k = 0, ls_m1 = 0, ls_m2 = 0;
    if constexpr (kLS) {
        ls_run = isD & (depth < kDepthLimit);
        uint32_t st_l = st;
        if (io.n_lights > 1)  // floor(u L) of u = m 2^-24, exactly
            ls_k = min((uint32_t)(io.n_lights - 1), (draw_bits(st_l) * (uint32_t)io.n_lights) >> 24);
        [[maybe_unused]] const uint32_t st_k = st_l;  // (after the light choice, which stays xorshift)
        ls_m1 = draw_bits(st_l);
        ls_m2 = draw_bits(st_l);
        if constexpr (kStrat) {
            ls_m1 = first ? fh.z : ls_m1;
            ls_m2 = first ? fh.w : ls_m2;
            st_l = first ? st_k : st_l;
        }
        st = ls_run ? st_l : st;
    }
    [[maybe_unused]] const bool sd = first & isD;  // (no roulette at depth 0: isD is the material)
    uint32_t m1;
    if constexpr (kStrat) {
        uint32_t st_a = st;
        const uint32_t mx = draw_bits(st_a);
        m1 = sd ? fh.x : mx;
        st = sd ? st : st_a;
    } else
    m1 = draw_bits(st);
    bool fres_refl = false;  // dielectric lane reflected by its Fresnel draw (isG & fres & reflect)
    // its value u = m1 2^-24, converted once for the diffuse phi (fast
    // mode: v_sin / v_cos take revolutions) and the Fresnel compare
    const float u1 = (float)m1 * 0x1p-24f;
    // every lane sets it below (exact mode: reflecting lanes in the spec
    // block; fast mode: the diffuse/dielectric block forms every material's
    // direction, the spec block serves the waves that skip it)
    f3 nd = d;
    // a wave with only mirror lanes skips the diffuse/dielectric work
    // (wave-uniform, exact: those lanes' values are all overwritten)
    // (the active lanes less the mirror lanes' mask, which the spec compare
    // above already formed: a ballot of isD | isG was materialised as
    // v_cndmask + v_cmp, one of mat != PTG_SPECULAR as another compare;
    // killed lanes of those materials run the block for nothing, their
    // values unused)
    const bool dg_wave = (__ballot(1) & ~__ballot(mat == PTG_SPECULAR)) != 0ull;
    if (dg_wave)
    {
        PTG_STAT(4);
#if PTG_BLOCK_STATS == 3  // debug: wave cycles of the diffuse/dielectric block in [14]
        const unsigned long long dg_t0 = clock64();
#endif
        {
        // the second xorshift step, once for every lane of the block: the
        // diffuse r and the draw of a reflection chosen by the Fresnel draw
        // are the same step of the same state (st right after m1).  The
        // lanes that take it -- diffuse, Fresnel-reflected -- adopt st2 in
        // the one select after the Fresnel block; killed, mirror, totally
        // reflected and refracting lanes keep st.
        uint32_t st2 = st;
        uint32_t m2 = draw_bits(st2);
        if constexpr (kStrat)
            m2 = sd ? fh.y : m2;
        // read only where isD (the ?: operands and the isD branch below):
        // no initial values to set for the other lanes
        float cp, sp, ra;
        if (isD) {  // main.cpp:46-47: phi = 2 pi u, r = u
            const uint32_t m_phi = m1;
            ra = (float)m2 * 0x1p-24f;  // draw()'s value of the shared step
            if constexpr (!kExact) {
                cp = __builtin_amdgcn_cosf(u1);  // Math<false>::sincos2pi of m1
                sp = __builtin_amdgcn_sinf(u1);
            } else
            Math<kExact>::sincos2pi(m_phi, trig, cp, sp);
        }
        // op1: diffuse -> u = norm((|w.x| > 0.1 ? y : x) x w) (main.cpp:52); dielectric -> norm(d) (main.cpp:75)
        f3 uu = __builtin_fabsf(nn.x) > 0.1f ? mk3(nn.z, 0.0f, -nn.x) : mk3(0.0f, -nn.z, nn.y);
        const f3 v1raw = isD ? uu : d;
        const float r1 = Math<kExact>::rsqrt(dot3(v1raw, v1raw));
        // (fast mode: the normalising multiply waits for the Fresnel block --
        // a reflecting lane keeps its d as it is; nothing before reads v1)
        [[maybe_unused]] f3 v1 = v1raw;
        if constexpr (kExact)
            v1 = mk3(v1raw.x * r1, v1raw.y * r1, v1raw.z * r1);
        // (fast mode: only dielectric lanes read x0, and there v1 = d r1, so
        // v1.nn = (nn.d) r1 = kn r1 -- the dot the mirror already uses)
        const float x0 = kExact ? -dot3(v1, nn) : -(kn * r1);
        // fast mode: one v_min_f32 (differs from the select only for NaN)
        const float cthG = kExact ? (1.0f < x0 ? 1.0f : x0) : __builtin_fminf(1.0f, x0);  // main.cpp:77
        // op2: diffuse -> sin theta = sqrt(r); dielectric -> sin theta = sqrt(1 - cos^2)
        // (fast mode: the argument is >= 0 on every lane that reads s2 --
        // ra >= 0, and 0 < x0 <= 1 + rounding on a dielectric lane (nn faces
        // the ray), so cthG <= 1 and 1 - cthG^2 >= 0 -- so sqrt0's clamp of
        // negative inputs is left out)
        const float s2 = kExact ? Math<kExact>::sqrt0(isD ? ra : __builtin_fmaf(-cthG, cthG, 1.0f))
                                : Math<kExact>::sqrt(isD ? ra : __builtin_fmaf(-cthG, cthG, 1.0f));
        const float ratio = front ? 0.5f : 2.0f;  // main.cpp:72
        // fast mode: ratio sin theta once, for the refraction test and |r_out_perp| below
        [[maybe_unused]] const float rs2 = kExact ? 0.0f : ratio * s2;
        if (isG) {
            bool reflect = (kExact ? ratio * s2 : rs2) > 1.0f;  // cannot refract: no Fresnel draw (main.cpp:89)
            if (!reflect) {
                const float r0 = 0x1.c71c74p-4f;  // ((1-ratio)/(1+ratio))^2, equal for ratio 0.5 and 2
                float xm = 1.0f - cthG;
                float x2 = xm * xm;
                float x5 = (x2 * x2) * xm;
                float R = __builtin_fmaf(1.0f - r0, x5, r0);
                reflect = R > u1;
                fres_refl = reflect;  // (the reflection's draw after this one: st2, selected below)
            }
            spec = reflect;
        }
        // one select for the shared second step (lane masks combined by the scalar unit)
        if constexpr (kStrat)
            st = ((isD & !sd) || fres_refl) ? st2 : st;
        else
        st = (isD || fres_refl) ? st2 : st;
        // op3: diffuse -> cos theta = sqrt(1 - r); dielectric -> |r_out_parallel| (main.cpp:94)
        if constexpr (!kExact) {
            // One direction for every material of the block, as a linear
            // combination of nn, vv = nn x v1 and v1:
            //   diffuse     nn s3 + vv ss + v1 cs                (main.cpp:53-55)
            //   reflection  d - 2 kn nn                          (main.cpp:60-67; v1 = d, not normalised)
            //   refraction  r_out_perp - nn s3 with r_out_perp = (nn cthG + v1) ratio (main.cpp:93-96),
            //               = nn (ratio cthG - s3) + v1 ratio
            // in the operation order of the diffuse line.  A diffuse lane
            // runs its earlier operations on its earlier values; so does a
            // reflecting lane (vv 0 + d 1 is d, then fma(nn, -2 kn, d)), the
            // mirror spheres' lanes included; a refracting lane rounds the
            // same vector differently (three roundings either way).  ratio
            // cthG - s3 does not cancel: entering (ratio 0.5) ratio cthG <=
            // 0.5 and s3 = sqrt(1 - sin^2 theta / 4) >= 0.866; leaving
            // (ratio 2) a lane refracts only where 2 sin theta <= 1, so
            // ratio cthG >= 1.732 and s3 <= 1.
            const float rsel = spec ? 1.0f : r1;  // spec is final here
            v1 = mk3(v1raw.x * rsel, v1raw.y * rsel, v1raw.z * rsel);
            // (nn and v1 are unit and v1.nn = -cos theta, so |r_out_perp|^2 =
            // ratio^2 (1 - cos^2 theta) = rs2^2 -- one fma for the dot and
            // its subtraction, r_out_perp itself never formed.  The one
            // assumption added: cthG is the un-clamped x0 wherever the clamp
            // does not bind, which is where s2^2 is 1 - x0^2; then rs2^2 and
            // |r_out_perp|^2 differ by roundings only.  Where it binds,
            // cthG = 1 and s2 = 0: the argument is 1, r_out_perp is within
            // rounding of 0.)
            const float gq = __builtin_fmaf(-rs2, rs2, 1.0f);
            const float s3 = Math<kExact>::sqrt(isD ? 1.0f - ra : __builtin_fabsf(gq));  // both arguments >= 0
            const f3 vv = cross3(nn, v1);
            const float k3r = -(kn + kn), k3t = __builtin_fmaf(ratio, cthG, -s3);
            const float K3 = isD ? s3 : (spec ? k3r : k3t);
            const float K2 = isD ? sp * s2 : 0.0f;
            const float K1 = isD ? cp * s2 : (spec ? 1.0f : ratio);
            // (written to d itself, whose last reader was v1: formed in
            // registers of its own, the result took three copies per
            // iteration to reach the loop-carried d)
            d = mk3(__builtin_fmaf(nn.x, K3, __builtin_fmaf(vv.x, K2, v1.x * K1)),
                    __builtin_fmaf(nn.y, K3, __builtin_fmaf(vv.y, K2, v1.y * K1)),
                    __builtin_fmaf(nn.z, K3, __builtin_fmaf(vv.z, K2, v1.z * K1)));
            nd = d;
        } else {
            const f3 perp = mk3(__builtin_fmaf(nn.x, cthG, v1.x) * ratio, __builtin_fmaf(nn.y, cthG, v1.y) * ratio,
                                __builtin_fmaf(nn.z, cthG, v1.z) * ratio);
            const float s3 = Math<kExact>::sqrt(isD ? 1.0f - ra : __builtin_fabsf(1.0f - dot3(perp, perp)));
            if (isD) {  // main.cpp:53-55 (unit by construction, not re-normalised)
                f3 vv = cross3(nn, v1);
                float cs = cp * s2, ss = sp * s2;
                nd = mk3(__builtin_fmaf(nn.x, s3, __builtin_fmaf(vv.x, ss, v1.x * cs)),
                         __builtin_fmaf(nn.y, s3, __builtin_fmaf(vv.y, ss, v1.y * cs)),
                         __builtin_fmaf(nn.z, s3, __builtin_fmaf(vv.z, ss, v1.z * cs)));
            } else {  // refraction, main.cpp:93-96
                nd = mk3(__builtin_fmaf(nn.x, -s3, perp.x), __builtin_fmaf(nn.y, -s3, perp.y),
                         __builtin_fmaf(nn.z, -s3, perp.z));
            }
        }
        }
#if PTG_BLOCK_STATS == 3
        {
            const unsigned long long dg_t1 = clock64();
            if (__lane_id() == __ffsll((long long)__ballot(1)) - 1)
                atomicAdd(&ptg_dbg_stats[(blockIdx.x & 255) * 16 + 14], dg_t1 - dg_t0);
        }
#endif
    }
    // fast mode: the block above formed the reflecting lanes' direction as
    // well, so the mirror's own code is that block's wave-uniform else -- a
    // wave of mirror lanes only (frequent in box_mirror's tube of mirror
    // walls); box waves never execute it
    if (kExact || !dg_wave)
    if (spec) {  // main.cpp:60-67 (fuzz draw consumed, multiplied by 0)
        PTG_STAT(5);
        // (fast mode: an empty statement that the compiler may not execute
        // speculatively -- without it the two tests above are folded into
        // one select and every wave runs this block's arithmetic again)
        if constexpr (!kExact)
            asm volatile("");
        // (fast mode: on the facing normal nn = +-on, its dot kn)
        float k = !kExact ? kn : dot3(on, d);
        k = k + k;
        // (the reflection's draw after a Fresnel draw: the block's shared second step)
        const f3 rn = !kExact ? nn : on;
        nd = mk3(__builtin_fmaf(-k, rn.x, d.x), __builtin_fmaf(-k, rn.y, d.y), __builtin_fmaf(-k, rn.z, d.z));
    }
    if constexpr (kLS) {
        io.skip_next = ls_run;
        io.to_shadow = false;
        if (ls_run) {
            const LightRec *lr = io.lights + ls_k;
            const float4 lc = lr->c, le = lr->e;
            const f3 w = mk3(lc.x - p.x, lc.y - p.y, lc.z - p.z);
            const float d2 = dot3(w, w);
            // (a point inside the light, d2 <= R^2 -- a dome light, a lamp of
            // emissive glass: nothing here; the next hit can only meet that
            // light from the back, where its emission is not skipped)
            if (d2 > lc.w && io.hid != __float_as_int(le.w)) {
                const float q = Math<kExact>::div(lc.w, d2);
                const float omc = Math<kExact>::div(q, 1.0f + Math<kExact>::sqrt0(1.0f - q));  // 1 - cos theta_max
                const float a = ((float)ls_m1 * 0x1p-24f) * omc;
                const float ct = 1.0f - a;
                const float sth = Math<kExact>::sqrt0(a * (2.0f - a));
                float cph, sph;
                Math<kExact>::sincos2pi(ls_m2, trig, cph, sph);
                const float iw = Math<kExact>::rsqrt(d2);
                const f3 sw = mk3(w.x * iw, w.y * iw, w.z * iw);
                // the diffuse sampler's basis rule (main.cpp:52) around sw
                const f3 su = norm3m<kExact>(__builtin_fabsf(sw.x) > 0.1f ? mk3(sw.z, 0.0f, -sw.x)
                                                                          : mk3(0.0f, -sw.z, sw.y));
                const f3 sv = cross3(sw, su);
                const float kc = cph * sth, ks = sph * sth;
                const f3 l = mk3(__builtin_fmaf(sw.x, ct, __builtin_fmaf(sv.x, ks, su.x * kc)),
                                 __builtin_fmaf(sw.y, ct, __builtin_fmaf(sv.y, ks, su.y * kc)),
                                 __builtin_fmaf(sw.z, ct, __builtin_fmaf(sv.z, ks, su.z * kc)));
                const float cs = dot3(nn, l);
                if (cs > 0.0f) {
                    const float wgt = ((cs + cs) * omc) * (float)io.n_lights;
                    ls.pend = mk3((T.x * le.x) * wgt, (T.y * le.y) * wgt, (T.z * le.z) * wgt);
                    ls.nd = nd;
                    ls.light = __float_as_int(le.w);
                    nd = l;
                    io.to_shadow = true;
                }
            }
        }
    }
    o = p;
    d = nd;
    return killed | (depth >= kDepthLimit);
}

// Slab row -> image (output) row for the band shard.
__host__ __device__ __forceinline__ int out_row_of(const KArgs &A, int slab_row)
{
    int band = slab_row / A.band_rows;
    return (band * A.shard_count + A.shard_rank) * A.band_rows + (slab_row - band * A.band_rows);
}

// Exact per-path quantisation (include/ptgpu.h "Sample accumulation").
// trunc(c * 2^32) for c in [0, 2^30] without double arithmetic: integer part
// and fraction * 2^32 are both exact in fp32, so this equals the oracle's
// (uint64_t)((double)c * 0x1p32) bit for bit.
// quant() is exact for c in [0, 2^30]; NaN and negative values become 0 and
// larger ones 2^30 -- the counting kernel reports such paths
// (PTG_FLAG_COUNT_NONFINITE), none are expected
__device__ __forceinline__ bool in_quant_range(float c) { return c >= 0.0f && c <= 0x1p30f; }
// the clip quant() applies, as a value (the second moment squares it)
__device__ __forceinline__ float quant_clip(float c) { return !(c >= 0.0f) ? 0.0f : (c > 0x1p30f ? 0x1p30f : c); }
__device__ __forceinline__ unsigned long long quant(float c)
{
    if (!(c >= 0.0f))
        return 0ull;
    if (c > 0x1p30f)
        c = 0x1p30f;
    float ip = __builtin_truncf(c);
    uint32_t hi = (uint32_t)ip;
    uint32_t lo = (uint32_t)((c - ip) * 0x1p32f);
    return ((unsigned long long)hi << 32) | lo;
}

// One work unit per wave: a pixel group (pixels_per_wave pixels of one slab
// row, all their sub-pixels = up to 64 "slots") x one chunk of samples.
// The unit's nv*cnt paths form a pool: every lane starts one path, and a lane
// whose path ends takes the next unstarted path of the pool (ballot + rank),
// so all lanes stay busy until the pool is empty.  Path radiance is
// accumulated exactly (u64) per slot in LDS and added to the global
// accumulator once per unit.
//
// The body of the render kernels.  kMoments (moments_kernel, progressive
// passes with PTG_FLAG_MOMENTS): every finished path also adds
// quant(cl(c) * cl(c)) of its components to a second per-slot LDS sum, added
// to the second HBM accumulator acc2 (laid out like A.acc) at unit end.
//
// kGather (gather_kernel, ptg_accumulate_active_device): the unit's pixels are
// an entry of the active list's unit table instead of a pixel group -- up to
// pixels_per_wave active pixels of one slab row, anywhere in the row.  Pixel p
// already holds n_p samples (the count slab); its slots' keys are shifted by
// n_p G once here, so that the unit's local samples [0, add_samples) draw what
// samples [n_p, n_p + add_samples) draw unshifted (sample_state(key + b G, s)
// == sample_state(key, b + s)); the main loop is the same.
struct GatherArgs {
    const int4 *units;              // unit table: {slab row, first index in the row's list, pixels, 0}
    const int *list;                // per slab row (stride W) its active x, ascending
    const int *counts;              // per slab pixel the samples it holds
    const unsigned long long *rec;  // device record {active pixels, active units}
    long long max_units;            // the launch covers units [0, min(rec[1], max_units)) ...
    int n_chunks;                   // ... x n_chunks chunks of lvl_chunk[0] samples, chunk-major
};
//
// kLS (the ls_* kernels, PTG_FLAG_LIGHT_SAMPLING with a non-empty light list):
// shade() may turn a lane's next segment into a shadow segment (LsLane, LsIo
// above).  Two more wave masks carry that state: smask, the lane's next
// segment is a shadow segment; nmask, its next hit skips the listed emitters.
// Shadow and bounce segments of different lanes share the scan iterations.
//
// kStrat (the *_strat kernels, PTG_FLAG_STRATIFIED): a path's four pairs
// (sobol_pairs.hpp) are formed with its camera ray, in the refill batch where
// the lanes work together, from the slot's twelve seeds in LDS (formed once
// with its key).  Pairs 0 and 1 go into the camera ray; pairs 2 and 3 ride
// with the prefetched ray (a third 16-byte row of the lane's record) and move
// into the lane's first-hit row lds_fh when the path starts, which shade()
// is handed in every iteration and reads at depth 0 only.
template <bool kCount, bool kBvh, bool kExact, bool kMoments, bool kGather = false, bool kLS = false,
          bool kStrat = false>
__device__ __forceinline__ void render_unit(const KArgs A, unsigned long long *const acc2,
                                            const GatherArgs G = GatherArgs{})
{
    constexpr int kWaves = kBlockOf<kBvh> / 64;
    __shared__ unsigned long long lds_acc[kWaves][64 * 3];
    __shared__ unsigned long long lds_acc2[kMoments ? kWaves : 1][kMoments ? 64 * 3 : 1];  // second moments
    __shared__ unsigned long long lds_key[kWaves][64];
    __shared__ uint32_t lds_pix[kWaves][64];  // slot -> x | sx << 20 | sy << 26
    // kStrat: per slot the seeds {sa, sb, sc} of pairs 0..3; per lane its path's first-hit values;
    // gather kernel: per slot the samples its pixel holds (the pairs take the absolute sample index)
    __shared__ uint4 lds_sob[kStrat ? kWaves : 1][kStrat ? 64 : 1][3];
    __shared__ uint4 lds_fh[kStrat ? kWaves : 1][kStrat ? 64 : 1];
    __shared__ uint32_t lds_held[kStrat && kGather ? kWaves : 1][kStrat && kGather ? 64 : 1];
    // sphere records staged once per workgroup in LDS (uniform-address
    // ds_read_b128 broadcasts in the scan, by-id gathers at hits); larger
    // scenes read geometry with wave-uniform scalar loads from L2/HBM instead
    constexpr bool kLdsGeo = !kBvh;  // linear scenes (<= kMaxLdsSpheres) live in LDS
    // dynamic LDS: n geometry records then n shading records (96 B/sphere),
    // sized at launch so small scenes keep 8 workgroups per CU
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    LinRec *lds_lin = reinterpret_cast<LinRec *>(dyn_lds);
    const LinRec *recs = A.lin;
    // linear kernel: the sin/cos table in LDS; the BVH kernel (latency bound
    // on its node loads) reads it from global memory (L1): measured the same
    const float2 *trig = A.trig;
    if constexpr (kLdsGeo) {
        if constexpr (kExact) {  // (the fast mode's v_sin/v_cos need no table)
            __shared__ float2 lds_trig[kTrigEntries];
            for (int i = threadIdx.x; i < kTrigEntries; i += kBlock)
                lds_trig[i] = A.trig[i];
            trig = lds_trig;
        }
        for (int i = threadIdx.x; i <= A.n + 1 + 2; i += kBlock)  // n records + the sentinel + the wall table(s)
            lds_lin[i] = A.lin[i];
        recs = lds_lin;
    }
    __shared__ float4 lds_cam[4];
    // a starting path's T, depth and E, read in paths_done (linear kernel: 2
    // LDS reads and a move for 7 moves, box -0.9 %; the BVH kernel, bound by
    // its node loads, keeps the moves: C5 +0.3 % with the reads)
    constexpr bool kStartLds = !kBvh;
    __shared__ float4 lds_start[kStartLds ? 2 : 1];
    __shared__ int lds_coop_done;  // cooperative levels: waves of the workgroup finished
    if (threadIdx.x == 0) {
        lds_coop_done = 0;
        if constexpr (kStartLds) {
            lds_start[0] = make_float4(1.0f, 1.0f, 1.0f, __int_as_float(0));
            lds_start[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        const CamC c = cam_of(A);
        lds_cam[0] = c.p;
        lds_cam[1] = c.b;
        lds_cam[2] = c.X;
        lds_cam[3] = c.Y;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // wave-uniform by construction; readfirstlane lets the compiler keep all
    // per-unit bookkeeping in SGPRs
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long unit = (long long)blockIdx.x * kWaves + wv;
    if (unit >= A.n_units)
        return;  // whole wave
    // unit -> level (wave-uniform: a few scalar compares) -> pixel group and
    // sample chunk; chunk-major within a level (neighbours are different
    // pixel groups)
    int lv = 0;
    while (lv + 1 < A.n_levels && unit >= A.lvl_unit[lv + 1])
        ++lv;
    const long long t = unit - A.lvl_unit[lv];
    const int nlg = A.lvl_group[lv + 1] - A.lvl_group[lv];
    const bool coop = A.lvl_coop[lv] != 0;  // wave wv of the workgroup takes chunk wv of one pixel group
    const int ps = A.lvl_psplit[lv];        // units per pixel group (pixel-split level) or 1
    const long long nlu = (long long)nlg * ps;  // units per sample chunk
    // part-major like chunk-major: neighbouring units are different pixel groups
    const long long tg = coop ? t / kWaves : t % nlu;
    const int group = A.lvl_group[lv] + (int)(coop ? tg : tg % nlg);
    const int part = coop ? 0 : (int)(tg / nlg);
    const int len = A.lvl_chunk[lv];
    int s0 = A.sample_begin + (int)(coop ? t % kWaves : t / nlu) * len;
    int4 ent = make_int4(0, 0, 0, 0);
    if constexpr (kGather) {
        // the true unit count is the device's (scalar loads, like the table
        // entry: everything here is wave-uniform); a wave past it exits
        long long n_au = (long long)G.rec[1];
        n_au = n_au < G.max_units ? n_au : G.max_units;
        if (unit >= n_au * G.n_chunks)
            return;  // whole wave
        // (the 64-bit division runs on the vector unit: its results back to SGPRs)
        const long long cq = unit / n_au;
        const int c = __builtin_amdgcn_readfirstlane((int)cq);                // < n_chunks
        const int u = __builtin_amdgcn_readfirstlane((int)(unit - cq * n_au));  // < n_au <= n_groups
        ent = G.units[u];
        ent.x = __builtin_amdgcn_readfirstlane(ent.x);
        ent.y = __builtin_amdgcn_readfirstlane(ent.y);
        ent.z = __builtin_amdgcn_readfirstlane(ent.z);
        s0 = c * len;  // local samples [0, add_samples) = [sample_begin, sample_end)
    }
    if (s0 >= A.sample_end)
        return;  // whole wave: alignment padding before a cooperative level
#if PTG_UNIT_TRACE
    const unsigned long long trace_t0 = wall_clock64();
#endif
    // the unit holds every sample of its pixels: resolve in the wave
    const bool in_wave = A.lvl_inwave[lv] != 0;
    const int slab_row = kGather ? ent.x : group / A.waves_per_row;
    const int xblk = group - slab_row * A.waves_per_row;
    const int r = out_row_of(A, slab_row);
    const int y = A.H - 1 - r;  // main.cpp:181: y = 0 is the bottom row
    // the unit's pixels: x0, x0 + ps, ... (ps = 1: a contiguous group)
    const int x0 = xblk * A.pixels_per_wave + part;
    int npix = (A.pixels_per_wave - part + ps - 1) / ps;
    const int left = A.W - x0 > 0 ? (A.W - x0 + ps - 1) / ps : 0;
    npix = npix < left ? npix : left;
    if constexpr (kGather)
        npix = ent.z;  // (x0 is not used: the slots' x come from the list)
    const int nv = r < A.H ? npix * A.lanes_per_pixel : 0;  // valid slots are a prefix
    int cnt = A.sample_end - s0;
    cnt = cnt < len ? cnt : len;
    const int total = nv * cnt;

    lds_acc[wv][lane] = 0ull;
    lds_acc[wv][lane + 64] = 0ull;
    lds_acc[wv][lane + 128] = 0ull;
    if constexpr (kMoments) {
        lds_acc2[wv][lane] = 0ull;
        lds_acc2[wv][lane + 64] = 0ull;
        lds_acc2[wv][lane + 128] = 0ull;
    }
    if (lane < nv) {
        int px = x0 + (lane / A.lanes_per_pixel) * ps;
        if constexpr (kGather)
            px = G.list[(size_t)slab_row * A.W + ent.y + lane / A.lanes_per_pixel];
        int sub = lane % A.lanes_per_pixel;
        int sy = sub / A.nsub;
        int sx = sub - sy * A.nsub;
        const uint64_t pix_sub = ((uint64_t)y * (uint64_t)A.W + (uint64_t)px) * (uint64_t)A.lanes_per_pixel + (uint64_t)sub;
        uint64_t key = key_hash(A.seed, pix_sub);
        if constexpr (kStrat) {  // (from the sub-pixel's own key: the gather kernel's shift is not part of it)
            const sobol::Seeds q0 = sobol::seeds_of(key, 0), q1 = sobol::seeds_of(key, 1), q2 = sobol::seeds_of(key, 2),
                               q3 = sobol::seeds_of(key, 3);
            lds_sob[wv][lane][0] = make_uint4(q0.sa, q0.sb, q0.sc, q1.sa);
            lds_sob[wv][lane][1] = make_uint4(q1.sb, q1.sc, q2.sa, q2.sb);
            lds_sob[wv][lane][2] = make_uint4(q2.sc, q3.sa, q3.sb, q3.sc);
            if constexpr (kGather)
                lds_held[wv][lane] = (uint32_t)G.counts[(size_t)slab_row * A.W + px];
        }
        if constexpr (kGather)
            key += (uint64_t)(uint32_t)G.counts[(size_t)slab_row * A.W + px] * 0x9E3779B97F4A7C15ull;
        lds_key[wv][lane] = key;
        lds_pix[wv][lane] = (uint32_t)px | ((uint32_t)sx << 20) | ((uint32_t)sy << 26);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

    int slot = 0;
    f3 o, d, T, E;
    int depth = 0;
    uint32_t st = 0;
    uint32_t segs = 0;  // scene scans executed by this lane
    ScanCount scnt;     // BVH sphere/box tests (counting kernel)
    // Each lane keeps its NEXT path's camera ray prefetched in LDS: a lane
    // whose path ends starts the prefetched one at once (two LDS reads), and
    // the camera code runs only in refills of >= PTG_REFILL_BATCH lanes (or
    // when a lane would otherwise idle).
    __shared__ float4 lds_pre[kWaves][64][kStrat ? 3 : 2];
    // the lane's own record.  BVH kernel: its address formed at each use
    // (v_mbcnt of an opaque all-ones mask: not hoisted), not held in a VGPR
    // for the unit -- at 64 VGPRs it had been spilled and reloaded in the main
    // loop (C5 -0.3 %; the linear kernel, with VGPRs to spare, is 1.4 % slower
    // that way)
    auto pre_rec = [&]() -> float4 * {
        if constexpr (kBvh) {
            unsigned ones = ~0u;
            asm volatile("" : "+s"(ones));
            const unsigned ln = __builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
            return lds_pre[wv][ln];
        } else {
            return lds_pre[wv][lane];
        }
    };
    // it / nv and it % nv (only for a unit of fewer than 64 slots; it <
    // 64 * kMaxChunk = 2^22, so the float quotient is within 1 of it / nv and
    // one correction step is exact) through a float reciprocal formed at
    // each use: the compiler's
    // integer division by the unit's nv kept its constants in VGPRs for the
    // whole unit (spilled to scratch)
    auto divmod_nv = [&](int it, int &q, int &r) {
        int n = nv;
        asm volatile("" : "+s"(n));
        q = (int)((float)it * __builtin_amdgcn_rcpf((float)n));
        r = it - q * n;
        q = r < 0 ? q - 1 : (r >= n ? q + 1 : q);
        r = r < 0 ? r + n : (r >= n ? r - n : r);
    };
    // the lane's first-hit row (kStrat), addressed like its record
    [[maybe_unused]] auto fh_row = [&]() -> uint4 * {
        if constexpr (kBvh) {
            unsigned ones = ~0u;
            asm volatile("" : "+s"(ones));
            const unsigned ln = __builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
            return &lds_fh[wv][ln];
        } else {
            return &lds_fh[wv][lane];
        }
    };
    auto ray_of = [&](int it, f3 &ro, f3 &rd, uint32_t &rs, [[maybe_unused]] uint4 &fh) {
        int sl, sample;
        if (nv == 64) {
            sl = it & 63;
            sample = s0 + (it >> 6);
        } else {
            int q;
            divmod_nv(it, q, sl);
            sample = s0 + q;
        }
        Lane L;
        uint32_t pk = lds_pix[wv][sl];
        L.x = (int)(pk & 0xFFFFFu);
        int yy = y;  // opaque: (float)y is converted here, not held in a VGPR for the unit
        asm volatile("" : "+s"(yy));
        L.y = yy;
        L.sx = (int)((pk >> 20) & 63u);
        L.sy = (int)(pk >> 26);
        L.key = lds_key[wv][sl];
        // the index is opaque to the compiler, so the reads stay here
        // instead of being hoisted into registers live for the whole unit
        int ci = 0;
        asm volatile("" : "+v"(ci));
        const CamC C{lds_cam[ci], lds_cam[ci + 1], lds_cam[ci + 2], lds_cam[ci + 3]};
        if constexpr (kStrat) {
            uint32_t sabs = (uint32_t)sample;
            if constexpr (kGather)
                sabs += lds_held[wv][sl];
            const uint32_t brs = sobol::brev(sabs);
            const uint4 a = lds_sob[wv][sl][0], b = lds_sob[wv][sl][1], c = lds_sob[wv][sl][2];
            uint4 cq;
            sobol::pair_brev(sobol::Seeds{a.x, a.y, a.z}, brs, cq.x, cq.y);
            sobol::pair_brev(sobol::Seeds{a.w, b.x, b.y}, brs, cq.z, cq.w);
            sobol::pair_brev(sobol::Seeds{b.z, b.w, c.x}, brs, fh.x, fh.y);
            sobol::pair_brev(sobol::Seeds{c.y, c.z, c.w}, brs, fh.z, fh.w);
            camera_ray<true>(C, L, (uint32_t)sample, rs, ro, rd, cq);
        } else
        camera_ray(C, L, (uint32_t)sample, rs, ro, rd);
    };
    // (BVH scenes: a started ray is fresh -- in neither of the main loop's
    // scan-phase masks, which its lane has left by then)
    auto begin = [&](int it, f3 ro, f3 rd, uint32_t rs, [[maybe_unused]] const uint4 fh) {
        if constexpr (kStrat)
            *fh_row() = fh;
        if (nv == 64) {
            slot = it & 63;
        } else {
            int q;
            divmod_nv(it, q, slot);
        }
        o = ro;
        d = rd;
        st = rs;
        T = mk3(1.0f, 1.0f, 1.0f);
        E = mk3(0.0f, 0.0f, 0.0f);
        depth = 0;
    };
    auto store_pre = [&](int it, f3 ro, f3 rd, uint32_t rs, [[maybe_unused]] const uint4 fh) {
        float4 *rec = pre_rec();
        if constexpr (kStrat)
            rec[2] = make_float4(__uint_as_float(fh.x), __uint_as_float(fh.y), __uint_as_float(fh.z), __uint_as_float(fh.w));
        rec[0] = make_float4(ro.x, ro.y, rd.x, rd.y);
        // ro.z (= the camera's z, the lens offset has no z) rides in the
        // record's last word: read back with the ray, not as a kernel
        // argument (a scalar load + wait in the path-start block)
        rec[1] = make_float4(rd.z, __uint_as_float(rs), __int_as_float(it), ro.z);
    };
    // the lanes' loop state as wave masks (SGPRs, updated by the scalar unit
    // at wave level; a lane's bit read with inverse_ballot): kept per lane,
    // the bools lived in VGPRs and every iteration re-formed their lane masks
    // with compares.  hmask: a prefetched ray in LDS; wmask: path ended, no
    // prefetched ray yet (E kept until the batch); pmask: a finished path's
    // radiance parked in the lane's LDS record; amask: the lane holds a path
    // (the scalar unit sets it at unit start, clears a bit where a path ends
    // with no prefetched ray to start, sets it where refill starts an idle
    // lane; a lane in wmask is not in amask)
    unsigned long long hmask = 0ull, wmask = 0ull, pmask = 0ull;
    unsigned long long amask = __ballot(lane < total);
    auto lane_in = [](unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); };
    // light sampling: the lane's shadow-segment state and its two masks (a
    // path that ends leaves both bits clear, so a started path begins clear)
    [[maybe_unused]] LsLane ls{};
    [[maybe_unused]] unsigned long long smask = 0ull, nmask = 0ull;
    auto ls_io = [&]() {  // (at wave level: every lane reads its bits)
        LsIo io{};
        if constexpr (kLS) {
            io.lights = A.lights;
            io.n_lights = A.n_lights;
            io.shadow = lane_in(smask);
            io.skip = lane_in(nmask);
        }
        return io;
    };
    if (lane < total) {
        f3 ro, rd;
        uint32_t rs;
        uint4 fh{};
        ray_of(lane, ro, rd, rs, fh);
        begin(lane, ro, rd, rs, fh);
    }
    if (64 + lane < total) {
        f3 ro, rd;
        uint32_t rs;
        uint4 fh{};
        ray_of(64 + lane, ro, rd, rs, fh);
        store_pre(64 + lane, ro, rd, rs, fh);
    }
    hmask = __ballot(64 + lane < total);
    int next = total < 128 ? total : 128;  // wave-uniform pool cursor
    uint32_t bad = 0;  // counting kernel: paths with a NaN / negative / > 2^30 radiance component
    auto flush = [&](float ex, float ey, float ez, int sl) {
        if constexpr (kCount)
            bad += (in_quant_range(ex) && in_quant_range(ey) && in_quant_range(ez)) ? 0u : 1u;
        atomicAdd(&lds_acc[wv][sl], quant(ex));
        atomicAdd(&lds_acc[wv][sl + 64], quant(ey));
        atomicAdd(&lds_acc[wv][sl + 128], quant(ez));
        if constexpr (kMoments) {
            const float cx = quant_clip(ex), cy = quant_clip(ey), cz = quant_clip(ez);
            atomicAdd(&lds_acc2[wv][sl], quant(cx * cx));
            atomicAdd(&lds_acc2[wv][sl + 64], quant(cy * cy));
            atomicAdd(&lds_acc2[wv][sl + 128], quant(cz * cz));
        }
    };
    // A finished path parks its radiance (E, slot) in the lane's LDS record
    // lds_pre[wv][lane], which just gave up its prefetched ray; the quantise +
    // LDS adds run for all parked lanes at the next refill batch (before the
    // refill writes new prefetched rays there).  A lane that finishes again
    // before the batch has no prefetched ray: it waits (E in registers),
    // which forces a batch; there its E is parked, and it starts a new ray.
    auto park = [&]() { pre_rec()[0] = make_float4(E.x, E.y, E.z, __int_as_float(slot)); };
    auto flush_parked = [&]() {
        const float4 pk = pre_rec()[0];
        flush(pk.x, pk.y, pk.z, __float_as_int(pk.w));
    };
    // path end of the lanes in done (a wave mask): park the radiance and
    // start the prefetched ray, or wait
    auto paths_done = [&](const unsigned long long done) {
        if (done == 0ull)
            return;
        const unsigned long long start = done & hmask;
        if (lane_in(start)) {
            const float4 *rec = pre_rec();
            const float4 p0 = rec[0], p1 = rec[1];
            [[maybe_unused]] uint4 fh{};
            if constexpr (kStrat) {  // the started path's first-hit values: from its record to the lane's row
                const float4 p2 = rec[2];
                fh = make_uint4(__float_as_uint(p2.x), __float_as_uint(p2.y), __float_as_uint(p2.z), __float_as_uint(p2.w));
            }
            park();
            if constexpr (kStartLds) {
                // T, depth and E read from the workgroup's constant record
                // (uniform address; the offset is opaque so the reads stay
                // here), issued behind the ray's reads and the park: one
                // wait for all of them, and the values land in the
                // loop-carried registers without copies
                unsigned so = 0;  // (a byte offset: no shift to scale an index)
                asm volatile("" : "+v"(so));
                const float4 *sc = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(lds_start) + so);
                const float4 c0 = sc[0], c1 = sc[1];
                if constexpr (kStrat)
                    *fh_row() = fh;
                if (nv == 64) {
                    slot = __float_as_int(p1.z) & 63;
                } else {
                    int q;
                    divmod_nv(__float_as_int(p1.z), q, slot);
                }
                o = mk3(p0.x, p0.y, p1.w);
                d = mk3(p0.z, p0.w, p1.x);
                st = __float_as_uint(p1.y);
                T = mk3(c0.x, c0.y, c0.z);
                depth = __float_as_int(c0.w);
                E = mk3(c1.x, c1.y, c1.z);
            } else {
                begin(__float_as_int(p1.z), mk3(p0.x, p0.y, p1.w), mk3(p0.z, p0.w, p1.x), __float_as_uint(p1.y), fh);
            }
        }
        pmask |= start;
        hmask &= ~start;
        wmask |= done & ~start;
        amask &= ~done | start;
    };
    // refill batch: flush parked paths, prefetch camera rays for lanes
    // without one, start idle lanes
    auto refill = [&]() {
        if (next < total) {
            const unsigned long long need = __ballot(1) & ~hmask;
            const int nn = (int)__popcll(need);
            if (nn >= PTG_REFILL_BATCH || wmask != 0ull) {
                PTG_STAT(6);
#if PTG_BLOCK_STATS == 3
                PTG_SUB_T(rf_t0);
#endif
                const unsigned long long idle = ~amask;  // (waiting lanes included)
                if (lane_in(pmask))
                    flush_parked();
                if (lane_in(wmask))
                    park();
                pmask = wmask;
                wmask = 0ull;
#if PTG_BLOCK_STATS == 3
                PTG_SUB_T(rf_t1);
                unsigned long long rf_ray = 0;
#endif
                // lanes of need below this one (v_mbcnt: no 64-bit lane mask held in VGPRs)
                const int ni = next + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32),
                                                                     __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
                const unsigned long long got = need & __ballot(ni < total);
                if (lane_in(got)) {
                    f3 ro, rd;
                    uint32_t rs;
                    uint4 fh{};
#if PTG_BLOCK_STATS == 3
                    PTG_SUB_T(rr_t0);
#endif
                    ray_of(ni, ro, rd, rs, fh);
#if PTG_BLOCK_STATS == 3
                    rf_ray = clock64() - rr_t0;
#endif
                    if (lane_in(idle))  // idle lane: start it now (its record may hold a parked path)
                        begin(ni, ro, rd, rs, fh);
                    else
                        store_pre(ni, ro, rd, rs, fh);
                }
                hmask |= got & ~idle;
                amask |= got & idle;
                next += nn;
#if PTG_BLOCK_STATS == 3
                {
                    const unsigned long long rf_t2 = clock64();
                    unsigned long long ray_max = rf_ray;  // the wave's camera-ray time: its slowest lane's span
                    for (int off = 32; off > 0; off >>= 1)
                        ray_max = max(ray_max, (unsigned long long)__shfl_xor(ray_max, off, 64));
                    PTG_SUB_ADD(0, 1ull);
                    PTG_SUB_ADD(1, rf_t1 - rf_t0);
                    PTG_SUB_ADD(2, ray_max);
                    PTG_SUB_ADD(3, (rf_t2 - rf_t1) - ray_max);
                }
#endif
            }
        } else if (wmask != 0ull) {  // pool exhausted: nothing left for this lane
            if (lane_in(wmask))
                flush(E.x, E.y, E.z, slot);
            wmask = 0ull;
        }
    };
    if constexpr (!kBvh) {
#if PTG_BLOCK_STATS == 3  // debug: wave cycles of the linear kernel's scan / shade / refill / loop control
        unsigned long long ph_cyc[6] = {0, 0, 0, 0, 0, 0}, ph_t = clock64();
        auto lin_phase = [&](int i) {
            const unsigned long long t_ = clock64();
            ph_cyc[i] += t_ - ph_t;
            ph_t = t_;
        };
#endif
        for (;;) {
            if ((amask | wmask) == 0ull)
                break;
            PTG_STAT(0);
#if PTG_BLOCK_STATS == 3
            lin_phase(5);
            float t3 = 0.0f;
            const LinRec *w3 = nullptr;
            if (lane_in(amask)) {
                if constexpr (kCount)
                    segs += 1;
                w3 = scene_scan<kExact, kCount>(A, recs, o, d, t3, scnt);
            }
            lin_phase(0);
            paths_done(__ballot(lane_in(amask) && shade<kExact>(w3 != recs + A.n ? &w3->s : nullptr, t3, trig, o, d, T, E, depth, st)));
            lin_phase(3);
            refill();
            lin_phase(4);
#else
            bool done = false;
            [[maybe_unused]] LsIo io = ls_io();
            [[maybe_unused]] uint4 fh{};
            if constexpr (kStrat)  // (at wave level, unconditionally: selected in shade)
                fh = *fh_row();
            if (lane_in(amask)) {
                PTG_STAT(1);
                if constexpr (kCount)
                    segs += 1;
                if constexpr (kStrat)
                    done = segment<kBvh, kExact, kCount, kLS, true>(A, recs, trig, o, d, T, E, depth, st, scnt, ls, io, fh);
                else if constexpr (kLS)
                    done = segment<kBvh, kExact, kCount, true>(A, recs, trig, o, d, T, E, depth, st, scnt, ls, io);
                else
                done = segment<kBvh, kExact, kCount>(A, recs, trig, o, d, T, E, depth, st, scnt);
            }
            if constexpr (kLS) {  // every active lane was shaded: its bits anew (idle lanes: clear)
                smask = __ballot(io.to_shadow);
                nmask = __ballot(io.skip_next);
            }
            paths_done(__ballot(done));
            refill();
#endif
        }
#if PTG_BLOCK_STATS == 3
        if (lane == 0)
            for (int k = 0; k < 6; ++k)
                atomicAdd(&ptg_dbg_stats[(blockIdx.x & 255) * 16 + 8 + k], ph_cyc[k]);
#endif
    } else {
        // BVH scenes: each lane is fresh (ray set, scan not started), walking
        // or ready (scan done, to be shaded); an iteration starts the fresh
        // lanes' scans, walks until enough lanes are ready (PTG_READY_FRAC/8
        // of the active lanes) or none walks, shades the ready lanes.
        BvhTrav tr{};  // started per segment by bvh_start
        unsigned long long wk = 0ull, rd = 0ull;  // walking / scan done (see the loop)
#if PTG_LEAF_SPLIT
        __shared__ uint8_t lds_pair[kWaves][2][64];  // leaf phase: owner / helper lane of each rank
#endif
        // kernel-argument pointers used in the loops, pinned in SGPRs once:
        // left to the compiler they were re-loaded (s_load + wait) in every
        // node step and every shade
        gptr<u32x4> qnodes = (gptr<u32x4>)A.bvh_qnodes;
        asm volatile("" : "+s"(qnodes));
        gptr<int> cont = (gptr<int>)A.bvh_cont;
        asm volatile("" : "+s"(cont));
        if constexpr (kExact)  // (the fast mode's sin/cos read no table)
            asm volatile("" : "+s"(trig));
#if PTG_BLOCK_STATS == 2
        unsigned long long ph_cyc[6] = {0, 0, 0, 0, 0, 0}, ph_t = clock64();
#endif
        for (;;) {
            if ((amask | wmask) == 0ull)
                break;
            PTG_PHASE(5);
            // the lanes' scan phase as wave masks (like hmask / wmask / pmask):
            // wk walking, rd scan done (to be shaded); a fresh lane is active
            // and in neither.  A lane's scan is done when ni == -1 and no leaf
            // is parked: two single-compare ballots (a ballot of the combined
            // predicate is materialised as v_cndmask + v_cmp)
            const unsigned long long act = amask;
            {
                const unsigned long long fresh = act & ~(wk | rd);
                if (lane_in(fresh)) {
                    if constexpr (kCount)
                        segs += 1;
                    bvh_start<kCount && !PTG_WAVE_STATS, kExact>(A, o, d, tr, scnt);
                }
                const unsigned long long fin = fresh & __ballot(tr.ni == -1) & __ballot(tr.pend < 0);
                rd |= fin;
                wk |= fresh & ~fin;
            }
            PTG_PHASE(0);
            {
                const SlabRay sr = slab_ray(A, o, d);
                const int na = (int)__popcll(act);
                // Node steps in an inner loop, the leaf phase in the outer one:
                // with both in one loop body, the merge of the two branches'
                // traversal states cost 14+ v_mov per node step (the compiler
                // copied the 7 state registers out and back in; C5 -1.5 %).
                for (;;) {
                    unsigned long long mhas = 0ull;
                    bool walk_done = false;
                    for (;;) {
                        // ballots of single compares: a ballot of a combined
                        // predicate (x && y) is materialised as v_cndmask + v_cmp,
                        // 2 VALU each.  A walking lane is in amask (a path
                        // ends only in shading, after the walk), and na does not
                        // change inside the walk.
                        const unsigned long long mt = wk;
                        const int nt = (int)__popcll(mt);
                        if (mt == 0ull || 8 * (na - nt) >= PTG_READY_FRAC * na) {
                            walk_done = true;
                            break;
                        }
                        mhas = __ballot(tr.pend >= 0) & mt;  // walking lanes holding a leaf
                        if (8 * (int)__popcll(mhas) >= PTG_LEAF_FRAC * nt)
                            break;  // leaf phase
#if PTG_WAVE_STATS == 1  // debug: wave-level node steps (first active lane only)
                        if constexpr (kCount)
                            scnt.boxes += __lane_id() == __ffsll((long long)__ballot(1)) - 1 ? 1 : 0;
#endif
                        PTG_PHASE(5);
                        // (the node step as selects for the whole wave, like the
                        // leaf completion: +2.3 % -- its loads and selects for idle lanes)
                        if (lane_in(mt & ~mhas))
                            bvh_node_step<kCount && !PTG_WAVE_STATS>(cont, qnodes, sr, tr, scnt);
                        PTG_PHASE(1);
                        {
                            const unsigned long long fin = wk & __ballot(tr.ni == -1) & __ballot(tr.pend < 0);
                            rd |= fin;
                            wk &= ~fin;
                        }
                    }
                    if (walk_done)
                        break;
                    // leaf phase (round 1: spreading the parked leaves' spheres over
                    // the whole wave with ds_bpermute + LDS atomicMin measured 1.7 %
                    // slower; pairing idle lanes with the long leaves 1.2-1.5 % faster)
#if PTG_LEAF_SPLIT
                    bvh_leaf_split<kCount && !PTG_WAVE_STATS, kExact>(A, cont, o, d, lane_in(mhas), mhas, tr, scnt,
                                                               lds_pair[wv]);
#else
                    if (lane_in(mhas))
                        bvh_leaf<kCount && !PTG_WAVE_STATS, kExact>(A, cont, o, d, tr, scnt);
#endif
                    PTG_PHASE(2);
                    {
                        const unsigned long long fin = wk & __ballot(tr.ni == -1) & __ballot(tr.pend < 0);
                        rd |= fin;
                        wk &= ~fin;
                    }
                }
            }
#if PTG_WAVE_STATS == 2  // debug: wave-level main-loop iterations / iterations that shade (first active lane)
            if constexpr (kCount) {
                const bool first_lane = __lane_id() == __ffsll((long long)__ballot(1)) - 1;
                scnt.boxes += first_lane ? 1 : 0;
                scnt.spheres += (first_lane && rd != 0ull) ? 1 : 0;
            }
#endif
            PTG_PHASE(5);
            bool done = false;
            const unsigned long long shade_m = rd;
            rd = 0ull;
            [[maybe_unused]] LsIo io = ls_io();
            [[maybe_unused]] uint4 fh{};
            if constexpr (kStrat)
                fh = *fh_row();
            if (lane_in(shade_m)) {
                const int sid = tr.best;
                const ShadeRec *hrec = sid >= 0 ? A.shade + sid : nullptr;
                if constexpr (kStrat) {
                    io.hid = sid;
                    done = shade<kExact, kLS, true>(hrec, tr.tb, trig, o, d, T, E, depth, st, ls, io, fh);
                } else if constexpr (kLS) {
                    io.hid = sid;
                    done = shade<kExact, true>(hrec, tr.tb, trig, o, d, T, E, depth, st, ls, io);
                } else
                done = shade<kExact>(hrec, tr.tb, trig, o, d, T, E, depth, st);
            }
            if constexpr (kLS) {  // the shaded lanes' bits anew; a lane still walking keeps its own
                smask = (smask & ~shade_m) | __ballot(io.to_shadow);
                nmask = (nmask & ~shade_m) | __ballot(io.skip_next);
            }
            paths_done(__ballot(done));
            PTG_PHASE(3);
            refill();
            PTG_PHASE(4);
        }
#if PTG_BLOCK_STATS == 2
        if (lane == 0)
            for (int k = 0; k < 6; ++k)
                atomicAdd(&ptg_dbg_stats[(blockIdx.x & 255) * 16 + 8 + k], ph_cyc[k]);
#endif
    }
    if (lane_in(pmask))
        flush_parked();
    // the lane index re-formed here (v_mbcnt of an opaque all-ones mask):
    // taken from the work-item id it was held, and spilled, through the main
    // loop for the epilogue's uses
    const int lane_e = [] {
        unsigned ones = ~0u;
        asm volatile("" : "+s"(ones));
        return (int)__builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
    }();
    if constexpr (kCount) {
        unsigned long long ws = segs, wsph = scnt.spheres, wbox = scnt.boxes, wbad = bad;
        for (int off = 32; off > 0; off >>= 1) {
            ws += __shfl_xor(ws, off, 64);
            wsph += __shfl_xor(wsph, off, 64);
            wbox += __shfl_xor(wbox, off, 64);
            wbad += __shfl_xor(wbad, off, 64);
        }
        if (lane_e == 0 && A.count_nonfinite && wbad)
            atomicAdd(A.segments + 3, wbad);
        if (lane_e == 0 && ws)
            atomicAdd(A.segments, ws);
        if (lane_e == 0 && A.count_tests) {
            atomicAdd(A.segments + 1, wsph);
            atomicAdd(A.segments + 2, wbox);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    bool coop_last = false;
    if (coop) {
        // publish this wave's sums (its LDS adds are complete), count it; the
        // wave that completes the count adds every wave's sums and resolves
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        int prev = 0;
        if (lane_e == 0)
            prev = __hip_atomic_fetch_add(&lds_coop_done, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        prev = __shfl(prev, 0, 64);
        coop_last = prev == kWaves - 1;
        if (!coop_last) {
            PTG_TRACE_END();
            return;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (in_wave || coop_last) {
        // the unit (or the workgroup) holds every sample of its pixels:
        // resolve here (main.cpp:195-196, same arithmetic as resolve_kernel)
        // and write 12 B per pixel -- the only HBM traffic of the frame
        if (lane_e < npix && r < A.H) {
            f3 pix = mk3(0.0f, 0.0f, 0.0f);
            for (int j = 0; j < A.lanes_per_pixel; ++j) {
                const int sl = lane_e * A.lanes_per_pixel + j;
                float m[3];
                for (int c = 0; c < 3; ++c) {
                    unsigned long long sum = lds_acc[wv][sl + 64 * c];
                    if (coop_last) {
                        sum = 0ull;
                        for (int w = 0; w < kWaves; ++w)  // exact: integer sums in any order
                            sum += lds_acc[w][sl + 64 * c];
                    }
                    const float mean = A.samps > 0 ? (float)(((double)sum * 0x1p-32) / (double)A.samps) : 0.0f;
                    m[c] = mean < 0.0f ? 0.0f : (1.0f < mean ? 1.0f : mean);
                }
                pix = mk3(__builtin_fmaf(m[0], A.inv_sub2, pix.x), __builtin_fmaf(m[1], A.inv_sub2, pix.y),
                          __builtin_fmaf(m[2], A.inv_sub2, pix.z));
            }
            // opaque lane: the address is formed here, not hoisted to the
            // unit start and held (spilled) in VGPRs through the main loop
            int ln = lane_e;
            asm volatile("" : "+v"(ln));
            float *out = A.out + ((size_t)slab_row * A.W + x0 + ln * ps) * 3;
            out[0] = pix.x;
            out[1] = pix.y;
            out[2] = pix.z;
        }
    } else if (lane_e < nv) {
        // several units share these pixels: exact u64 adds, resolved later
        // opaque: the address is formed here, not held in VGPRs for the unit
        int ln = lane_e, row = slab_row, px0 = x0;
        asm volatile("" : "+v"(ln), "+s"(row), "+s"(px0));
        unsigned long long *g = A.acc + (((size_t)row * A.W + px0) * A.lanes_per_pixel + ln) * 3;
        size_t gi = 0;
        if constexpr (kGather) {  // each slot's own pixel
            gi = ((size_t)row * A.W + (lds_pix[wv][ln] & 0xFFFFFu)) * A.lanes_per_pixel + ln % A.lanes_per_pixel;
            g = A.acc + gi * 3;
        }
        unsigned long long vx = lds_acc[wv][ln], vy = lds_acc[wv][ln + 64], vz = lds_acc[wv][ln + 128];
        if (vx) atomicAdd(g + 0, vx);
        if (vy) atomicAdd(g + 1, vy);
        if (vz) atomicAdd(g + 2, vz);
        if constexpr (kMoments) {
            unsigned long long *g2 = acc2 + (((size_t)row * A.W + px0) * A.lanes_per_pixel + ln) * 3;
            if constexpr (kGather)
                g2 = acc2 + gi * 3;
            const unsigned long long wx = lds_acc2[wv][ln], wy = lds_acc2[wv][ln + 64], wz = lds_acc2[wv][ln + 128];
            if (wx) atomicAdd(g2 + 0, wx);
            if (wy) atomicAdd(g2 + 1, wy);
            if (wz) atomicAdd(g2 + 2, wz);
        }
    }
    PTG_TRACE_END();
}

template <bool kCount, bool kBvh, bool kExact>
__global__ __launch_bounds__(kBlockOf<kBvh>, PTG_MIN_WAVES_PER_EU) void render_kernel(KArgs A)
{
    render_unit<kCount, kBvh, kExact, false>(A, nullptr);
}

// Progressive passes with PTG_FLAG_MOMENTS (plan_single_level: every unit
// accumulates in HBM, no in-wave or cooperative resolve).
// The second LDS array leaves room for 6 waves per SIMD (8 without it): the
// register budget follows.
constexpr int kMomentsWavesPerEu = PTG_MIN_WAVES_PER_EU < 6 ? PTG_MIN_WAVES_PER_EU : 6;
template <bool kBvh, bool kExact, bool kCount = false>
__global__ __launch_bounds__(kBlockOf<kBvh>, kMomentsWavesPerEu) void moments_kernel(KArgs A, unsigned long long *acc2)
{
    render_unit<kCount, kBvh, kExact, true>(A, acc2);
}

// Adaptive passes (ptg_accumulate_active_device): the units of the active
// list, both moments summed, every unit accumulates in HBM.
template <bool kBvh, bool kExact, bool kCount = false>
__global__ __launch_bounds__(kBlockOf<kBvh>, kMomentsWavesPerEu) void gather_kernel(KArgs A, unsigned long long *acc2,
                                                                                   GatherArgs G)
{
    render_unit<kCount, kBvh, kExact, true, true>(A, acc2, G);
}

// PTG_FLAG_LIGHT_SAMPLING with a non-empty light list: the three kernels
// above with render_unit's kLS.  The shadow-segment state (7 VGPRs) does not
// fit the one-shot kernel's 64-VGPR budget, so all three take the moments
// kernels' 6 waves per SIMD (80 VGPRs; DESIGN.md "Light sampling").  Kernels
// of their own, so the plain kernels keep their names and their code.
template <bool kCount, bool kBvh, bool kExact>
__global__ __launch_bounds__(kBlockOf<kBvh>, kMomentsWavesPerEu) void render_ls(KArgs A)
{
    render_unit<kCount, kBvh, kExact, false, false, true>(A, nullptr);
}
template <bool kBvh, bool kExact, bool kCount = false>
__global__ __launch_bounds__(kBlockOf<kBvh>, kMomentsWavesPerEu) void moments_ls(KArgs A, unsigned long long *acc2)
{
    render_unit<kCount, kBvh, kExact, true, false, true>(A, acc2);
}
template <bool kBvh, bool kExact, bool kCount = false>
__global__ __launch_bounds__(kBlockOf<kBvh>, kMomentsWavesPerEu) void gather_ls(KArgs A, unsigned long long *acc2,
                                                                               GatherArgs G)
{
    render_unit<kCount, kBvh, kExact, true, true, true>(A, acc2, G);
}

// PTG_FLAG_STRATIFIED: the kernels above with render_unit's kStrat, with and
// without light sampling.  The seeds, the longer records and the first-hit
// rows take 5 KB of LDS per wave: 38-46 KB per workgroup of the linear
// kernels, which leaves a CU 3 or 4 of them where the plain kernel runs 8, so
// they are compiled for the 3 waves per SIMD the LDS allows (DESIGN.md
// "Stratified sampling").  Kernels of their own: the plain and ls kernels
// keep their names and code.
constexpr int kStratWavesPerEu = PTG_MIN_WAVES_PER_EU < 3 ? PTG_MIN_WAVES_PER_EU : 3;
template <bool kCount, bool kBvh, bool kExact, bool kLS>
__global__ __launch_bounds__(kBlockOf<kBvh>, kStratWavesPerEu) void render_strat(KArgs A)
{
    render_unit<kCount, kBvh, kExact, false, false, kLS, true>(A, nullptr);
}
template <bool kCount, bool kBvh, bool kExact, bool kLS>
__global__ __launch_bounds__(kBlockOf<kBvh>, kStratWavesPerEu) void moments_strat(KArgs A, unsigned long long *acc2)
{
    render_unit<kCount, kBvh, kExact, true, false, kLS, true>(A, acc2);
}
template <bool kCount, bool kBvh, bool kExact, bool kLS>
__global__ __launch_bounds__(kBlockOf<kBvh>, kStratWavesPerEu) void gather_strat(KArgs A, unsigned long long *acc2,
                                                                                  GatherArgs G)
{
    render_unit<kCount, kBvh, kExact, true, true, kLS, true>(A, acc2, G);
}

// The pixel value from the exact sums g of its sub-pixels after samps samples
// (main.cpp:195-196): the clamped sub-pixel means added with weight 1/nsub^2
// in (sy, sx) order.  Shared by resolve_kernel (one samps for the slab) and
// resolve_active_kernel (each pixel's own count).
__device__ __forceinline__ f3 resolve_pixel(const KArgs &A, unsigned long long *g, const int &samps, const int &keep)
{
    f3 pix = mk3(0.0f, 0.0f, 0.0f);
    for (int j = 0; j < A.lanes_per_pixel; ++j) {
        float m[3];
        for (int c = 0; c < 3; ++c) {
            unsigned long long sum = g[3 * j + c];
            if (!keep)
                g[3 * j + c] = 0ull;
            float mean = samps > 0 ? (float)(((double)sum * 0x1p-32) / (double)samps) : 0.0f;
            m[c] = mean < 0.0f ? 0.0f : (1.0f < mean ? 1.0f : mean);
        }
        pix = mk3(__builtin_fmaf(m[0], A.inv_sub2, pix.x), __builtin_fmaf(m[1], A.inv_sub2, pix.y),
                  __builtin_fmaf(m[2], A.inv_sub2, pix.z));
    }
    return pix;
}

// main.cpp:195-196 per pixel (resolve_pixel); re-zeroes the accumulator for
// the next frame.
__global__ __launch_bounds__(256) void resolve_kernel(KArgs A)
{
    const long long i = (long long)A.resolve_row0 * A.W + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)A.slab_rows * A.W)
        return;
    const int slab_row = (int)(i / A.W);
    if (out_row_of(A, slab_row) >= A.H)
        return;
    unsigned long long *g = A.acc + (size_t)i * A.lanes_per_pixel * 3;
    const f3 pix = resolve_pixel(A, g, A.samps, A.keep_acc);
    float *out = A.out + (size_t)i * 3;
    out[0] = pix.x;
    out[1] = pix.y;
    out[2] = pix.z;
}

// ptg_resolve_active_device: resolve_kernel's arithmetic with each pixel's
// own sample count (0 samples: 0); the sums are kept.
__global__ __launch_bounds__(256) void resolve_active_kernel(KArgs A, const int *__restrict__ counts)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)A.slab_rows * A.W)
        return;
    if (out_row_of(A, (int)(i / A.W)) >= A.H)
        return;
    const int np = counts[i], keep = 1;
    const f3 pix = resolve_pixel(A, A.acc + (size_t)i * A.lanes_per_pixel * 3, np, keep);
    float *out = A.out + (size_t)i * 3;
    out[0] = pix.x;
    out[1] = pix.y;
    out[2] = pix.z;
}

// include/ptgpu.h "per-pixel noise estimates": from a pixel's exact sums g1
// (S1) and g2 (S2) after n >= 2 samples, the variance V[3] of its value and
// its relative standard error.  Shared by noise_kernel (one n for the slab)
// and select_over_kernel (each pixel's own count).
__device__ __forceinline__ float noise_pixel(const KArgs &A, const unsigned long long *g1,
                                             const unsigned long long *g2, const double n, const double floor,
                                             double V[3])
{
    f3 pix = mk3(0.0f, 0.0f, 0.0f);
    double vs[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < A.lanes_per_pixel; ++j) {
        float m[3];
        for (int c = 0; c < 3; ++c) {
            const double m1 = ((double)g1[3 * j + c] * 0x1p-32) / n;
            const double m2 = ((double)g2[3 * j + c] * 0x1p-32) / n;
            const float mean = (float)m1;
            m[c] = mean < 0.0f ? 0.0f : (1.0f < mean ? 1.0f : mean);
            double v = m2 - m1 * m1;
            v = (v > 0.0 ? v : 0.0) / (n - 1.0);
            vs[c] += v < 0.25 ? v : 0.25;
        }
        pix = mk3(__builtin_fmaf(m[0], A.inv_sub2, pix.x), __builtin_fmaf(m[1], A.inv_sub2, pix.y),
                  __builtin_fmaf(m[2], A.inv_sub2, pix.z));
    }
    const double w = (double)A.inv_sub2 * (double)A.inv_sub2;
    V[0] = w * vs[0];
    V[1] = w * vs[1];
    V[2] = w * vs[2];
    const double sigma = __builtin_sqrt((V[0] + V[1] + V[2]) / 3.0);
    const double mu = ((double)pix.x + (double)pix.y + (double)pix.z) / 3.0;
    return (float)(sigma / (mu > floor ? mu : floor));
}

// The four statistics of ptg_noise_device, reduced per wave and per workgroup
// (LDS), then one vector atomic per workgroup and value; every thread of the
// workgroup calls it.
__device__ __forceinline__ void reduce_noise_stats(unsigned over, unsigned cnt, unsigned long long fixed,
                                                   unsigned rho_bits, unsigned long long *stats)
{
    for (int off = 32; off > 0; off >>= 1) {  // every lane of the wave takes part
        over += __shfl_xor(over, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
        fixed += __shfl_xor(fixed, off, 64);
        const unsigned other = __shfl_xor(rho_bits, off, 64);
        rho_bits = rho_bits > other ? rho_bits : other;
    }
    __shared__ unsigned long long red[4][4];
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *r = red[threadIdx.x >> 6];
        r[0] = over;
        r[1] = fixed;
        r[2] = rho_bits;
        r[3] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[4] = {0ull, 0ull, 0ull, 0ull};
        for (int wv = 0; wv < 4; ++wv) {
            t[0] += red[wv][0];
            t[1] += red[wv][1];
            t[2] = t[2] > red[wv][2] ? t[2] : red[wv][2];
            t[3] += red[wv][3];
        }
        if (t[3]) {
            atomicAdd(stats + 0, t[0]);
            atomicAdd(stats + 1, t[1]);
            atomicMax(stats + 2, t[2]);
            atomicAdd(stats + 3, t[3]);
        }
    }
}

// ptg_noise_device (include/ptgpu.h "per-pixel noise estimates"): one thread
// per slab pixel (grid-stride), from the exact sums A.acc (S1) and acc2 (S2)
// after A.samps samples: the pixel value p as resolve_kernel computes it, per
// channel the variance V of that value (every sub-pixel's variance of the
// mean capped at 1/4: the image clamps the mean to [0, 1]) and the relative
// standard error rho = sqrt(mean V) / max(mean p, floor); var / rho / stats
// are optional.  stats: four integers, reduced per thread, per wave and per
// workgroup (LDS), then one vector atomic per workgroup and value -- the
// result does not depend on any order, and the grid is small enough
// (ptg_noise_device: at most kNoiseBlocks workgroups) that the atomics on the
// one cache line do not set the time (one per wave of a 1920x1080 frame:
// 1.58 ms, against 0.22 ms without the stats).
constexpr int kNoiseBlocks = 2048;  // 8 workgroups of 256 per CU on 256 CUs
__global__ __launch_bounds__(256) void noise_kernel(KArgs A, const unsigned long long *__restrict__ acc2,
                                                    double rel_error, double floor, float *__restrict__ var,
                                                    float *__restrict__ rho_out, unsigned long long *stats)
{
    const long long total = (long long)A.slab_rows * A.W;
    const long long stride = (long long)gridDim.x * 256;
    unsigned over = 0u, cnt = 0u, rho_bits = 0u;
    unsigned long long fixed = 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        if (out_row_of(A, (int)(i / A.W)) >= A.H)
            continue;  // a slab row past the image
        const unsigned long long *g1 = A.acc + (size_t)i * A.lanes_per_pixel * 3;
        const unsigned long long *g2 = acc2 + (size_t)i * A.lanes_per_pixel * 3;
        double V[3];
        const float rho = noise_pixel(A, g1, g2, (double)A.samps, floor, V);
        if (var) {
            var[(size_t)i * 3 + 0] = (float)V[0];
            var[(size_t)i * 3 + 1] = (float)V[1];
            var[(size_t)i * 3 + 2] = (float)V[2];
        }
        if (rho_out)
            rho_out[i] = rho;
        over += (double)rho > rel_error ? 1u : 0u;
        fixed += (unsigned long long)((rho < 4096.0f ? rho : 4096.0f) * 0x1p20f);
        const unsigned bits = __float_as_uint(rho);  // rho >= 0: the bit patterns order like the values
        rho_bits = rho_bits > bits ? rho_bits : bits;
        cnt += 1u;
    }
    if (!stats)
        return;  // the whole grid
    reduce_noise_stats(over, cnt, fixed, rho_bits, stats);
}

// ---- adaptive sampling: the active list (include/ptgpu.h "adaptive sampling") ----
// ptg_select_active_device, step 1: noise_kernel with each pixel's own sample
// count n_p (n_p < 2: rho = +inf) -- per slab pixel a byte "over the target"
// (0 in rows past the image, so step 2 may read any row), optionally rho, and
// the four statistics.
__global__ __launch_bounds__(256) void select_over_kernel(KArgs A, const unsigned long long *__restrict__ acc2,
                                                          const int *__restrict__ counts, double rel_error,
                                                          double floor, uint8_t *__restrict__ over_out,
                                                          float *__restrict__ rho_out, unsigned long long *stats)
{
    const long long total = (long long)A.slab_rows * A.W;
    const long long stride = (long long)gridDim.x * 256;
    unsigned over = 0u, cnt = 0u, rho_bits = 0u;
    unsigned long long fixed = 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        if (out_row_of(A, (int)(i / A.W)) >= A.H) {
            over_out[i] = 0;
            continue;  // a slab row past the image
        }
        const int np = counts[i];
        float rho = __builtin_inff();
        if (np >= 2) {
            double V[3];
            rho = noise_pixel(A, A.acc + (size_t)i * A.lanes_per_pixel * 3, acc2 + (size_t)i * A.lanes_per_pixel * 3,
                              (double)np, floor, V);
        }
        if (rho_out)
            rho_out[i] = rho;
        const unsigned is_over = (double)rho > rel_error ? 1u : 0u;
        over_out[i] = (uint8_t)is_over;
        over += is_over;
        fixed += (unsigned long long)((rho < 4096.0f ? rho : 4096.0f) * 0x1p20f);
        const unsigned bits = __float_as_uint(rho);
        rho_bits = rho_bits > bits ? rho_bits : bits;
        cnt += 1u;
    }
    if (!stats)
        return;  // the whole grid
    reduce_noise_stats(over, cnt, fixed, rho_bits, stats);
}

// ptg_noise_active_device: noise_kernel's variance slab and rho with each
// pixel's own sample count n_p, the filter's guide for an adaptive frame (one
// thread per slab pixel, grid-stride; var and rho_out each optional).
// n_p < 2 knows nothing beyond the clamp's bound: rho = +inf as in
// select_over_kernel, and per channel the V noise_pixel yields when every
// sub-pixel's variance sits at the 1/4 cap.  No statistics: the select step
// supplies them.
__global__ __launch_bounds__(256) void noise_active_kernel(KArgs A, const unsigned long long *__restrict__ acc2,
                                                           const int *__restrict__ counts, double floor,
                                                           float *__restrict__ var, float *__restrict__ rho_out)
{
    const long long total = (long long)A.slab_rows * A.W;
    const long long stride = (long long)gridDim.x * 256;
    const float v_cap = (float)(((double)A.inv_sub2 * (double)A.inv_sub2) * ((double)A.lanes_per_pixel * 0.25));
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        if (out_row_of(A, (int)(i / A.W)) >= A.H)
            continue;  // a slab row past the image
        const int np = counts[i];
        float rho = __builtin_inff();
        float v[3] = {v_cap, v_cap, v_cap};
        if (np >= 2) {
            double V[3];
            rho = noise_pixel(A, A.acc + (size_t)i * A.lanes_per_pixel * 3, acc2 + (size_t)i * A.lanes_per_pixel * 3,
                              (double)np, floor, V);
            v[0] = (float)V[0];
            v[1] = (float)V[1];
            v[2] = (float)V[2];
        }
        if (var) {
            var[(size_t)i * 3 + 0] = v[0];
            var[(size_t)i * 3 + 1] = v[1];
            var[(size_t)i * 3 + 2] = v[2];
        }
        if (rho_out)
            rho_out[i] = rho;
    }
}

// List building, step 1: one workgroup per slab row writes the row's active x
// in ascending order to list[row * W ...] and their number to row_count[row].
// Active: flags == NULL, or some flag byte of the pixel's (2 dilate + 1)^2
// window, clipped to the image, is set (dilate > 0 only with shard_count 1,
// where slab row j is image row j).  Ranks: ballot / mbcnt within a wave, the
// waves' counts through LDS -- the order does not depend on any timing.
__global__ __launch_bounds__(256) void list_rows_kernel(KArgs A, const uint8_t *__restrict__ flags, int dilate,
                                                        int *__restrict__ list, int *__restrict__ row_count)
{
    const int row = blockIdx.x;
    const bool valid_row = out_row_of(A, row) < A.H;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ int wave_cnt[4];
    int base = 0;  // the row's active pixels left of this tile (workgroup-uniform)
    for (int x0 = 0; x0 < A.W; x0 += 256) {
        const int x = x0 + (int)threadIdx.x;
        bool act = false;
        if (valid_row && x < A.W) {
            if (!flags) {
                act = true;
            } else if (dilate == 0) {
                act = flags[(size_t)row * A.W + x] != 0;
            } else {
                const int r0 = row - dilate > 0 ? row - dilate : 0;
                const int r1 = row + dilate < A.H - 1 ? row + dilate : A.H - 1;
                const int c0 = x - dilate > 0 ? x - dilate : 0;
                const int c1 = x + dilate < A.W - 1 ? x + dilate : A.W - 1;
                for (int rr = r0; rr <= r1; ++rr)
                    for (int cc = c0; cc <= c1; ++cc)
                        act |= flags[(size_t)rr * A.W + cc] != 0;
            }
        }
        const unsigned long long m = __ballot(act);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0)
            wave_cnt[wv] = (int)__popcll(m);
        __syncthreads();
        int before = 0, tile = 0;
        for (int w = 0; w < 4; ++w) {
            const int c = wave_cnt[w];
            before += w < wv ? c : 0;
            tile += c;
        }
        if (act)
            list[(size_t)row * A.W + base + before + rank] = x;  // base + before + rank < the row's count <= W
        base += tile;
        __syncthreads();  // wave_cnt is rewritten by the next tile
    }
    if (threadIdx.x == 0)
        row_count[row] = base;
}

// Step 1 for a shard of a multi-device frame (ptg_set_active_gathered_device):
// list_rows_kernel's output from the over bytes of the WHOLE frame, gathered
// rank-major (shard_count slabs of slab_rows * W bytes, ptg_unshard_device's
// layout) -- with interleaved bands the window rows of a pixel live in other
// shards' slabs.  Separable, per tile of 256 columns:
//   1. the row's <= 17 window rows (clipped to the image) are mapped to
//      gathered slab rows once, in LDS (workgroup-uniform);
//   2. each lane ORs its column over those rows (coalesced byte loads); the
//      wave's ballot is a 64-bit word in LDS -- 4 words a tile, and a fifth
//      from the first `dilate` columns right of it (the seam: x = 255 needs
//      columns up to 263); the word left of the tile is carried in a register;
//   3. every wave dilates the 4 words horizontally, each OR-ed with its two
//      neighbours shifted by -dilate..+dilate (dilate <= 8 < 64) -- scalar
//      work; its own word gives the lanes' flags, the popcounts of all four
//      the ranks (no second pass through LDS).
// Columns >= W and rows outside the image contribute no set bit, so the window
// is clipped; slab rows past the image are never read.
constexpr int kMaxDilate = 8;

__device__ __forceinline__ unsigned long long dilate_word(unsigned long long l, unsigned long long c,
                                                          unsigned long long r, int dilate)
{
    unsigned long long d = c;
    for (int k = 1; k <= dilate; ++k)  // column b -+ k set: pixel b is active
        d |= (c << k) | (l >> (64 - k)) | (c >> k) | (r << (64 - k));
    return d;
}

__global__ __launch_bounds__(256) void list_rows_gathered_kernel(KArgs A, const uint8_t *__restrict__ gathered,
                                                                 int dilate, int *__restrict__ list,
                                                                 int *__restrict__ row_count)
{
    const int row = blockIdx.x;
    const int r = out_row_of(A, row);
    if (r >= A.H) {  // a slab row past the image (the whole workgroup)
        if (threadIdx.x == 0)
            row_count[row] = 0;
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ long long win_row[2 * kMaxDilate + 1];  // gathered slab row (rank-major) of each window row
    __shared__ unsigned long long word[5];             // column-OR ballots: the tile's four, the right seam's
    const int r0 = r - dilate > 0 ? r - dilate : 0;
    const int r1 = r + dilate < A.H - 1 ? r + dilate : A.H - 1;
    const int n_win = r1 - r0 + 1;
    if ((int)threadIdx.x < n_win) {
        const int rr = r0 + (int)threadIdx.x;
        const int band = rr / A.band_rows;
        const int rank = band % A.shard_count;
        win_row[threadIdx.x] = (long long)rank * A.slab_rows + (long long)(band / A.shard_count) * A.band_rows +
                               (rr - band * A.band_rows);
    }
    __syncthreads();
    auto column_or = [&](int x, bool on) -> unsigned long long {
        unsigned v = 0u;
        if (on && x < A.W)
            for (int j = 0; j < n_win; ++j)
                v |= gathered[(size_t)win_row[j] * A.W + x];
        return __ballot(v != 0u);
    };
    unsigned long long left = 0ull;  // the word of the 64 columns left of the tile (workgroup-uniform)
    int base = 0;                    // the row's active pixels left of this tile (workgroup-uniform)
    for (int x0 = 0; x0 < A.W; x0 += 256) {
        const int x = x0 + (int)threadIdx.x;
        const unsigned long long own = column_or(x, true);
        if (lane == 0)
            word[wv] = own;
        if (wv == 0) {  // the seam: the first `dilate` columns of the next tile
            const unsigned long long seam = column_or(x + 256, lane < dilate);
            if (lane == 0)
                word[4] = seam;
        }
        __syncthreads();
        unsigned long long w[6];
        w[0] = left;
        for (int i = 0; i < 5; ++i)
            w[i + 1] = word[i];
        int before = 0, tile = 0;
        unsigned long long mine = 0ull;
        for (int i = 0; i < 4; ++i) {
            const int nv = A.W - (x0 + 64 * i);  // the word's columns inside the image
            const unsigned long long valid = nv >= 64 ? ~0ull : (nv > 0 ? (1ull << nv) - 1ull : 0ull);
            const unsigned long long d = dilate_word(w[i], w[i + 1], w[i + 2], dilate) & valid;
            const int c = (int)__popcll(d);
            before += i < wv ? c : 0;
            tile += c;
            mine = i == wv ? d : mine;
        }
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mine >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((unsigned)mine, 0u));
        if ((mine >> lane) & 1ull)
            list[(size_t)row * A.W + base + before + rank] = x;  // base + before + rank < the row's count <= W
        base += tile;
        left = w[4];
        __syncthreads();  // word is rewritten by the next tile
    }
    if (threadIdx.x == 0)
        row_count[row] = base;
}

// Step 2, one workgroup: a row's pixels are cut into units of pixels_per_wave
// (units never span rows); row_unit0[row] = the units of the rows before it
// (an exclusive scan: shuffles within a wave, LDS across the workgroup, a
// carry across tiles of 256 rows).  Writes the device record {active pixels,
// active units}, the same two values to info (optional), and adds them to
// stats[4], stats[5] (optional).
__global__ __launch_bounds__(256) void list_units_kernel(int slab_rows, int ppw, const int *__restrict__ row_count,
                                                         int *__restrict__ row_unit0, unsigned long long *rec,
                                                         unsigned long long *info, unsigned long long *stats)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ int wave_sum[4];
    __shared__ unsigned long long wave_pix[4];
    unsigned long long pixels = 0ull;
    int carry = 0;
    for (int r0 = 0; r0 < slab_rows; r0 += 256) {
        const int r = r0 + (int)threadIdx.x;
        const int cnt = r < slab_rows ? row_count[r] : 0;
        const int nu = (cnt + ppw - 1) / ppw;
        pixels += (unsigned long long)cnt;
        int incl = nu;
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            incl += lane >= off ? v : 0;
        }
        if (lane == 63)
            wave_sum[wv] = incl;
        __syncthreads();
        int before = 0, tile = 0;
        for (int w = 0; w < 4; ++w) {
            const int c = wave_sum[w];
            before += w < wv ? c : 0;
            tile += c;
        }
        if (r < slab_rows)
            row_unit0[r] = carry + before + incl - nu;
        carry += tile;
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1)
        pixels += __shfl_xor(pixels, off, 64);
    if (lane == 0)
        wave_pix[wv] = pixels;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long np = wave_pix[0] + wave_pix[1] + wave_pix[2] + wave_pix[3];
        rec[0] = np;
        rec[1] = (unsigned long long)carry;
        if (info) {
            info[0] = np;
            info[1] = (unsigned long long)carry;
        }
        if (stats) {
            atomicAdd(stats + 4, np);
            atomicAdd(stats + 5, (unsigned long long)carry);
        }
    }
}

// Step 3, one workgroup per slab row: the row's entries of the unit table,
// {slab row, first index in the row's list, pixels}.  The entries written are
// [0, rec[1]), at most n_groups (the table's size).
__global__ __launch_bounds__(256) void list_fill_kernel(int ppw, const int *__restrict__ row_count,
                                                        const int *__restrict__ row_unit0, int4 *__restrict__ units)
{
    const int row = blockIdx.x;
    const int cnt = row_count[row], u0 = row_unit0[row];
    for (int k = threadIdx.x; k * ppw < cnt; k += 256)
        units[u0 + k] = make_int4(row, k * ppw, cnt - k * ppw < ppw ? cnt - k * ppw : ppw, 0);
}

// After gather_kernel (not inside it: other chunks of the same pixel read
// n_p at unit setup): one wave per unit (grid-stride) adds add_samples to the
// counts of the unit's pixels, the same units [0, min(rec[1], max_units)).
__global__ __launch_bounds__(256) void bump_counts_kernel(int W, const int4 *__restrict__ units,
                                                          const int *__restrict__ list,
                                                          const unsigned long long *__restrict__ rec,
                                                          long long max_units, int add, int *__restrict__ counts)
{
    long long n = (long long)rec[1];
    n = n < max_units ? n : max_units;
    const int lane = threadIdx.x & 63;
    for (long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); u < n; u += (long long)gridDim.x * 4) {
        const int4 e = units[u];
        if (lane < e.z) {
            const size_t rowbase = (size_t)e.x * W;
            counts[rowbase + list[rowbase + e.y + lane]] += add;
        }
    }
}

// Parity probe: one path per record {x, y, sx, sy, sample}.
template <bool kBvh, bool kExact, bool kLS, bool kStrat>
__device__ __forceinline__ void trace_path(const KArgs &A, const int32_t *coords, int n, float *out, int32_t *segs_out)
{
    int i = blockIdx.x * kTraceBlock + threadIdx.x;
    if (i >= n)
        return;
    Lane L;
    L.x = coords[5 * i + 0];
    L.y = coords[5 * i + 1];
    L.sx = coords[5 * i + 2];
    L.sy = coords[5 * i + 3];
    uint32_t sample = (uint32_t)coords[5 * i + 4];
    uint64_t pixel_sub = ((uint64_t)L.y * (uint64_t)A.W + (uint64_t)L.x) * (uint64_t)A.lanes_per_pixel +
                         (uint64_t)(L.sy * A.nsub + L.sx);
    L.key = key_hash(A.seed, pixel_sub);
    f3 o, d;
    uint32_t st;
    [[maybe_unused]] LsLane ls{};
    [[maybe_unused]] LsIo io{};
    [[maybe_unused]] uint4 fh{};
    if constexpr (kStrat) {
        const uint32_t brs = sobol::brev(sample);
        uint4 cq;
        sobol::pair_brev(sobol::seeds_of(L.key, 0), brs, cq.x, cq.y);
        sobol::pair_brev(sobol::seeds_of(L.key, 1), brs, cq.z, cq.w);
        sobol::pair_brev(sobol::seeds_of(L.key, 2), brs, fh.x, fh.y);
        sobol::pair_brev(sobol::seeds_of(L.key, 3), brs, fh.z, fh.w);
        camera_ray<true>(cam_of(A), L, sample, st, o, d, cq);
    } else
    camera_ray(cam_of(A), L, sample, st, o, d);
    f3 T = mk3(1.0f, 1.0f, 1.0f), E = mk3(0.0f, 0.0f, 0.0f);
    int depth = 0, segs = 0;
    bool done = false;
    while (!done) {
        segs += 1;
        ScanCount scnt;
        if constexpr (kLS || kStrat) {  // (shadow segments are scans too)
            if constexpr (kLS) {
                io.lights = A.lights;
                io.n_lights = A.n_lights;
                io.shadow = io.to_shadow;
                io.skip = io.skip_next;
                io.to_shadow = io.skip_next = false;
            }
            done = segment<kBvh, kExact, false, kLS, kStrat>(A, A.lin, A.trig, o, d, T, E, depth, st, scnt, ls, io, fh);
        } else
        done = segment<kBvh, kExact>(A, A.lin, A.trig, o, d, T, E, depth, st, scnt);
    }
    out[3 * i + 0] = E.x;
    out[3 * i + 1] = E.y;
    out[3 * i + 2] = E.z;
    segs_out[i] = segs;
}
template <bool kBvh, bool kExact, bool kLS = false>
__global__ __launch_bounds__(kTraceBlock) void trace_kernel(KArgs A, const int32_t *coords, int n, float *out,
                                                         int32_t *segs_out)
{
    trace_path<kBvh, kExact, kLS, false>(A, coords, n, out, segs_out);
}
// PTG_FLAG_STRATIFIED
template <bool kBvh, bool kExact, bool kLS>
__global__ __launch_bounds__(kTraceBlock) void trace_strat(KArgs A, const int32_t *coords, int n, float *out,
                                                        int32_t *segs_out)
{
    trace_path<kBvh, kExact, kLS, true>(A, coords, n, out, segs_out);
}

// ptg_features_device: the first hit of the pixel's nsub^2 deterministic
// camera rays (camera_ray with both jitter draws 0.5 and no lens offset), by
// the renderer's own scan in exact arithmetic; one thread per slab pixel.
// 12 floats: {n.xyz, z}, {P.xyz, hit}, {albedo.rgb, 0} (include/ptgpu.h).
template <bool kBvh>
__global__ __launch_bounds__(256) void features_kernel(KArgs A, float4 *__restrict__ feat)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)A.slab_rows * A.W)
        return;
    const int slab_row = (int)(i / A.W);
    const int r = out_row_of(A, slab_row);
    if (r >= A.H)
        return;
    const int px = (int)(i - (long long)slab_row * A.W);
    const int y = A.H - 1 - r;  // main.cpp:181
    const CamC C = cam_of(A);
    const f3 o = mk3(C.p.x, C.p.y, C.p.z);
    f3 n = mk3(0.0f, 0.0f, 0.0f), P = n, a = n;
    float z = 0.0f;
    int hits = 0;
    for (int sy = 0; sy < A.nsub; ++sy)
        for (int sx = 0; sx < A.nsub; ++sx) {
            const float xin = __builtin_fmaf(C.b.w, 0.5f, (float)px + (float)sx * C.b.w);
            const float yin = __builtin_fmaf(C.b.w, 0.5f, (float)y + (float)sy * C.b.w);
            const float fs = xin * C.X.w;
            const float ft = yin * C.Y.w;
            const f3 d = mk3(__builtin_fmaf(C.Y.x, ft, __builtin_fmaf(C.X.x, fs, C.b.x)),
                             __builtin_fmaf(C.Y.y, ft, __builtin_fmaf(C.X.y, fs, C.b.y)),
                             __builtin_fmaf(C.Y.z, ft, __builtin_fmaf(C.X.z, fs, C.b.z)));
            float t;
            ScanCount cnt;
            const ShadeRec *hit;
            if constexpr (kBvh) {
                const int id = scene_scan_bvh<false, true>(A, o, d, t, cnt);
                hit = id >= 0 ? A.shade + id : nullptr;
            } else {
                const LinRec *w = scene_scan<true>(A, A.lin, o, d, t, cnt);
                hit = w != A.lin + A.n ? &w->s : nullptr;
            }
            if (!hit)
                continue;
            // the hit point and the facing normal as shade<true> forms them
            const float4 s0 = hit->s0, s2 = hit->s2;
            const f3 p = mk3(__builtin_fmaf(d.x, t, o.x), __builtin_fmaf(d.y, t, o.y), __builtin_fmaf(d.z, t, o.z));
            const f3 on = mk3((p.x - s0.x) * s2.w, (p.y - s0.y) * s2.w, (p.z - s0.z) * s2.w);
            const bool front = dot3(on, d) < 0.0f;
            hits += 1;
            n = mk3(n.x + (front ? on.x : -on.x), n.y + (front ? on.y : -on.y), n.z + (front ? on.z : -on.z));
            P = mk3(P.x + p.x, P.y + p.y, P.z + p.z);
            a = mk3(a.x + s2.x, a.y + s2.y, a.z + s2.z);
            z = __builtin_fmaf(t, Math<true>::sqrt(dot3(d, d)), z);
        }
    const float k = (float)(hits > 0 ? hits : 1);
    float4 *out = feat + (size_t)i * 3;
    out[0] = make_float4(n.x / k, n.y / k, n.z / k, z / k);
    out[1] = make_float4(P.x / k, P.y / k, P.z / k, (float)hits / (float)A.lanes_per_pixel);
    out[2] = hits > 0 ? make_float4(a.x / k, a.y / k, a.z / k, 0.0f) : make_float4(1.0f, 1.0f, 1.0f, 0.0f);
}

#include "follow_features.hpp"  // features_follow_kernel (ptg_features_follow_device)

// ptg_math_probe_device: the primitives as the render kernels call them
template <bool kExact>
__global__ __launch_bounds__(256) void math_probe_kernel(int op, const float *in, float *out, int n,
                                                         const float2 *trig)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    if (op == PTG_PROBE_SQRT) {
        out[i] = Math<kExact>::sqrt(in[i]);
    } else if (op == PTG_PROBE_RSQRT) {
        out[i] = Math<kExact>::rsqrt(in[i]);
    } else if (op == PTG_PROBE_DIV) {
        out[i] = Math<kExact>::div(in[2 * i], in[2 * i + 1]);
    } else {
        float c, s;
        Math<kExact>::sincos2pi(__float_as_uint(in[i]) & 0xFFFFFFu, trig, c, s);
        out[2 * i] = c;
        out[2 * i + 1] = s;
    }
}

// ptg_sampler_pairs_device: PTG_FLAG_STRATIFIED's pairs 0..3 of one path per
// record {x, y, sx, sy, sample}, as the render kernels form them
__global__ __launch_bounds__(256) void sampler_pairs_kernel(KArgs A, const int32_t *coords, int n, uint32_t *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t pixel_sub = ((uint64_t)coords[5 * i + 1] * (uint64_t)A.W + (uint64_t)coords[5 * i + 0]) *
                                   (uint64_t)A.lanes_per_pixel +
                               (uint64_t)(coords[5 * i + 3] * A.nsub + coords[5 * i + 2]);
    const uint64_t key = key_hash(A.seed, pixel_sub);
    const uint32_t brs = sobol::brev((uint32_t)coords[5 * i + 4]);
    for (int j = 0; j < sobol::kPairs; ++j) {
        uint32_t m0, m1;
        sobol::pair_brev(sobol::seeds_of(key, j), brs, m0, m1);
        out[8 * i + 2 * j] = m0;
        out[8 * i + 2 * j + 1] = m1;
    }
}

__global__ void unshard_kernel(const float *__restrict__ src, float *__restrict__ dst, int W, int band_rows,
                               int count, int slab_rows)
{
    int r = blockIdx.y;
    int band = r / band_rows;
    int k = band % count;
    int j = band / count;
    size_t srow = (size_t)k * slab_rows + (size_t)j * band_rows + (size_t)(r - band * band_rows);
    const float *s = src + srow * (size_t)W * 3;
    float *t = dst + (size_t)r * (size_t)W * 3;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < W * 3; i += gridDim.x * blockDim.x)
        t[i] = s[i];
}

// utils.cpp:11-16: round(pow(clamp(x), 1/2.2) * 255)
__global__ void tonemap_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, size_t count)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    double x = (double)in[i];
    x = x < 0.0 ? 0.0 : (1.0 < x ? 1.0 : x);
    out[i] = (uint8_t)(int)round(pow(x, 1.0 / 2.2) * 255.0);
}

}  // namespace

struct ptg_context {
    int device;
    int n;
    int wave_slots;     // CUs x 32 resident waves (split-tail sizing)
    LinRec *d_lin;      // linear scenes
    ShadeRec *d_shade;  // BVH scenes
    void *d_bvh;  // one allocation: nodes | leaf geometry | leaf ids | big geometry | big ids
    float2 *d_trig;  // sin/cos table (trig_table)
    unsigned long long *d_acc;  // exact per-sub-pixel sums; kept zero between frames by resolve
    size_t acc_elems;
    bool acc_dirty;  // progressive sums may be in d_acc (accumulate / keep_acc resolve since the last reset)
    KArgs base;  // camera + scene fields filled
    ptg_sphere *d_sph64;  // the scene as given (PTG_FLAG_REFERENCE_F64)
    ptg_camera cam64;
    // PTG_FLAG_MOMENTS: exact per-sub-pixel sums of squares, laid out like d_acc; allocated on first use
    unsigned long long *d_acc2;
    size_t acc2_elems;
    bool moments_pass;  // a pass since the last reset added to d_acc2 ...
    bool plain_pass;    // ... or ran without the flag (d_acc2 then lacks its samples: no noise estimate)
    // adaptive sampling (ptg_*_active_device), allocated on first use: per slab pixel its sample count, the
    // over-target bytes, the active list (per slab row, stride W, its active x ascending), per slab row its
    // active pixels and first unit, the unit table (n_groups entries) and the device record {pixels, units}
    int32_t *d_counts;
    uint8_t *d_over;
    int *d_list, *d_row_count, *d_row_unit0;
    int4 *d_units;
    unsigned long long *d_rec;
    size_t ad_pixels, ad_rows, ad_groups;  // what the buffers above have room for
    ptg_params list_frame;  // the frame the active list was built for ...
    bool list_valid;        // ... if any since the last reset
    bool uniform_pass;      // a ptg_accumulate_device pass since the last reset: no adaptive entry point
    bool adaptive_pass;     // a ptg_accumulate_active_device pass since the last reset: no uniform n describes the sums
    long long adaptive_added;  // the adds since the last reset: no count is above their sum
    // PTG_FLAG_LIGHT_SAMPLING: the scene's light list (scene indices; more than kMaxLights: the flag is
    // refused) and its device records (base.lights, base.n_lights)
    int n_lights;
    int light_ids[kMaxLights];
    LightRec *d_lights;
};

namespace {

int set_device(int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PTG_ERR_NO_DEVICE, "no HIP device visible");
    if (device >= count)
        return fail(PTG_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    if (device >= 0)
        PTG_HIP(hipSetDevice(device));
    return PTG_OK;
}

// ptg_context_create: one of the context's device tables, allocated and filled
template <typename T>
int upload(T *&dst, const void *src, size_t bytes, const char *what)
{
    if (hipMalloc(&dst, bytes) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, std::string("hipMalloc of ") + what + " failed");
    PTG_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return PTG_OK;
}

#if PTG_BLOCK_STATS
// a 256 x 16 block-counter array (ptg_dbg_stats, ptg_dbg_stats2) summed over its slots, then zeroed
template <typename Sym>
int read_block_stats(const Sym &sym, unsigned long long *out16)
{
    std::vector<unsigned long long> h(256 * 16);
    PTG_HIP(hipDeviceSynchronize());
    PTG_HIP(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(sym), h.size() * sizeof(h[0])));
    for (int i = 0; i < 16; ++i) {
        out16[i] = 0;
        for (int b = 0; b < 256; ++b)
            out16[i] += h[b * 16 + i];
    }
    std::vector<unsigned long long> z(h.size(), 0ull);
    PTG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(sym), z.data(), z.size() * sizeof(z[0])));
    return PTG_OK;
}
#endif

}  // namespace

extern "C" {

// internal (csrc/ptg_multi.cpp): set the thread-local error of ptg_last_error
int ptg_set_error_(int code, const char *msg) { return fail(code, msg ? msg : ""); }

int ptg_abi_version(void) { return PTG_ABI_VERSION; }

#if PTG_UNIT_TRACE
// debug builds only: the per-unit trace of the launches since the last call
// (3 values per unit, see ptg_unit_trace; then zeroed)
int ptg_unit_trace_(unsigned long long *out, int n_units)
{
    const size_t n = (size_t)std::min(n_units, kTraceUnits) * 3;
    PTG_HIP(hipDeviceSynchronize());
    PTG_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(ptg_unit_trace), n * sizeof(unsigned long long)));
    std::vector<unsigned long long> z(n, 0ull);
    PTG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ptg_unit_trace), z.data(), n * sizeof(unsigned long long)));
    return PTG_OK;
}
#endif
#if PTG_BLOCK_STATS
// debug builds only: the 16 block counters summed over their 256 slots (then zeroed)
int ptg_debug_stats2_(unsigned long long *out16) { return read_block_stats(ptg_dbg_stats2, out16); }
int ptg_debug_stats_(unsigned long long *out16) { return read_block_stats(ptg_dbg_stats, out16); }
#endif

const char *ptg_last_error(void) { return g_last_error.c_str(); }

int ptg_device_count(int *count)
{
    if (!count)
        return fail(PTG_ERR_INVALID_ARGUMENT, "count is NULL");
    *count = 0;
    if (hipGetDeviceCount(count) != hipSuccess)
        *count = 0;
    return PTG_OK;
}

int ptg_shard_rows(int32_t height, int32_t band_rows, int32_t shard_count, int32_t *rows)
{
    if (!rows || height <= 0 || band_rows <= 0 || shard_count <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "invalid shard geometry");
    *rows = shard_slab_rows(height, band_rows, shard_count);
    return PTG_OK;
}

int ptg_context_create(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int device,
                       ptg_context **out)
{
    if (!out || !cam || (n_spheres && !spheres))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (n_spheres > (size_t)(1 << 24))
        return fail(PTG_ERR_UNSUPPORTED, "too many spheres");
    for (size_t i = 0; i < n_spheres; ++i)
        if (!sphere_ok(spheres[i]))
            return fail(PTG_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(i) + " is invalid");
    int rc = set_device(device);
    if (rc)
        return rc;
    int dev = 0;
    PTG_HIP(hipGetDevice(&dev));
    ptg_context *ctx = new ptg_context();  // zeroed, base included
    ctx->device = dev;
    {
        hipDeviceProp_t prop;
        ctx->wave_slots = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount * 32 : 8192;
    }
    const int n = ctx->n = (int)n_spheres;
    ctx->cam64 = *cam;
    KArgs &A = ctx->base;
    // prepare (scene_prep.hpp): the upload tables; the scan layout goes straight into A
    const bool linear = n <= kLinearMax;
    const SceneRecs sc = prepare_scene(spheres, n, cam);
    std::vector<LinRec> lin;
    BvhUpload bvh;
    if (linear)
        lin = prepare_linear_upload(spheres, n, cam, sc, A);
    else
        bvh = prepare_bvh_upload(spheres, n, cam, sc.geo);
    float trig[2 * kTrigEntries];
    trig_table(trig);
    // allocate and upload.  linear scenes: d_lin; BVH scenes: d_shade (scene index order) + d_bvh
    rc = linear ? upload(ctx->d_lin, lin.data(), lin.size() * sizeof(LinRec), "the scene")
                : upload(ctx->d_shade, sc.shade.data(), (size_t)n * sizeof(ShadeRec), "the scene");
    if (!rc)
        rc = upload(ctx->d_trig, trig, sizeof(trig), "the sin/cos table");
    if (!rc && n)
        rc = upload(ctx->d_sph64, spheres, (size_t)n * sizeof(ptg_sphere), "the scene (f64)");
    if (!rc && !linear)
        rc = upload(ctx->d_bvh, bvh.blob.data(), bvh.blob.size(), "the BVH");
    // the light list (light sampling); too long a list is refused where the flag is given
    const std::vector<int> light_ids = light_list_of(spheres, n, cam);
    ctx->n_lights = (int)light_ids.size();
    if (!rc && ctx->n_lights > 0 && ctx->n_lights <= kMaxLights) {
        std::vector<int> id_of(n);
        for (int i = 0; i < n; ++i)
            id_of[i] = i;
        if (linear) {  // the scan reports scan positions
            KArgs scratch{};
            const std::vector<int> order = scan_order_of(spheres, n, cam, sc, scratch);
            for (int j = 0; j < n; ++j)
                id_of[order[j]] = j;
        }
        const std::vector<LightRec> lrecs = light_records(spheres, light_ids, id_of);
        for (int k = 0; k < ctx->n_lights; ++k)
            ctx->light_ids[k] = light_ids[k];
        rc = upload(ctx->d_lights, lrecs.data(), lrecs.size() * sizeof(LightRec), "the light list");
    }
    if (rc) {
        ptg_context_destroy(ctx);
        return rc;
    }
    // the scene and camera fields of every launch's KArgs
    A.trig = ctx->d_trig;
    A.lin = ctx->d_lin;
    A.shade = ctx->d_shade;
    A.n = n;
    A.room_nmr = room_neg_margin(A);
    A.lights = ctx->d_lights;
    A.n_lights = ctx->d_lights ? ctx->n_lights : 0;
    if (!linear) {
        const unsigned char *blob = static_cast<const unsigned char *>(ctx->d_bvh);
        A.bvh_qnodes = reinterpret_cast<const uint4 *>(blob + bvh.off_q);
        A.bvh_cont = reinterpret_cast<const int *>(blob + bvh.off_cont);
        A.bvh_sph = reinterpret_cast<const float4 *>(blob + bvh.off_geo);
        A.bvh_id = reinterpret_cast<const int *>(blob + bvh.off_id);
        A.big_geo = reinterpret_cast<const GeoRec *>(blob + bvh.off_bgeo);
        A.big_id = reinterpret_cast<const int *>(blob + bvh.off_bid);
        for (int c = 0; c < 3; ++c) {
            A.q_lo[c] = bvh.q_lo[c];
            A.q_scale[c] = bvh.q_scale[c];
        }
        A.n_nodes = bvh.n_nodes;
        A.n_big = bvh.n_big;
    }
    prepare_camera(cam, A);
    *out = ctx;
    return PTG_OK;
}

int ptg_scene_layout(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int32_t *anchor_axis,
                     int32_t *scan_order)
{
    if (!cam || (n_spheres && (!spheres || !anchor_axis || !scan_order)))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_spheres > (size_t)(1 << 24))
        return fail(PTG_ERR_UNSUPPORTED, "too many spheres");
    const int n = (int)n_spheres;
    const SceneRecs sc = prepare_scene(spheres, n, cam);
    KArgs ends{};
    std::vector<int> order;
    if (n <= kLinearMax)
        order = scan_order_of(spheres, n, cam, sc, ends);
    for (int i = 0; i < n; ++i)
        anchor_axis[i] = sc.axis[i];
    for (int k = 0; k < 3 && n <= kLinearMax; ++k)
        if (ends.pairs[k])  // the pair leads axis k's group
            anchor_axis[order[k == 0 ? 0 : ends.end_ax[k - 1]]] = anchor_axis[order[(k == 0 ? 0 : ends.end_ax[k - 1]) + 1]] = k + 3;
    for (int i = 0; i < n; ++i)
        scan_order[i] = n <= kLinearMax ? order[i] : i;
    return PTG_OK;
}

int ptg_light_list(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int32_t *ids, int cap,
                   int *n_lights)
{
    if (!cam || !n_lights || (n_spheres && !spheres) || cap < 0 || (cap && !ids))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_spheres > (size_t)(1 << 24))
        return fail(PTG_ERR_UNSUPPORTED, "too many spheres");
    const std::vector<int> list = light_list_of(spheres, (int)n_spheres, cam);
    *n_lights = (int)list.size();
    for (int k = 0; k < cap && k < (int)list.size(); ++k)
        ids[k] = list[k];
    if ((int)list.size() > kMaxLights)
        return fail(PTG_ERR_UNSUPPORTED, "light sampling: " + std::to_string(list.size()) +
                                             " small emitters, at most " + std::to_string(kMaxLights));
    return PTG_OK;
}

int ptg_context_destroy(ptg_context *ctx)
{
    if (!ctx)
        return PTG_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->d_lin)
        (void)hipFree(ctx->d_lin);
    if (ctx->d_shade)
        (void)hipFree(ctx->d_shade);
    if (ctx->d_trig)
        (void)hipFree(ctx->d_trig);
    if (ctx->d_bvh)
        (void)hipFree(ctx->d_bvh);
    if (ctx->d_acc)
        (void)hipFree(ctx->d_acc);
    if (ctx->d_acc2)
        (void)hipFree(ctx->d_acc2);
    if (ctx->d_sph64)
        (void)hipFree(ctx->d_sph64);
    if (ctx->d_lights)
        (void)hipFree(ctx->d_lights);
    for (void *q : {(void *)ctx->d_counts, (void *)ctx->d_over, (void *)ctx->d_list, (void *)ctx->d_row_count,
                    (void *)ctx->d_row_unit0, (void *)ctx->d_units, (void *)ctx->d_rec})
        if (q)
            (void)hipFree(q);
    delete ctx;
    return PTG_OK;
}

}  // extern "C"

namespace {

size_t acc_elems_for(const KArgs &A) { return (size_t)A.slab_rows * A.W * A.lanes_per_pixel * 3; }

// the second accumulator zero and no pass on record
int forget_moments(ptg_context *ctx, hipStream_t stream)
{
    if (ctx->d_acc2 && ctx->moments_pass)  // (only such passes write to it)
        PTG_HIP(hipMemsetAsync(ctx->d_acc2, 0, ctx->acc2_elems * sizeof(unsigned long long), stream));
    ctx->moments_pass = ctx->plain_pass = false;
    // the adaptive frame with them: counts zero, no list, no pass of either kind on record
    if (ctx->d_counts && (ctx->adaptive_pass || ctx->adaptive_added))
        PTG_HIP(hipMemsetAsync(ctx->d_counts, 0, ctx->ad_pixels * sizeof(int32_t), stream));
    ctx->list_valid = ctx->uniform_pass = ctx->adaptive_pass = false;
    ctx->adaptive_added = 0;
    return PTG_OK;
}

// exact accumulator: allocated (zeroed) on first use at a size; resolve_kernel
// keeps it zero between one-shot frames.  The zeroing is queued on the launch
// stream: a hipMemset on the null stream is not ordered before kernels on a
// non-blocking stream (ptg_render_multi's), whose first frame could then add
// into a buffer being cleared (seen once as a differing box_mirror frame)
int ensure_acc(ptg_context *ctx, size_t need, hipStream_t stream)
{
    if (need <= ctx->acc_elems)
        return PTG_OK;
    if (ctx->d_acc)
        PTG_HIP(hipFree(ctx->d_acc));
    ctx->d_acc = nullptr;
    ctx->acc_elems = 0;
    if (hipMalloc(&ctx->d_acc, need * sizeof(unsigned long long)) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the accumulator failed");
    PTG_HIP(hipMemsetAsync(ctx->d_acc, 0, need * sizeof(unsigned long long), stream));
    ctx->acc_elems = need;
    ctx->acc_dirty = false;  // (a progressive frame in the old buffer is lost: reset before reuse)
    return forget_moments(ctx, stream);
}

// PTG_FLAG_MOMENTS passes: the second accumulator at the first one's size
// (ensure_acc first), zeroed on allocation like it
int ensure_acc2(ptg_context *ctx, hipStream_t stream)
{
    if (ctx->acc_elems <= ctx->acc2_elems)
        return PTG_OK;
    if (ctx->d_acc2)
        PTG_HIP(hipFree(ctx->d_acc2));
    ctx->d_acc2 = nullptr;
    ctx->acc2_elems = 0;
    if (hipMalloc(&ctx->d_acc2, ctx->acc_elems * sizeof(unsigned long long)) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the second-moment accumulator failed");
    PTG_HIP(hipMemsetAsync(ctx->d_acc2, 0, ctx->acc_elems * sizeof(unsigned long long), stream));
    ctx->acc2_elems = ctx->acc_elems;
    return PTG_OK;
}

// Both accumulators zero, no progressive frame in them (reset; a one-shot
// frame that needs the first accumulator after progressive passes)
int clear_accumulation(ptg_context *ctx, hipStream_t stream)
{
    if (ctx->d_acc)
        PTG_HIP(hipMemsetAsync(ctx->d_acc, 0, ctx->acc_elems * sizeof(unsigned long long), stream));
    ctx->acc_dirty = false;
    return forget_moments(ctx, stream);
}

// ptg_noise_device / ptg_read_moments_device: the second accumulator holds
// the squares of exactly the samples the first one holds
int check_moments(const ptg_context *ctx, const KArgs &A, const char *who)
{
    if (!ctx->moments_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": no PTG_FLAG_MOMENTS pass since the last reset");
    if (ctx->plain_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": a pass since the last reset ran without PTG_FLAG_MOMENTS");
    if (!ctx->d_acc2 || ctx->acc2_elems < acc_elems_for(A) || ctx->acc_elems < acc_elems_for(A))
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": the passes were of a smaller frame");
    return PTG_OK;
}

// While adaptive passes are in the sums, the pixels hold different numbers of
// samples: the entry points that take one n for the slab refuse ...
int refuse_after_adaptive(const ptg_context *ctx, const char *who)
{
    if (ctx->adaptive_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": adaptive passes since the last reset (the pixels "
                                              "hold different sample counts: use the *_active entry points, or reset)");
    return PTG_OK;
}

// ... and the adaptive ones after a uniform pass, which the count slab does not know of
int refuse_after_uniform(const ptg_context *ctx, const char *who)
{
    if (ctx->uniform_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": a ptg_accumulate_device pass since the last reset "
                                              "(the sample counts do not describe its sums: reset first)");
    return PTG_OK;
}

// PTG_FLAG_LIGHT_SAMPLING on a scene with more small emitters than the light list holds
int check_lights(const ptg_context *ctx, const ptg_params *p)
{
    if ((p->flags & PTG_FLAG_LIGHT_SAMPLING) && ctx->n_lights > kMaxLights)
        return fail(PTG_ERR_UNSUPPORTED, "light sampling: " + std::to_string(ctx->n_lights) +
                                             " small emitters, at most " + std::to_string(kMaxLights));
    return PTG_OK;
}

// The device entry points' common start, after their argument checks: the
// context's device current and the launch plan for samples [s_begin, s_end);
// with_acc: the exact accumulator at the plan's size as well.
int begin_launch(ptg_context *ctx, const ptg_params *p, KArgs &A, int &grid, hipStream_t s, bool with_acc,
                 int s_begin = 0, int s_end = -1, bool accumulate_only = false)
{
    PTG_HIP(hipSetDevice(ctx->device));
    int rc = check_lights(ctx, p);
    if (!rc)
        rc = fill_launch(ctx->base, ctx->wave_slots, p, A, grid, s_begin, s_end, accumulate_only);
    return rc || !with_acc ? rc : ensure_acc(ctx, acc_elems_for(A), s);
}

// a run-time bool as a compile-time one: f(std::true_type{}) or f(std::false_type{})
template <class F>
void with_bool(bool b, F &&f)
{
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// PTG_FLAG_STRATIFIED: the *_strat kernel of the launch (G: the gather kernel's)
int launch_strat(const KArgs &A, int grid, bool count, hipStream_t s, unsigned long long *acc2, const GatherArgs *G)
{
    const bool is_bvh = A.n > kLinearMax;
    const size_t lds = is_bvh ? 0 : (size_t)(A.n + 2 + 2) * sizeof(LinRec);
    with_bool(A.n_lights > 0, [&](auto ls) {
        with_bool(count, [&](auto cn) {
            with_bool(is_bvh, [&](auto bv) {
                with_bool(A.exact_math != 0, [&](auto ex) {
                    constexpr bool kL = decltype(ls)::value, kC = decltype(cn)::value, kB = decltype(bv)::value,
                                   kE = decltype(ex)::value;
                    constexpr int kBl = kB ? PTG_BVH_BLOCK : kBlock;
                    if (G)
                        gather_strat<kC, kB, kE, kL><<<grid, kBl, lds, s>>>(A, acc2, *G);
                    else if (acc2)
                        moments_strat<kC, kB, kE, kL><<<grid, kBl, lds, s>>>(A, acc2);
                    else
                        render_strat<kC, kB, kE, kL><<<grid, kBl, lds, s>>>(A);
                });
            });
        });
    });
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int launch_render(const KArgs &A, int grid, bool count, hipStream_t s, unsigned long long *acc2 = nullptr)
{
    if (grid <= 0)
        return PTG_OK;
    if (A.stratified)
        return launch_strat(A, grid, count, s, acc2, nullptr);
    const bool bvh = A.n > kLinearMax;
    const size_t lds = bvh ? 0 : (size_t)(A.n + 2 + 2) * sizeof(LinRec);
    // the exact mode's sin/cos table has its own LDS (render_kernel)
    // light sampling with lights to sample (n_lights is 0 without the flag): the ls kernels
    const int sel = (A.n_lights > 0 ? 16 : 0) | (acc2 ? 8 : 0) | (count ? 4 : 0) | (bvh ? 2 : 0) | (A.exact_math ? 1 : 0);
    switch (sel) {
    case 24: moments_ls<false, false, false><<<grid, kBlock, lds, s>>>(A, acc2); break;
    case 25: moments_ls<false, true, false><<<grid, kBlock, lds, s>>>(A, acc2); break;
    case 26: moments_ls<true, false, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2); break;
    case 27: moments_ls<true, true, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2); break;
    case 28: moments_ls<false, false, true><<<grid, kBlock, lds, s>>>(A, acc2); break;
    case 29: moments_ls<false, true, true><<<grid, kBlock, lds, s>>>(A, acc2); break;
    case 30: moments_ls<true, false, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2); break;
    case 31: moments_ls<true, true, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2); break;
    case 16: render_ls<false, false, false><<<grid, kBlock, lds, s>>>(A); break;
    case 17: render_ls<false, false, true><<<grid, kBlock, lds, s>>>(A); break;
    case 18: render_ls<false, true, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A); break;
    case 19: render_ls<false, true, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A); break;
    case 20: render_ls<true, false, false><<<grid, kBlock, lds, s>>>(A); break;
    case 21: render_ls<true, false, true><<<grid, kBlock, lds, s>>>(A); break;
    case 22: render_ls<true, true, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A); break;
    case 23: render_ls<true, true, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A); break;
    case 8: moments_kernel<false, false, false><<<grid, kBlock, lds, s>>>(A, acc2); break;
    case 9: moments_kernel<false, true, false><<<grid, kBlock, lds, s>>>(A, acc2); break;
    case 10: moments_kernel<true, false, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2); break;
    case 11: moments_kernel<true, true, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2); break;
    case 12: moments_kernel<false, false, true><<<grid, kBlock, lds, s>>>(A, acc2); break;
    case 13: moments_kernel<false, true, true><<<grid, kBlock, lds, s>>>(A, acc2); break;
    case 14: moments_kernel<true, false, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2); break;
    case 15: moments_kernel<true, true, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2); break;
    case 0: render_kernel<false, false, false><<<grid, kBlock, lds, s>>>(A); break;
    case 1: render_kernel<false, false, true><<<grid, kBlock, lds, s>>>(A); break;
    case 2: render_kernel<false, true, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A); break;
    case 3: render_kernel<false, true, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A); break;
    case 4: render_kernel<true, false, false><<<grid, kBlock, lds, s>>>(A); break;
    case 5: render_kernel<true, false, true><<<grid, kBlock, lds, s>>>(A); break;
    case 6: render_kernel<true, true, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A); break;
    default: render_kernel<true, true, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A); break;
    }
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

// PTG_FLAG_REFERENCE_F64: the reference's double arithmetic (ref64.hpp), one
// lane per sub-pixel; out64 or out32 receives the slab
int launch_ref64(const ptg_context *ctx, const KArgs &A, double *out64, float *out32,
                 unsigned long long *d_segments, hipStream_t s)
{
    ref64::Args R{};
    R.spheres = ctx->d_sph64;
    R.n = ctx->n;
    R.cam = ctx->cam64;
    R.W = A.W;
    R.H = A.H;
    R.samps = A.samps;
    R.nsub = A.nsub;
    R.lanes_per_pixel = A.lanes_per_pixel;
    R.pixels_per_wave = A.pixels_per_wave;
    R.waves_per_row = A.waves_per_row;
    R.slab_rows = A.slab_rows;
    R.band_rows = A.band_rows;
    R.shard_rank = A.shard_rank;
    R.shard_count = A.shard_count;
    R.seed = A.seed;
    R.out64 = out64;
    R.out32 = out32;
    R.segments = d_segments;
    R.n_lights = A.n_lights;  // (0 without PTG_FLAG_LIGHT_SAMPLING: plan_frame)
    R.stratified = A.stratified;
    for (int k = 0; k < A.n_lights; ++k)
        R.lights[k] = ctx->light_ids[k];
    const long long waves = (long long)A.slab_rows * A.waves_per_row;
    const long long blocks = (waves + 3) / 4;
    if (blocks > 0x7FFFFFFFLL)
        return fail(PTG_ERR_UNSUPPORTED, "image too large for the reference-arithmetic mode");
    if (blocks > 0)
        ref64::render_kernel<<<(unsigned)blocks, 256, 0, s>>>(R);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int launch_gather(const KArgs &A, int grid, bool count, hipStream_t s, unsigned long long *acc2, const GatherArgs &G)
{
    if (grid <= 0)
        return PTG_OK;
    if (A.stratified)
        return launch_strat(A, grid, count, s, acc2, &G);
    const bool bvh = A.n > kLinearMax;
    const size_t lds = bvh ? 0 : (size_t)(A.n + 2 + 2) * sizeof(LinRec);
    switch ((A.n_lights > 0 ? 8 : 0) | (count ? 4 : 0) | (bvh ? 2 : 0) | (A.exact_math ? 1 : 0)) {
    case 8: gather_ls<false, false, false><<<grid, kBlock, lds, s>>>(A, acc2, G); break;
    case 9: gather_ls<false, true, false><<<grid, kBlock, lds, s>>>(A, acc2, G); break;
    case 10: gather_ls<true, false, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2, G); break;
    case 11: gather_ls<true, true, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2, G); break;
    case 12: gather_ls<false, false, true><<<grid, kBlock, lds, s>>>(A, acc2, G); break;
    case 13: gather_ls<false, true, true><<<grid, kBlock, lds, s>>>(A, acc2, G); break;
    case 14: gather_ls<true, false, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2, G); break;
    case 15: gather_ls<true, true, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2, G); break;
    case 0: gather_kernel<false, false, false><<<grid, kBlock, lds, s>>>(A, acc2, G); break;
    case 1: gather_kernel<false, true, false><<<grid, kBlock, lds, s>>>(A, acc2, G); break;
    case 2: gather_kernel<true, false, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2, G); break;
    case 3: gather_kernel<true, true, false><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2, G); break;
    case 4: gather_kernel<false, false, true><<<grid, kBlock, lds, s>>>(A, acc2, G); break;
    case 5: gather_kernel<false, true, true><<<grid, kBlock, lds, s>>>(A, acc2, G); break;
    case 6: gather_kernel<true, false, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2, G); break;
    default: gather_kernel<true, true, true><<<grid, PTG_BVH_BLOCK, 0, s>>>(A, acc2, G); break;
    }
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

// The adaptive buffers at the frame's size (allocated on first use; a larger
// frame replaces them: counts zero, no list)
int ensure_adaptive(ptg_context *ctx, const KArgs &A, hipStream_t stream)
{
    const size_t pixels = (size_t)A.slab_rows * A.W, rows = (size_t)A.slab_rows, groups = (size_t)A.n_groups;
    if (pixels <= ctx->ad_pixels && rows <= ctx->ad_rows && groups <= ctx->ad_groups)
        return PTG_OK;
    if (ctx->adaptive_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT, "the adaptive passes since the last reset were of a smaller frame");
    for (void **q : {(void **)&ctx->d_counts, (void **)&ctx->d_over, (void **)&ctx->d_list, (void **)&ctx->d_row_count,
                     (void **)&ctx->d_row_unit0, (void **)&ctx->d_units, (void **)&ctx->d_rec}) {
        if (*q)
            PTG_HIP(hipFree(*q));
        *q = nullptr;
    }
    ctx->ad_pixels = ctx->ad_rows = ctx->ad_groups = 0;
    ctx->list_valid = false;
    if (hipMalloc(&ctx->d_counts, pixels * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&ctx->d_over, pixels) != hipSuccess || hipMalloc(&ctx->d_list, pixels * sizeof(int)) != hipSuccess ||
        hipMalloc(&ctx->d_row_count, rows * sizeof(int)) != hipSuccess ||
        hipMalloc(&ctx->d_row_unit0, rows * sizeof(int)) != hipSuccess ||
        hipMalloc(&ctx->d_units, groups * sizeof(int4)) != hipSuccess ||
        hipMalloc(&ctx->d_rec, 2 * sizeof(unsigned long long)) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the adaptive-sampling buffers failed");
    PTG_HIP(hipMemsetAsync(ctx->d_counts, 0, pixels * sizeof(int32_t), stream));
    PTG_HIP(hipMemsetAsync(ctx->d_rec, 0, 2 * sizeof(unsigned long long), stream));
    ctx->ad_pixels = pixels;
    ctx->ad_rows = rows;
    ctx->ad_groups = groups;
    return PTG_OK;
}

// the slab geometry of two frames is the same (the active list and the counts are indexed by it)
bool same_slab(const ptg_params &a, const ptg_params &b)
{
    return a.width == b.width && a.height == b.height && a.num_subpixels == b.num_subpixels &&
           a.band_rows == b.band_rows && a.shard_rank == b.shard_rank && a.shard_count == b.shard_count;
}

// The adaptive entry points' common start: argument checks done, no uniform
// pass in the sums, the launch plan's frame fields, both accumulators and the
// adaptive buffers at the frame's size.
int begin_adaptive(ptg_context *ctx, const ptg_params *p, KArgs &A, hipStream_t s, const char *who)
{
    if (p->flags & PTG_FLAG_REFERENCE_F64)
        return fail(PTG_ERR_UNSUPPORTED, std::string(who) + ": progressive passes are fp32 only");
    int rc = refuse_after_uniform(ctx, who), grid = 0;
    if (rc || (rc = begin_launch(ctx, p, A, grid, s, /*with_acc=*/true)) || (rc = ensure_acc2(ctx, s)))
        return rc;
    A.acc = ctx->d_acc;
    return ensure_adaptive(ctx, A, s);
}

// List-building steps 2 and 3 after step 1: list_rows_kernel on `flags`, or,
// gathered, list_rows_gathered_kernel on the whole frame's rank-major slabs
int build_list(ptg_context *ctx, const ptg_params *p, const KArgs &A, const uint8_t *flags, int dilate,
               unsigned long long *d_info, unsigned long long *d_stats, hipStream_t s, bool gathered = false)
{
    if (A.slab_rows > 0) {
        if (gathered)
            list_rows_gathered_kernel<<<A.slab_rows, 256, 0, s>>>(A, flags, dilate, ctx->d_list, ctx->d_row_count);
        else
            list_rows_kernel<<<A.slab_rows, 256, 0, s>>>(A, flags, dilate, ctx->d_list, ctx->d_row_count);
        PTG_HIP(hipGetLastError());
    }
    list_units_kernel<<<1, 256, 0, s>>>(A.slab_rows, A.pixels_per_wave, ctx->d_row_count, ctx->d_row_unit0, ctx->d_rec,
                                        d_info, d_stats);
    PTG_HIP(hipGetLastError());
    if (A.slab_rows > 0) {
        list_fill_kernel<<<A.slab_rows, 256, 0, s>>>(A.pixels_per_wave, ctx->d_row_count, ctx->d_row_unit0, ctx->d_units);
        PTG_HIP(hipGetLastError());
    }
    ctx->list_frame = *p;
    ctx->list_valid = true;
    return PTG_OK;
}

int launch_resolve(const KArgs &A, hipStream_t s)
{
    long long pixels = (long long)(A.slab_rows - A.resolve_row0) * A.W;
    if (pixels <= 0)
        return PTG_OK;
    resolve_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, s>>>(A);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

}  // namespace

extern "C" {

int ptg_render_device(ptg_context *ctx, const ptg_params *params, float *d_slab, unsigned long long *d_segments,
                      void *stream)
{
    if (!ctx || !d_slab)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/false)))
        return rc;
    if (params->flags & PTG_FLAG_REFERENCE_F64)
        return launch_ref64(ctx, A, nullptr, d_slab, d_segments, s);
    // several units per pixel, a split tail accumulated in HBM, or no samples at all
    const bool resolve = A.needs_resolve || grid == 0;
    if ((rc = ensure_acc(ctx, resolve ? acc_elems_for(A) : 0, s)))
        return rc;
    A.out = d_slab;
    A.acc = ctx->d_acc;
    A.segments = d_segments;
    if (resolve && ctx->acc_dirty) {
        // progressive sums left by accumulate / keep_acc resolve: a one-shot
        // frame starts from zero (its resolve leaves the buffer zero again)
        if ((rc = clear_accumulation(ctx, s)))
            return rc;
    }
    if ((rc = launch_render(A, grid, d_segments != nullptr, s)))
        return rc;
    return resolve ? launch_resolve(A, s) : PTG_OK;
}

int ptg_launch_info(ptg_context *ctx, const ptg_params *params, int64_t *info, int n_info)
{
    if (!ctx || !info || n_info < 1)
        return fail(PTG_ERR_INVALID_ARGUMENT, "launch_info: NULL argument");
    int rc = check_params(params);
    if (rc)
        return rc;
    KArgs A;
    int grid = 0;
    if ((rc = fill_launch(ctx->base, ctx->wave_slots, params, A, grid)))
        return rc;
    const bool bvh = ctx->n > kLinearMax;
    const int64_t v[PTG_LAUNCH_INFO_COUNT] = {
        bvh ? 0 : A.box_mode, bvh ? 0 : A.box_walls_out, bvh ? 1 : 0, A.n_units, grid, A.n_levels,
        A.needs_resolve ? 1 : 0, (int64_t)(A.pairs[0] | (A.pairs[1] << 1) | (A.pairs[2] << 2))};
    for (int i = 0; i < n_info; ++i)
        info[i] = i < PTG_LAUNCH_INFO_COUNT ? v[i] : 0;
    return PTG_OK;
}

int ptg_accumulate_device(ptg_context *ctx, const ptg_params *params, int32_t sample_begin, int32_t sample_end,
                          unsigned long long *d_segments, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (sample_begin < 0 || sample_end < sample_begin || sample_end > params->samples)
        return fail(PTG_ERR_INVALID_ARGUMENT, "sample range must satisfy 0 <= begin <= end <= samples");
    if (params->flags & PTG_FLAG_REFERENCE_F64)
        return fail(PTG_ERR_UNSUPPORTED, "progressive passes are fp32 only (the reference-arithmetic mode sums "
                                         "its samples sequentially, main.cpp:192)");
    if ((rc = refuse_after_adaptive(ctx, "accumulate")))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true, sample_begin, sample_end,
                           /*accumulate_only=*/true)))
        return rc;
    const bool moments = (params->flags & PTG_FLAG_MOMENTS) != 0;
    if (moments && (rc = ensure_acc2(ctx, s)))
        return rc;
    A.acc = ctx->d_acc;
    A.segments = d_segments;
    ctx->acc_dirty = true;
    if (grid > 0)  // (an empty pass adds no samples to either accumulator)
        (moments ? ctx->moments_pass : ctx->plain_pass) = ctx->uniform_pass = true;
    return launch_render(A, grid, d_segments != nullptr, s, moments ? ctx->d_acc2 : nullptr);
}

int ptg_resolve_device(ptg_context *ctx, const ptg_params *params, int32_t samples_done, float *d_slab, void *stream)
{
    if (!ctx || !d_slab)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (samples_done < 0 || samples_done > params->samples)
        return fail(PTG_ERR_INVALID_ARGUMENT, "samples_done must be in [0, samples]");
    if ((rc = refuse_after_adaptive(ctx, "resolve")))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true)))
        return rc;
    A.samps = samples_done;  // mean over the samples accumulated so far
    A.keep_acc = 1;
    A.resolve_row0 = 0;  // every row (the one-shot split tail does not apply here)
    A.acc = ctx->d_acc;
    A.out = d_slab;
    return launch_resolve(A, s);
}

int ptg_reset_accumulation_device(ptg_context *ctx, const ptg_params *params, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true)))
        return rc;
    return clear_accumulation(ctx, s);
}

int ptg_noise_device(ptg_context *ctx, const ptg_params *params, int32_t samples_done, double rel_error, double floor,
                     float *d_var, float *d_rho, unsigned long long *d_stats, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (samples_done < 2 || samples_done > params->samples)
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise: samples_done must be in [2, samples]");
    if (!(floor > 0.0) || !(rel_error >= 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise: floor must be > 0 and rel_error >= 0");
    if ((rc = refuse_after_adaptive(ctx, "noise")))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true)) || (rc = check_moments(ctx, A, "noise")))
        return rc;
    A.samps = samples_done;
    A.acc = ctx->d_acc;
    const long long pixels = (long long)A.slab_rows * A.W;
    if (pixels <= 0 || (!d_var && !d_rho && !d_stats))
        return PTG_OK;
    const long long blocks = (pixels + 255) / 256;  // the kernel strides over the rest
    noise_kernel<<<(unsigned)(blocks < kNoiseBlocks ? blocks : kNoiseBlocks), 256, 0, s>>>(
        A, ctx->d_acc2, rel_error, floor, d_var, d_rho, d_stats);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_read_moments_device(ptg_context *ctx, const ptg_params *params, unsigned long long *d_sum,
                            unsigned long long *d_sumsq, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true)))
        return rc;
    const size_t bytes = acc_elems_for(A) * sizeof(unsigned long long);
    if (d_sumsq) {
        if ((rc = check_moments(ctx, A, "read_moments")))
            return rc;
        PTG_HIP(hipMemcpyAsync(d_sumsq, ctx->d_acc2, bytes, hipMemcpyDeviceToDevice, s));
    }
    if (d_sum)
        PTG_HIP(hipMemcpyAsync(d_sum, ctx->d_acc, bytes, hipMemcpyDeviceToDevice, s));
    return PTG_OK;
}

int ptg_set_active_mask_device(ptg_context *ctx, const ptg_params *params, const uint8_t *d_mask,
                               unsigned long long *d_info, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "set_active_mask")))
        return rc;
    return build_list(ctx, params, A, d_mask, 0, d_info, nullptr, s);
}

int ptg_select_active_device(ptg_context *ctx, const ptg_params *params, double rel_error, double floor,
                             int32_t dilate, float *d_rho, unsigned long long *d_stats, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (!(floor > 0.0) || !(rel_error >= 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, "select_active: floor must be > 0 and rel_error >= 0");
    if (dilate < 0 || dilate > 8)
        return fail(PTG_ERR_INVALID_ARGUMENT, "select_active: dilate must be in [0, 8]");
    if (dilate > 0 && params->shard_count > 1)
        return fail(PTG_ERR_UNSUPPORTED, "select_active: dilate > 0 needs shard_count 1 (the neighbouring rows "
                                         "live in other shards)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "select_active")))
        return rc;
    const long long pixels = (long long)A.slab_rows * A.W;
    const long long blocks = (pixels + 255) / 256;  // the kernel strides over the rest
    select_over_kernel<<<(unsigned)(blocks < kNoiseBlocks ? blocks : kNoiseBlocks), 256, 0, s>>>(
        A, ctx->d_acc2, ctx->d_counts, rel_error, floor, ctx->d_over, d_rho, d_stats);
    PTG_HIP(hipGetLastError());
    return build_list(ctx, params, A, ctx->d_over, dilate, nullptr, d_stats, s);
}

int ptg_select_over_device(ptg_context *ctx, const ptg_params *params, double rel_error, double floor,
                           uint8_t *d_over, float *d_rho, unsigned long long *d_stats, void *stream)
{
    if (!ctx || !d_over)
        return fail(PTG_ERR_INVALID_ARGUMENT, "select_over: NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (!(floor > 0.0) || !(rel_error >= 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, "select_over: floor must be > 0 and rel_error >= 0");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "select_over")))
        return rc;
    const long long pixels = (long long)A.slab_rows * A.W;
    const long long blocks = (pixels + 255) / 256;  // the kernel strides over the rest
    select_over_kernel<<<(unsigned)(blocks < kNoiseBlocks ? blocks : kNoiseBlocks), 256, 0, s>>>(
        A, ctx->d_acc2, ctx->d_counts, rel_error, floor, d_over, d_rho, d_stats);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_noise_active_device(ptg_context *ctx, const ptg_params *params, double floor, float *d_var, float *d_rho,
                            void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (!(floor > 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise_active: floor must be > 0");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "noise_active")))
        return rc;
    const long long pixels = (long long)A.slab_rows * A.W;
    if (pixels <= 0 || (!d_var && !d_rho))
        return PTG_OK;
    const long long blocks = (pixels + 255) / 256;  // the kernel strides over the rest
    noise_active_kernel<<<(unsigned)(blocks < kNoiseBlocks ? blocks : kNoiseBlocks), 256, 0, s>>>(
        A, ctx->d_acc2, ctx->d_counts, floor, d_var, d_rho);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_set_active_gathered_device(ptg_context *ctx, const ptg_params *params, const uint8_t *d_over_gathered,
                                   int32_t dilate, unsigned long long *d_stats, void *stream)
{
    if (!ctx || !d_over_gathered)
        return fail(PTG_ERR_INVALID_ARGUMENT, "set_active_gathered: NULL context or over bytes");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (dilate < 0 || dilate > kMaxDilate)
        return fail(PTG_ERR_INVALID_ARGUMENT, "set_active_gathered: dilate must be in [0, 8]");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "set_active_gathered")))
        return rc;
    return build_list(ctx, params, A, d_over_gathered, dilate, nullptr, d_stats, s, /*gathered=*/true);
}

int ptg_accumulate_active_device(ptg_context *ctx, const ptg_params *params, int32_t add_samples, long long max_units,
                                 unsigned long long *d_segments, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (add_samples < 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "accumulate_active: add_samples must be >= 0");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "accumulate_active")))
        return rc;
    if (!ctx->list_valid)
        return fail(PTG_ERR_INVALID_ARGUMENT, "accumulate_active: no active list since the last reset "
                                              "(ptg_set_active_mask_device or ptg_select_active_device first)");
    if (!same_slab(ctx->list_frame, *params))
        return fail(PTG_ERR_INVALID_ARGUMENT, "accumulate_active: the active list was built for another frame");
    if (ctx->adaptive_added + add_samples > (1LL << 30))
        return fail(PTG_ERR_INVALID_ARGUMENT, "accumulate_active: a sample count could pass 2^30 (" +
                                                  std::to_string(ctx->adaptive_added) + " added since the last reset)");
    if (add_samples == 0)
        return PTG_OK;
    const long long bound = max_units <= 0 || max_units > A.n_groups ? (long long)A.n_groups : max_units;
    ActivePlan P;
    if ((rc = plan_active(A.n > kLinearMax, ctx->wave_slots, bound, add_samples, params->chunk_samples, P)))
        return rc;
    // the kernel's frame: local samples [0, add_samples) in chunks of P.chunk, every unit accumulates
    A.sample_begin = 0;
    A.sample_end = add_samples;
    plan_single_level(A, P.chunk, add_samples, /*one_shot=*/false);
    A.n_units = P.n_units;
    A.segments = d_segments;
    const GatherArgs G{ctx->d_units, ctx->d_list, ctx->d_counts, ctx->d_rec, bound, P.n_chunks};
    ctx->acc_dirty = true;
    ctx->adaptive_pass = ctx->moments_pass = true;
    ctx->adaptive_added += add_samples;
    if ((rc = launch_gather(A, P.grid, d_segments != nullptr, s, ctx->d_acc2, G)))
        return rc;
    const long long blocks = (bound + 3) / 4;
    bump_counts_kernel<<<(unsigned)(blocks < kNoiseBlocks ? blocks : kNoiseBlocks), 256, 0, s>>>(
        A.W, ctx->d_units, ctx->d_list, ctx->d_rec, bound, add_samples, ctx->d_counts);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_resolve_active_device(ptg_context *ctx, const ptg_params *params, float *d_slab, void *stream)
{
    if (!ctx || !d_slab)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "resolve_active")))
        return rc;
    A.out = d_slab;
    const long long pixels = (long long)A.slab_rows * A.W;
    if (pixels <= 0)
        return PTG_OK;
    resolve_active_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, s>>>(A, ctx->d_counts);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_read_sample_counts_device(ptg_context *ctx, const ptg_params *params, int32_t *d_counts, void *stream)
{
    if (!ctx || !d_counts)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "read_sample_counts")))
        return rc;
    PTG_HIP(hipMemcpyAsync(d_counts, ctx->d_counts, (size_t)A.slab_rows * A.W * sizeof(int32_t),
                           hipMemcpyDeviceToDevice, s));
    return PTG_OK;
}

int ptg_noise_schedule(int32_t min_samples, int32_t samples, int32_t *ends, int32_t cap, int32_t *n)
{
    if (!ends || !n)
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise_schedule: NULL argument");
    *n = 0;
    if (min_samples < 2 || samples < 2)
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise_schedule: min_samples and samples must be >= 2 (a variance "
                                              "needs two samples)");
    int32_t k = 0;
    for (int64_t e = min_samples; e < samples; e *= 2, ++k)
        if (k < cap)
            ends[k] = (int32_t)e;
    if (k < cap)
        ends[k] = samples;
    ++k;
    if (k > cap)
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise_schedule: " + std::to_string(k) + " passes, room for " +
                                                  std::to_string(cap));
    *n = k;
    return PTG_OK;
}

int ptg_trace_samples_device(ptg_context *ctx, const ptg_params *params, const int32_t *d_coords, size_t n,
                             float *d_out, int32_t *d_segs, void *stream)
{
    if (!ctx || (n && (!d_coords || !d_out || !d_segs)))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (n == 0)
        return PTG_OK;
    if (params->flags & PTG_FLAG_REFERENCE_F64)
        return fail(PTG_ERR_UNSUPPORTED, "trace_samples probes the fp32 kernel");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/false)))
        return rc;
    int blocks = (int)((n + kTraceBlock - 1) / kTraceBlock);
    const bool bvh = A.n > kLinearMax;
    if (A.stratified) {
        with_bool(A.n_lights > 0, [&](auto ls) {
            with_bool(bvh, [&](auto bv) {
                with_bool(A.exact_math != 0, [&](auto ex) {
                    trace_strat<decltype(bv)::value, decltype(ex)::value, decltype(ls)::value>
                        <<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs);
                });
            });
        });
    } else if (A.n_lights > 0) {  // light sampling with lights to sample
        if (A.exact_math)
            bvh ? trace_kernel<true, true, true><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs)
                : trace_kernel<false, true, true><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs);
        else
            bvh ? trace_kernel<true, false, true><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs)
                : trace_kernel<false, false, true><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs);
    } else if (A.exact_math)
        bvh ? trace_kernel<true, true><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs)
            : trace_kernel<false, true><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs);
    else
        bvh ? trace_kernel<true, false><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs)
            : trace_kernel<false, false><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_sampler_pairs_device(ptg_context *ctx, const ptg_params *params, const int32_t *d_coords, size_t n,
                             uint32_t *d_out, void *stream)
{
    if (!ctx || (n && (!d_coords || !d_out)))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (n > (size_t)INT32_MAX / 8)
        return fail(PTG_ERR_UNSUPPORTED, "too many records");
    if (n == 0)
        return PTG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/false)))
        return rc;
    sampler_pairs_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(A, d_coords, (int)n, d_out);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_features_device(ptg_context *ctx, const ptg_params *params, float *d_feat, void *stream)
{
    if (!ctx || !d_feat)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: NULL context or output");
    if (reinterpret_cast<uintptr_t>(d_feat) % 16)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: the output must be 16-byte aligned");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    // the frame's geometry only: the scan's fields are those of the exact mode whatever the flags
    ptg_params geo = *params;
    geo.samples = 1;
    geo.chunk_samples = 0;
    geo.flags = PTG_FLAG_EXACT_MATH;
    if ((rc = begin_launch(ctx, &geo, A, grid, s, /*with_acc=*/false)))
        return rc;
    const long long pixels = (long long)A.slab_rows * A.W;
    const unsigned blocks = (unsigned)((pixels + 255) / 256);
    if (A.n > kLinearMax)
        features_kernel<true><<<blocks, 256, 0, s>>>(A, reinterpret_cast<float4 *>(d_feat));
    else
        features_kernel<false><<<blocks, 256, 0, s>>>(A, reinterpret_cast<float4 *>(d_feat));
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_features_follow_device(ptg_context *ctx, const ptg_params *params, int32_t max_bounces, float *d_feat,
                               void *stream)
{
    if (max_bounces < 0 || max_bounces > PTG_MAX_FOLLOW_BOUNCES)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: max_bounces must be 0..16");
    if (!ctx || !d_feat)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: NULL context or output");
    if (reinterpret_cast<uintptr_t>(d_feat) % 16)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: the output must be 16-byte aligned");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    // the frame's geometry only, as ptg_features_device plans it
    ptg_params geo = *params;
    geo.samples = 1;
    geo.chunk_samples = 0;
    geo.flags = PTG_FLAG_EXACT_MATH;
    if ((rc = begin_launch(ctx, &geo, A, grid, s, /*with_acc=*/false)))
        return rc;
    const long long pixels = (long long)A.slab_rows * A.W;
    const unsigned blocks = (unsigned)((pixels + 255) / 256);
    if (A.n > kLinearMax)
        features_follow_kernel<true><<<blocks, 256, 0, s>>>(A, max_bounces, reinterpret_cast<float4 *>(d_feat));
    else
        features_follow_kernel<false><<<blocks, 256, 0, s>>>(A, max_bounces, reinterpret_cast<float4 *>(d_feat));
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_math_probe_device(ptg_context *ctx, int32_t op, int32_t exact, const float *d_in, float *d_out, size_t n,
                          void *stream)
{
    if (!ctx || (n && (!d_in || !d_out)))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (op < PTG_PROBE_SQRT || op > PTG_PROBE_SINCOS)
        return fail(PTG_ERR_INVALID_ARGUMENT, "unknown probe op");
    if (n > (size_t)INT32_MAX / 2)
        return fail(PTG_ERR_UNSUPPORTED, "too many operands");
    if (n == 0)
        return PTG_OK;
    PTG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (exact)
        math_probe_kernel<true><<<blocks, 256, 0, s>>>(op, d_in, d_out, (int)n, ctx->d_trig);
    else
        math_probe_kernel<false><<<blocks, 256, 0, s>>>(op, d_in, d_out, (int)n, ctx->d_trig);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_unshard_device(const float *d_gathered, float *d_image, int32_t width, int32_t height, int32_t band_rows,
                       int32_t shard_count, void *stream)
{
    if (!d_gathered || !d_image || width <= 0 || height <= 0 || band_rows <= 0 || shard_count <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "invalid unshard arguments");
    if (height > 65535)
        return fail(PTG_ERR_UNSUPPORTED, "height > 65535");
    int32_t slab_rows = 0;
    ptg_shard_rows(height, band_rows, shard_count, &slab_rows);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int bx = std::max(1, std::min(64, (width * 3 + 255) / 256));
    unshard_kernel<<<dim3(bx, height), 256, 0, s>>>(d_gathered, d_image, width, band_rows, shard_count, slab_rows);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_tonemap_device(const float *d_image, uint8_t *d_out, size_t count, void *stream)
{
    if (!d_image || !d_out)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (count == 0)
        return PTG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    size_t blocks = (count + 255) / 256;
    tonemap_kernel<<<(unsigned)blocks, 256, 0, s>>>(d_image, d_out, count);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_render(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
               int device, double *image_rgb)
{
    if (!image_rgb)
        return fail(PTG_ERR_INVALID_ARGUMENT, "image is NULL");
    int rc = check_params(params);
    if (rc)
        return rc;
    ptg_context *ctx = nullptr;
    rc = ptg_context_create(spheres, n_spheres, cam, device, &ctx);
    if (rc)
        return rc;
    KArgs A;  // the frame's plan: the slab's geometry (and the reference-arithmetic mode's launch)
    int grid = 0;
    if ((rc = check_lights(ctx, params)) || (rc = fill_launch(ctx->base, ctx->wave_slots, params, A, grid))) {
        ptg_context_destroy(ctx);
        return rc;
    }
    const int slab_rows = A.slab_rows;
    size_t slab_elems = (size_t)slab_rows * params->width * 3;
    // the reference-arithmetic mode keeps its doubles to the host image
    const bool f64 = (params->flags & PTG_FLAG_REFERENCE_F64) != 0;
    const size_t esz = f64 ? sizeof(double) : sizeof(float);
    void *d_slab = nullptr;
    std::vector<unsigned char> host(slab_elems * esz);
    rc = PTG_OK;
    if (hipMalloc(&d_slab, slab_elems * esz) != hipSuccess) {
        ptg_context_destroy(ctx);
        return fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the image slab failed");
    }
    if (f64)
        rc = launch_ref64(ctx, A, static_cast<double *>(d_slab), nullptr, nullptr, nullptr);
    else
        rc = ptg_render_device(ctx, params, static_cast<float *>(d_slab), nullptr, nullptr);
    if (rc == PTG_OK) {
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess)
            e = hipMemcpy(host.data(), d_slab, slab_elems * esz, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            rc = fail(PTG_ERR_HIP, std::string("render: ") + hipGetErrorString(e));
    }
    (void)hipFree(d_slab);
    ptg_context_destroy(ctx);
    if (rc)
        return rc;
    const int W = params->width, H = params->height;
    for (int j = 0; j < slab_rows; ++j) {
        const int r = out_row_of(A, j);
        if (r >= H)
            continue;
        double *dst = image_rgb + (size_t)r * W * 3;
        const size_t off = (size_t)j * W * 3;
        if (f64)
            ptg_frames::add_image(dst, reinterpret_cast<const double *>(host.data()) + off, (size_t)W * 3);
        else
            ptg_frames::add_image(dst, reinterpret_cast<const float *>(host.data()) + off, (size_t)W * 3);
    }
    return PTG_OK;
}

}  // extern "C"
