// scan_linear.hpp -- the nearest-hit scan of linear scenes (up to kLinearMax
// spheres, records in LDS): scene_scan with its box mode, and ScanCount, the
// test counters both scans fill.  Included by ptg_render.hip inside its
// unnamed namespace, after render_config.hpp; needs KArgs and LinRec
// (kernel_args.hpp), f3 and Math (pt_device.hpp) and PTG_STAT.  Owns
// PTG_ASSUME_BOX_MODE; reads PTG_BLOCK_STATS.
#pragma once

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
