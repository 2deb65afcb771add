// scene_prep.hpp -- host-side scene preparation: what ptg_context_create
// uploads and the scene fields of KArgs.  Plain C++, no HIP API calls, so a
// stand-alone program can run it on the CPU (tests/launch_plan_check.cpp).
//   prepare_scene          double -> fp32 records in scene index order
//   prepare_linear_upload  linear scenes: scan order, wall pairs, box mode and
//                          the record table the linear kernel stages in LDS
//   prepare_bvh_upload     BVH scenes: the 8 interleaved wide layouts, leaf
//                          and huge-sphere records in one blob
// The oracle's Mode B (oracle/pt_oracle.c prep_B) makes the same choices.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bvh_build.hpp"
#include "kernel_args.hpp"

namespace {

inline bool sphere_ok(const ptg_sphere &s)
{
    if (!(s.radius > 0.0) || !std::isfinite(s.radius))
        return false;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(s.position[c]) || !std::isfinite(s.emission[c]) || !std::isfinite(s.color[c]))
            return false;
    return s.material >= PTG_DIFFUSE && s.material <= PTG_DIELECTRIC;
}

// Anchor of a huge sphere (DESIGN.md "Huge spheres"): the point P = C + R n0
// of the sphere and its outward normal n0.  The default n0 is the unit vector
// from C towards the camera.  When the point C + s R e_k of the dominant axis
// direction of that n0 (k = largest |n0_k|, s = its sign) lies near the scene
// -- within max(diagonal, 1) of the box around the camera and the non-huge
// spheres -- that axis point is the anchor instead: any point of the sphere is
// an exact anchor, and one near the scene keeps |o - P| at scene scale (box
// walls: the axis points lie inside that box).  Returns k, or -1 for the
// camera-facing anchor.  The oracle's prep_B makes the same choice
// (oracle/pt_oracle.c: choose_anchor_B).
struct SceneBox {
    double lo[3], hi[3], diag;
};

inline int choose_anchor(const ptg_sphere &sp, const ptg_camera *cam, const SceneBox &box, double P[3], double N[3])
{
    const double R = sp.radius;
    double v[3], len2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        v[c] = cam->position[c] - sp.position[c];
        len2 += v[c] * v[c];
    }
    const double len = std::sqrt(len2);
    for (int c = 0; c < 3; ++c)
        N[c] = len > 0.0 ? v[c] / len : (c == 1 ? 1.0 : 0.0);
    int k = 0;
    for (int c = 1; c < 3; ++c)
        if (std::fabs(N[c]) > std::fabs(N[k]))
            k = c;
    const double s = N[k] >= 0.0 ? 1.0 : -1.0;
    double out2 = 0.0;  // squared distance of the axis point from the scene box
    for (int c = 0; c < 3; ++c) {
        const double pa = sp.position[c] + (c == k ? s * R : 0.0);
        const double o = pa < box.lo[c] ? box.lo[c] - pa : (pa > box.hi[c] ? pa - box.hi[c] : 0.0);
        out2 += o * o;
    }
    const bool snap = std::sqrt(out2) <= std::max(box.diag, 1.0);
    for (int c = 0; c < 3; ++c) {
        if (snap)
            N[c] = c == k ? s : 0.0;
        P[c] = sp.position[c] + R * N[c];
    }
    return snap ? k : -1;
}

// Box around the camera and every non-huge sphere, and its diagonal.
// Computed once per scene and passed down.
inline SceneBox scene_box(const ptg_sphere *s, int n, const ptg_camera *cam)
{
    SceneBox b;
    for (int c = 0; c < 3; ++c)
        b.lo[c] = b.hi[c] = cam->position[c];
    for (int i = 0; i < n; ++i) {
        if (is_huge(s[i], cam))
            continue;
        for (int c = 0; c < 3; ++c) {
            b.lo[c] = std::min(b.lo[c], s[i].position[c] - s[i].radius);
            b.hi[c] = std::max(b.hi[c], s[i].position[c] + s[i].radius);
        }
    }
    double d2 = 0.0;
    for (int c = 0; c < 3; ++c)
        d2 += (b.hi[c] - b.lo[c]) * (b.hi[c] - b.lo[c]);
    b.diag = std::sqrt(d2);
    return b;
}

// The scene in fp32 records, scene index order.  axis[i] = anchor axis of a
// huge sphere (-1: camera-facing anchor or not huge).
struct SceneRecs {
    SceneBox box;
    std::vector<GeoRec> geo;
    std::vector<ShadeRec> shade;
    std::vector<int> axis;
};

// Host-side preparation (double -> fp32 records, scene index order), the
// counterpart of the oracle's Mode B prep_B.
inline SceneRecs prepare_scene(const ptg_sphere *s, int n, const ptg_camera *cam)
{
    SceneRecs out;
    out.box = scene_box(s, n, cam);
    out.geo.resize(n);
    out.shade.resize(n);
    out.axis.assign(n, -1);
    for (int i = 0; i < n; ++i) {
        const ptg_sphere &sp = s[i];
        const double R = sp.radius;
        GeoRec g;
        if (is_huge(sp, cam)) {
            double P[3], N[3];
            out.axis[i] = choose_anchor(sp, cam, out.box, P, N);
            g.g0 = make_float4((float)P[0], (float)P[1], (float)P[2], (float)R);
            g.g1 = make_float4((float)N[0], (float)N[1], (float)N[2], (float)(2.0 * R));
        } else {
            g.g0 = make_float4((float)sp.position[0], (float)sp.position[1], (float)sp.position[2],
                               (float)(-(R * R)));
            g.g1 = make_float4(0.0f, 0.0f, 0.0f, (float)(-(R * R)));
        }
        out.geo[i] = g;
        ShadeRec r;
        float cx = (float)sp.color[0], cy = (float)sp.color[1], cz = (float)sp.color[2];
        float p = cx;
        if (p < cy) p = cy;
        if (p < cz) p = cz;
        float rx = 0.0f, ry = 0.0f, rz = 0.0f;
        if (p > 0.0f) {
            float inv = 1.0f / p;
            rx = cx * inv;
            ry = cy * inv;
            rz = cz * inv;
        }
        int32_t mat = sp.material;
        float matf;
        std::memcpy(&matf, &mat, 4);
        // Russian roulette as an integer compare (main.cpp:130-131, u < p):
        // u = m 2^-24 exactly (m the draw's 24-bit integer), so u < p <=> m <
        // p 2^24 <=> m < ceil(p 2^24) -- the same decisions as the oracle's
        // float compare, without the draw's convert and scale
        uint32_t p24 = !(p > 0.0f) ? 0u : (p >= 1.0f ? (1u << 24) : (uint32_t)std::ceil((double)p * 16777216.0));
        float p24f;
        std::memcpy(&p24f, &p24, 4);
        r.s0 = make_float4((float)sp.position[0], (float)sp.position[1], (float)sp.position[2], p24f);
        r.s1 = make_float4((float)sp.emission[0], (float)sp.emission[1], (float)sp.emission[2], matf);
        r.s2 = make_float4(cx, cy, cz, (float)(1.0 / R));
        r.s3 = make_float4(rx, ry, rz, (float)(1.0 / R));
        out.shade[i] = r;
    }
    return out;
}

// A wall may take part in wall pairs / box mode only if no ray origin can lie
// genuinely inside it, beyond its tangent plane, where the "test only the
// wall the ray moves toward" rule would drop a hit of the wall from inside:
// the wall is not dielectric (no path is transmitted into it) and the camera
// is on the room side by more than the margin.  Other spheres need no check:
// a sphere sunk into the wall has its sunk part inside the wall, which a ray
// from the room reaches only through the wall's surface -- the wall is hit
// there first (tests/test_scene_file.py: a glass sphere sunk into a wall,
// pairs on vs every sphere tested, same image).  The oracle's wall_clear_B
// makes the same choice.
inline bool wall_clear(const ptg_sphere *s, int i, int k, bool plus_side, const ptg_camera *cam, const SceneBox &box)
{
    if (s[i].material == PTG_DIELECTRIC)
        return false;
    const double margin = 1e-4 * std::max(1.0, box.diag);
    const double a = plus_side ? s[i].position[k] - s[i].radius : s[i].position[k] + s[i].radius;
    return plus_side ? cam->position[k] < a - margin : cam->position[k] > a + margin;
}

// Wall pairs (DESIGN.md "wall pairs"): on each axis k, the first (scene
// index order) axis-anchored huge sphere whose centre lies on the + side of
// its anchor (anchor normal -e_k) and the first one on the - side.  Their
// tangent planes at the anchors, x_k = a_plus and x_k = a_minus, bound the
// room: a ray from an origin with a_minus <= o_k <= a_plus can hit the + wall
// only if d_k > 0 and the - wall only if d_k < 0 (each sphere lies entirely
// beyond its tangent plane).  The bounds widen by a margin of 1e-4 max(1, box
// diagonal) so that rays leaving a wall (origin rounded a hair past its
// plane) keep the rule; pair_lo/hi are those bounds rounded to float.  The
// oracle's prep_B forms the same pairs (pt_oracle.c).  plus[k] / minus[k] =
// scene index or -1.
inline void pair_walls(const ptg_sphere *s, int n, const ptg_camera *cam, const SceneRecs &sc, int plus[3],
                       int minus[3], float lo[3], float hi[3])
{
    const double margin = 1e-4 * std::max(1.0, sc.box.diag);
    for (int k = 0; k < 3; ++k) {
        plus[k] = minus[k] = -1;
        for (int i = 0; i < n; ++i) {
            if (sc.axis[i] != k)
                continue;
            const float nk = (&sc.geo[i].g1.x)[k];  // anchor normal component: exactly +-1
            if (nk < 0.0f && plus[k] < 0)
                plus[k] = i;
            if (nk > 0.0f && minus[k] < 0)
                minus[k] = i;
        }
        if (plus[k] < 0 || minus[k] < 0 || !wall_clear(s, plus[k], k, true, cam, sc.box) ||
            !wall_clear(s, minus[k], k, false, cam, sc.box)) {
            plus[k] = minus[k] = -1;
            lo[k] = hi[k] = 0.0f;
            continue;
        }
        const double a_plus = s[plus[k]].position[k] - s[plus[k]].radius;
        const double a_minus = s[minus[k]].position[k] + s[minus[k]].radius;
        lo[k] = (float)(a_minus - margin);
        hi[k] = (float)(a_plus + margin);
    }
}

// A sphere no ray can start inside (KArgs::box_walls_out).  A camera ray starts
// outside every sphere whose centre is farther from the camera than its
// radius plus the lens offset (< 2 lens radii: camera_ray's rd * (s + t));
// a ray reaches a surface point
// only from outside every opaque sphere it has not hit before, and a diffuse
// or mirror bounce leaves outward -- so, by induction, only dielectric
// spheres are ever entered (up to the fp32 rounding of a hit point next to a
// contact between two spheres, where the outside-only root lets the ray
// leave, as in exact arithmetic).
inline bool outside_only(const ptg_sphere &s, const ptg_camera *cam)
{
    double d2 = 0.0, p2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double t = s.position[c] - cam->position[c];
        d2 += t * t;
        p2 += cam->position[c] * cam->position[c];
    }
    // margins: the lens bound's, the fp32 rounding of a camera origin, the
    // double rounding of d2
    const double reach = s.radius + 2.0001 * cam->lens_radius + 1e-6 * (1.0 + std::sqrt(p2)) + 1e-9 * s.radius;
    return s.material != PTG_DIELECTRIC && d2 > reach * reach;
}

// KArgs::room_nmr.  The kernel's up = fl(plane_plus - o_k) >= -m implies
// plane_plus - o_k >= -m (1 + 2^-23) (a rounding of at most half an ulp of a
// difference near -m; a larger difference passes or fails with its sign), so
// with m = gap (1 - 2^-10) the origin lies below plane_plus + gap =
// pair_hi; the same for um and pair_lo.  Open sides (planes at +-inf, up or
// um = +inf) bound nothing, as their +-kFarPlane bounds (unreachable) did.
inline float room_neg_margin(const KArgs &A)
{
    double gap = HUGE_VAL;
    for (int k = 0; k < 3; ++k) {
        if (A.plane_plus[k] < HUGE_VALF)
            gap = std::min(gap, (double)A.pair_hi[k] - (double)A.plane_plus[k]);
        if (A.plane_minus[k] > -HUGE_VALF)
            gap = std::min(gap, (double)A.plane_minus[k] - (double)A.pair_lo[k]);
    }
    if (!(gap > 0.0) || gap == HUGE_VAL)
        return HUGE_VALF;  // no lane counts as inside: every wave takes the exact per-axis checks
    const float m = (float)(gap * (1.0 - 0x1p-10));
    return -std::nextafter(m, 0.0f);
}

// Box mode (scene_scan; DESIGN.md "box mode"): on when every axis-anchored
// wall is either one of its axis's pair or the only wall of its axis, at
// least one axis has a pair, and there is no other huge sphere.  Fills the
// per-axis records (scan positions in `order`) and tangent planes (the
// records' anchor coordinate), and extends the pair bounds to single walls
// (margin as pair_walls) and open sides (+-kFarPlane).  The oracle's prep_B
// makes the same choice.
inline void box_mode_of(const ptg_sphere *s, int n, const ptg_camera *cam, const SceneRecs &sc,
                        const std::vector<int> &order, KArgs &A)
{
    A.box_mode = 0;
    A.box_walls_out = 0;
    int cnt[3] = {0, 0, 0}, general = 0;
    for (int i = 0; i < n; ++i) {
        if (!is_huge(s[i], cam))
            continue;
        if (sc.axis[i] < 0)
            ++general;
        else
            ++cnt[sc.axis[i]];
    }
    bool ok = general == 0 && (A.pairs[0] || A.pairs[1] || A.pairs[2]);
    for (int k = 0; k < 3; ++k)
        ok = ok && (A.pairs[k] ? cnt[k] == 2 : cnt[k] <= 1);
    for (int i = 0; i < n && ok; ++i)  // single walls too (the pairs' members are clear)
        if (is_huge(s[i], cam) && sc.axis[i] >= 0)
            ok = wall_clear(s, i, sc.axis[i], (&sc.geo[i].g1.x)[sc.axis[i]] < 0.0f, cam, sc.box);
    if (!ok)
        return;
    const double margin = 1e-4 * std::max(1.0, sc.box.diag);
    for (int k = 0; k < 3; ++k) {
        A.rec_plus[k] = A.rec_minus[k] = -1;
        A.plane_plus[k] = HUGE_VALF;  // missing wall: never the nearest plane, never needed
        A.plane_minus[k] = -HUGE_VALF;
        const int begin = k == 0 ? 0 : A.end_ax[k - 1];
        for (int j = begin; j < A.end_ax[k]; ++j) {
            const int i = order[j];
            const float nk = (&sc.geo[i].g1.x)[k];  // anchor normal component: exactly +-1
            const float plane = (&sc.geo[i].g0.x)[k];  // the anchor point's coordinate
            if (nk < 0.0f) {  // centre on the + side
                A.rec_plus[k] = j * (int)sizeof(LinRec);
                A.plane_plus[k] = plane;
                if (!A.pairs[k])
                    A.pair_hi[k] = (float)(s[i].position[k] - s[i].radius + margin);
            } else {
                A.rec_minus[k] = j * (int)sizeof(LinRec);
                A.plane_minus[k] = plane;
                if (!A.pairs[k])
                    A.pair_lo[k] = (float)(s[i].position[k] + s[i].radius - margin);
            }
        }
        if (A.rec_plus[k] < 0)
            A.pair_hi[k] = kFarPlane;
        if (A.rec_minus[k] < 0)
            A.pair_lo[k] = -kFarPlane;
    }
    A.box_mode = 1;
    A.box_walls_out = 1;
    for (int i = 0; i < n; ++i)
        if (is_huge(s[i], cam) && sc.axis[i] >= 0 && !outside_only(s[i], cam))
            A.box_walls_out = 0;
}

// Linear scenes: scan order (scene_scan) -- huge spheres anchored on x, y, z
// (each axis group led by its wall pair, + wall first), then the other huge
// spheres, then the small ones, each group otherwise in scene index order.
// Writes the scan layout into A: end_ax / end_big (group ends), pairs and
// pair_lo/hi, and box mode's fields (box_mode_of).
inline std::vector<int> scan_order_of(const ptg_sphere *s, int n, const ptg_camera *cam, const SceneRecs &sc, KArgs &A)
{
    std::vector<int> order;
    int plus[3], minus[3];
    pair_walls(s, n, cam, sc, plus, minus, A.pair_lo, A.pair_hi);
    for (int k = 0; k < 3; ++k) {
        A.pairs[k] = plus[k] >= 0 ? 1 : 0;
        if (A.pairs[k]) {
            order.push_back(plus[k]);
            order.push_back(minus[k]);
        }
        for (int i = 0; i < n; ++i)
            if (sc.axis[i] == k && i != plus[k] && i != minus[k])
                order.push_back(i);
        A.end_ax[k] = (int)order.size();
    }
    box_mode_of(s, n, cam, sc, order, A);
    for (int i = 0; i < n; ++i)
        if (is_huge(s[i], cam) && sc.axis[i] < 0)
            order.push_back(i);
    A.end_big = (int)order.size();
    for (int i = 0; i < n; ++i)
        if (!is_huge(s[i], cam))
            order.push_back(i);
    return order;
}

// Records in scan order.  Axis-anchored records carry the signs in their
// constants: g0.w = s R, g1.w = s 2R (the kernel reads e_k and d_k).
inline void prepare_scan_order(const ptg_sphere *s, int n, const ptg_camera *cam, const SceneRecs &sc,
                               std::vector<GeoRec> &lgeo, std::vector<ShadeRec> &lshade, KArgs &A)
{
    lgeo.clear();
    lshade.clear();
    for (int i : scan_order_of(s, n, cam, sc, A)) {
        GeoRec g = sc.geo[i];
        if (sc.axis[i] >= 0) {
            const float sgn = (&g.g1.x)[sc.axis[i]];  // +-1 exactly
            g.g0.w = sgn * g.g0.w;
            g.g1.w = sgn * g.g1.w;
        }
        lgeo.push_back(g);
        lshade.push_back(sc.shade[i]);
    }
}

// Linear scenes (n <= kLinearMax): what the kernel stages in LDS -- the n
// records in scan order, interleaved | the no-hit sentinel | box mode's wall
// offset table | its wall geometry table (2 records' room).  Writes the scan
// layout into A (scan_order_of).
inline std::vector<LinRec> prepare_linear_upload(const ptg_sphere *s, int n, const ptg_camera *cam,
                                                 const SceneRecs &sc, KArgs &A)
{
    std::vector<GeoRec> lgeo;
    std::vector<ShadeRec> lshade;
    prepare_scan_order(s, n, cam, sc, lgeo, lshade, A);
    std::vector<LinRec> lin(n + 2 + 2);  // + the box-mode wall table(s) (scene_scan)
    std::memset(lin.data(), 0, lin.size() * sizeof(LinRec));
    for (int i = 0; i < n; ++i)
        lin[i] = LinRec{lgeo[i], lshade[i]};
    int32_t walls[6];
    for (int k = 0; k < 3; ++k) {
        walls[2 * k] = A.rec_plus[k];
        walls[2 * k + 1] = A.rec_minus[k];
    }
    std::memcpy(&lin[n + 1], walls, sizeof(walls));
    // entry 2 k + side: the wall's geometry, g1.x = its record's byte
    // offset; a missing wall: NaN geometry (its test never wins), offset 0
    GeoRec wg[6];
    for (int e = 0; e < 6; ++e) {
        const float qnan = __builtin_nanf("");
        const int off = walls[e];
        if (A.box_mode && off >= 0 && off / (int)sizeof(LinRec) < n) {
            wg[e] = lgeo[off / (int)sizeof(LinRec)];
            // the record's byte offset from the sentinel (scene_scan's
            // winner bi)
            const int32_t tag = (off / (int)sizeof(LinRec) - n) * (int)sizeof(LinRec);
            std::memcpy(&wg[e].g1.x, &tag, 4);
        } else {
            wg[e].g0 = make_float4(qnan, qnan, qnan, qnan);
            wg[e].g1 = make_float4(0.0f, qnan, qnan, qnan);
        }
    }
    static_assert(sizeof(wg) <= 2 * sizeof(LinRec), "wall geometry table size");
    std::memcpy(&lin[n + 2], wg, sizeof(wg));
    return lin;
}

// Light sampling (PTG_FLAG_LIGHT_SAMPLING): the scene indices of the spheres
// with an emission component > 0 that are not huge, ascending.  Huge
// emitters (and the sky) stay BRDF-sampled only.
inline std::vector<int> light_list_of(const ptg_sphere *s, int n, const ptg_camera *cam)
{
    std::vector<int> ids;
    for (int i = 0; i < n; ++i)
        if ((s[i].emission[0] > 0.0 || s[i].emission[1] > 0.0 || s[i].emission[2] > 0.0) && !is_huge(s[i], cam))
            ids.push_back(i);
    return ids;
}

// Their device records.  id_of[i] = what the scan reports for scene index i
// (linear scenes: its scan position; BVH scenes: i itself).
inline std::vector<LightRec> light_records(const ptg_sphere *s, const std::vector<int> &ids,
                                           const std::vector<int> &id_of)
{
    std::vector<LightRec> recs;
    for (int i : ids) {
        const int32_t id = id_of[i];
        float idf;
        std::memcpy(&idf, &id, 4);
        LightRec r;
        r.c = make_float4((float)s[i].position[0], (float)s[i].position[1], (float)s[i].position[2],
                          (float)(s[i].radius * s[i].radius));
        r.e = make_float4((float)s[i].emission[0], (float)s[i].emission[1], (float)s[i].emission[2], idf);
        recs.push_back(r);
    }
    return recs;
}

// The camera fields of KArgs (camera.cpp:32-38): pos, base = llc - pos, X, Y, lens radius.
inline void prepare_camera(const ptg_camera *cam, KArgs &A)
{
    A.pos_x = (float)cam->position[0];
    A.pos_y = (float)cam->position[1];
    A.pos_z = (float)cam->position[2];
    A.base_x = (float)(cam->lower_left_corner[0] - cam->position[0]);
    A.base_y = (float)(cam->lower_left_corner[1] - cam->position[1]);
    A.base_z = (float)(cam->lower_left_corner[2] - cam->position[2]);
    A.X_x = (float)cam->cam_x_axis[0];
    A.X_y = (float)cam->cam_x_axis[1];
    A.X_z = (float)cam->cam_x_axis[2];
    A.Y_x = (float)cam->cam_y_axis[0];
    A.Y_y = (float)cam->cam_y_axis[1];
    A.Y_z = (float)cam->cam_y_axis[2];
    A.lens = (float)cam->lens_radius;
}

// BVH scenes (n > kLinearMax): one allocation -- leaf records | leaf ids |
// huge spheres | their ids | the 8 interleaved wide layouts | their
// continuations -- with the byte offsets of its parts and the KArgs fields
// that describe the tree.
struct BvhUpload {
    std::vector<unsigned char> blob;
    size_t off_geo, off_id, off_bgeo, off_bid, off_q, off_cont;
    float q_lo[3], q_scale[3];
    int n_nodes, n_big;
};

inline BvhUpload prepare_bvh_upload(const ptg_sphere *spheres, int n, const ptg_camera *cam,
                                    const std::vector<GeoRec> &geo)
{
    BvhUpload u;
    std::vector<char> huge(n);
    for (int i = 0; i < n; ++i)
        huge[i] = is_huge(spheres[i], cam);
    BvhBuild b = build_bvh(spheres, n, huge);
    const size_t n_leaf = b.order.size(), n_big = b.big.size();
    u.off_geo = 0;
    u.off_id = u.off_geo + n_leaf * sizeof(float4);
    u.off_bgeo = (u.off_id + n_leaf * sizeof(int) + 15) & ~size_t(15);
    u.off_bid = u.off_bgeo + n_big * sizeof(GeoRec);
    u.off_q = (u.off_bid + n_big * sizeof(int) + 15) & ~size_t(15);
    const size_t n_recs = wide_bvh(b, 0, 0).size();  // records per layout
    // near-plane-first boxes: one layout per octant
    const size_t n_layouts = 8;
    const size_t stride = n_recs;  // (interleaved: 8 x n_recs records in all, no layout stride)
    u.off_cont = u.off_q + n_layouts * stride * sizeof(BvhNodeQ);
    const size_t total = u.off_cont + n_layouts * stride / kWide * sizeof(int32_t) + 16;
    u.blob.assign(total, 0);
    unsigned char *blob = u.blob.data();
    // the 8 layouts interleaved node by node: node j of layout k at
    // interleaved node 8 j + k, so the copies of one node share a 512-B
    // block instead of aliasing a power of two of records apart
    auto ilv = [](int32_t local, int k) { return ((local >> 2) * 8 + k) * 4 + (local & 3); };
    for (int k = 0; k < 8; ++k) {
        std::vector<BvhNodeQ> qk = wide_bvh(b, k, 0);
        const std::vector<int32_t> ck = wide_conts(qk, 0);
        for (size_t r = 0; r < qk.size(); ++r) {
            BvhNodeQ &z = qk[r];
            if (z.word >= 0)
                z.word = ilv(z.word, k);
            std::memcpy(blob + u.off_q + (size_t)ilv((int32_t)r, k) * sizeof(BvhNodeQ), &z, sizeof(z));
        }
        for (size_t j = 0; j < ck.size(); ++j) {
            const int32_t c = ck[j] >= 0 ? ilv(ck[j], k) : ck[j];
            std::memcpy(blob + u.off_cont + (j * 8 + (size_t)k) * sizeof(int32_t), &c, sizeof(c));
        }
    }
    const WideGrid wg(b.nodes.empty() ? BvhNodeHost{} : b.nodes[0]);
    for (int c = 0; c < 3; ++c) {
        u.q_lo[c] = wg.centre[c];
        u.q_scale[c] = wg.scale[c];
    }
    for (size_t i = 0; i < n_leaf; ++i) {
        const ptg_sphere &sp = spheres[b.order[i]];  // leaf record {C, -R^2}, as the GeoRec of a small sphere
        const float4 rec = make_float4((float)sp.position[0], (float)sp.position[1], (float)sp.position[2],
                                       (float)(-(sp.radius * sp.radius)));
        std::memcpy(blob + u.off_geo + i * sizeof(float4), &rec, sizeof(float4));
        std::memcpy(blob + u.off_id + i * sizeof(int), &b.order[i], sizeof(int));
    }
    for (size_t i = 0; i < n_big; ++i) {
        std::memcpy(blob + u.off_bgeo + i * sizeof(GeoRec), &geo[b.big[i]], sizeof(GeoRec));
        std::memcpy(blob + u.off_bid + i * sizeof(int), &b.big[i], sizeof(int));
    }
    u.n_nodes = (int)n_recs;
    u.n_big = (int)n_big;
    return u;
}

}  // namespace
