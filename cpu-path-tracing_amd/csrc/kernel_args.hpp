// kernel_args.hpp -- what the host hands the render kernels: the KArgs
// kernel-argument struct and the constants both sides size things by.
// Filled by scene_prep.hpp (scene fields) and launch_plan.hpp (frame and unit
// levels), read by the kernels of ptg_render.hip (render_unit.hpp and the
// device headers around it).  The field order and types of KArgs are the
// kernels' kernarg layout: do not reorder.
#pragma once

#include <cmath>

#include "../../include/ptgpu.h"
#include "pt_device.hpp"

namespace {

using namespace ptg;

#ifndef PTG_BLOCK
#define PTG_BLOCK 256  // linear-scene render kernel workgroup size
#endif
constexpr int kBlock = PTG_BLOCK;
constexpr int kMaxLevels = 4;     // unit levels: head + up to 3 split-tail levels
// samples per sub-pixel in one work unit, at most: a unit's paths are indexed
// it < 64 * chunk <= 2^22, where render_kernel's float-reciprocal divmod_nv is
// exact (fill_launch caps every level's chunk)
constexpr int kMaxChunk = 1 << 16;
// nearest-hit rule and scan: <= kLinearMax spheres -> linear scan from LDS with
// fraction comparisons; more -> BVH with the reference's per-candidate
// division rule (DESIGN.md "scene scan"); the oracle switches at the same n
#ifndef PTG_LINEAR_MAX
#define PTG_LINEAR_MAX 64
#endif
constexpr int kLinearMax = PTG_LINEAR_MAX;
#ifndef PTG_BVH_BLOCK
#define PTG_BVH_BLOCK 64  // BVH render kernel: one wave per workgroup, so a wave slot frees as soon as its unit ends
                          // (units of the 10,000-sphere scene differ widely in length: 64 beats 256 by 10 %, 128 by 6 %)
#endif
constexpr float kFarPlane = 1e30f;  // box mode: the room bound of an open side
constexpr double kBigRadius = 1000.0;
// A sphere takes the anchored form ("huge", DESIGN.md "huge spheres") when its
// radius is >= 1000 or more than 16 times the camera's distance to its
// surface (+1): locally plane-like for the scene, where c = |o - C|^2 - R^2
// cancels in fp32 (simple_scene's R = 100 ground: RMSE vs fp64 1.5e-3 ->
// 3.3e-4).  The oracle's is_huge_B applies the same rule.
inline bool is_huge(const ptg_sphere &sp, const ptg_camera *cam)
{
    if (sp.radius >= kBigRadius)
        return true;
    double d2 = 0.0;
    for (int c = 0; c < 3; ++c)
        d2 += (cam->position[c] - sp.position[c]) * (cam->position[c] - sp.position[c]);
    return sp.radius > 16.0 * (std::fabs(std::sqrt(d2) - sp.radius) + 1.0);
}

struct KArgs {
    const LinRec *lin;      // linear scenes (<= kLinearMax): n records in scan order + sentinel
    const ShadeRec *shade;  // BVH scenes: shading records in scene index order
    int n;
    // linear scenes: records in SCAN order (prepare_scan_order), grouped by
    // kind: [0, end_ax[0]) huge spheres anchored on the x axis, then y, then z
    // ([end_ax[k-1], end_ax[k])), then general huge spheres up to end_big,
    // then the small spheres up to n
    int end_ax[3];
    int end_big;
    int box_walls_out;  // box mode's walls: no ray starts inside any (outside_only); else the fast mode scans generically
    // wall pairs (pair_walls): axis k's group starts with a pair when
    // pairs[k] = 1 -- its wall on the + side, then its wall on the - side; a
    // lane whose origin lies in [pair_lo[k], pair_hi[k]] tests only the wall
    // its direction moves toward (d_k >= 0: the + wall)
    int pairs[3];
    float pair_lo[3], pair_hi[3];
    // box mode (scan_order_of: every axis-anchored wall belongs to the one
    // pair or is the one single wall of its axis, at least one pair, no
    // other huge sphere): per axis the + and - walls' records (-1: none) and
    // tangent planes (+-inf: none); pair_lo/hi bound the room on every
    // axis (+-kFarPlane where open)
    int box_mode;
    int rec_plus[3], rec_minus[3];  // byte offsets of the records
    float plane_plus[3], plane_minus[3];
    // box mode: -m, m > 0 the smallest gap between a wall's tangent plane and
    // its room bound (pair_lo/hi) less a rounding margin: an origin whose
    // plane distances up/um (scene_scan) are all >= -m lies inside the room
    // bounds (room_neg_margin); +inf where there is no such gap
    float room_nmr;
    // scenes with more than kLinearMax spheres: BVH (bvh_build.hpp)
    // the 4-wide tree (bvh_build.hpp wide_bvh): 8 near-plane-first layouts,
    // one per ray-direction octant, interleaved node by node (node j of
    // layout k at node 8 j + k), 4 records of 16 B per node
    const uint4 *bvh_qnodes;
    float q_lo[3], q_scale[3];  // box grid: plane = q_lo + value * q_scale (binary16 values)
    const float4 *bvh_sph;    // leaf-ordered spheres {C, -R^2} (BVH leaves hold only non-huge spheres)
    const int *bvh_id;        // leaf-ordered scene indices
    const GeoRec *big_geo;    // huge spheres, tested linearly
    const int *big_id;
    int n_nodes, n_big;
    const int *bvh_cont;  // per wide node (first record / 4) its continuation (bvh_build.hpp wide_conts)
    const float2 *trig;  // {cos, sin}(2 pi k / 128), staged in LDS (sincos2pi_tab)
    // camera (camera.cpp:32-38): pos, base = llc - pos, X, Y, lens_radius
    float pos_x, pos_y, pos_z;
    float base_x, base_y, base_z;
    float X_x, X_y, X_z;
    float Y_x, Y_y, Y_z;
    float lens;
    // image / sampling
    int W, H, samps, nsub, lanes_per_pixel, pixels_per_wave, waves_per_row;
    int slab_rows, band_rows, shard_rank, shard_count;
    float invW, invH, inv_samps, sub_len, inv_sub2;
    unsigned long long seed;
    int chunk, n_groups, single_chunk;
    // unit levels (fill_launch): level l covers pixel groups [lvl_group[l],
    // lvl_group[l + 1]) in chunks of lvl_chunk[l] samples, chunk-major, as
    // units [lvl_unit[l], lvl_unit[l + 1]); level 0 is the head, levels >= 1
    // the split tail (accumulated, then resolve_kernel from slab row
    // resolve_row0).  lvl_group[n_levels] = n_groups.
    int n_levels;
    int lvl_group[kMaxLevels + 1], lvl_chunk[kMaxLevels];
    // cooperative level (linear kernel's split tail with as many chunks as a
    // workgroup has waves): the waves of one workgroup take the chunks of one
    // pixel group, the last wave to finish adds the others' LDS sums and
    // resolves -- no HBM accumulator (lvl_unit[l] is a multiple of the
    // waves per workgroup)
    int lvl_coop[kMaxLevels];
    // pixel-split level (the BVH kernel's split tail): each pixel group in
    // lvl_psplit[l] units, unit k taking the group's pixels k, k + ps, k + 2ps,
    // ... (interleaved, so the units of a group cost about the same) with
    // every sample (lvl_inwave: resolved in the wave, nothing accumulated in
    // HBM); 1 elsewhere
    int lvl_psplit[kMaxLevels];
    int lvl_inwave[kMaxLevels];  // the level's units hold every sample of their pixels
    int needs_resolve;  // some level accumulates in HBM: resolve_kernel from resolve_row0
    long long lvl_unit[kMaxLevels + 1];
    int resolve_row0;
    int sample_begin, sample_end;  // samples [begin, end) of every sub-pixel in this launch
    int keep_acc;                  // resolve without re-zeroing (progressive previews)
    int count_tests;               // PTG_FLAG_COUNT_TESTS: segments[1..2] += sphere tests, box tests
    int count_nonfinite;           // PTG_FLAG_COUNT_NONFINITE: segments[3] += paths quant() would clip
    int exact_math;                // PTG_FLAG_EXACT_MATH: the kernels' exact arithmetic (pt_device.hpp Math)
    long long n_units;
    float *out;
    unsigned long long *acc;  // slab_rows * W * lanes_per_pixel * 3 exact sums
    unsigned long long *segments;
    // PTG_FLAG_LIGHT_SAMPLING (appended: the fields above keep their offsets):
    // the scene's light list; n_lights is 0 in a launch without the flag
    // (plan_frame), which then runs the plain kernels
    const LightRec *lights;
    int n_lights;
    // PTG_FLAG_STRATIFIED (in the struct's tail padding: no offset moves, the
    // size stays): the launch runs the *_strat kernels
    int stratified;
};

}  // namespace
