// launch_plan.hpp -- the launch plan: how a frame (or a shard, or a
// progressive pass) is cut into work units, one wave each.  fill_launch turns
// ptg_params into the frame and unit-level fields of KArgs and the grid size;
// the kernels index that table without checks (render_kernel's "unit ->
// level"), so its invariants are tested on the CPU (tests/launch_plan_check.cpp).
// Plain C++, no HIP API calls: the plan depends on the sphere count and the
// device's wave slots only.
#pragma once

#include <cstdint>
#include <string>

#include "kernel_args.hpp"
#include "ptg_error.hpp"

// ---- tunables (measured on the MI355X; A/B records under profiles/) --------
#ifndef PTG_UNIT_ROUNDS
#define PTG_UNIT_ROUNDS 2  // linear scenes below the split-tail size: work units for this many rounds of wave slots (2 beats 4 by 5 %, 12 by 12 % on C1)
#endif
#ifndef PTG_BVH_UNIT_MULT
#define PTG_BVH_UNIT_MULT 2  // BVH scenes below the split-tail threshold: this many times more work units (8-way C5 shards: 2 beats 1 and 4 by 2-5 %)
#endif
#ifndef PTG_TAIL_CHUNKS
#define PTG_TAIL_CHUNKS 8  // split-tail units per pixel group of the last rows (1: off)
#endif
#ifndef PTG_TAIL_LEVELS
// split-tail levels, each with twice the chunks of the one before (<= 3);
// measured: 2 or 3 levels (chunks 4/8/16) within 1 % of 1 level on the bench
// frame, its 2-8-way shards and box 1024x768
#define PTG_TAIL_LEVELS 1
#endif
#ifndef PTG_TAIL_CHUNKS_MANY
// ... with at least 5 rounds of wave slots (measured: box 1024x768x256 spp
// 2 % faster with 4 than with 8, the 1920x1080 frame the same; 2-8-way shards
// of that frame, 2-4 rounds, keep 8)
#define PTG_TAIL_CHUNKS_MANY 4
#endif
#ifndef PTG_BVH_TAIL_CHUNKS_MANY
// ... and for BVH scenes, whose pixel-split tail units carry every sample of
// their pixels (no HBM accumulation either way): 8 units of 2 pixels per
// group (C5 -0.85 % against 4, A/B 244.4-244.7 vs 246.3-247.1 ms; the box
// scenes keep 4, the cooperative LDS-reduced level)
#define PTG_BVH_TAIL_CHUNKS_MANY 8
#endif
#ifndef PTG_LIN_TAIL_HALF_ROUNDS
#define PTG_LIN_TAIL_HALF_ROUNDS 2  // linear scenes: split-tail rows, in half rounds of the device's wave slots
#endif
#ifndef PTG_BVH_TAIL_HALF_ROUNDS
#define PTG_BVH_TAIL_HALF_ROUNDS 2  // BVH scenes: split-tail rows, in half rounds of the device's wave slots
#endif
#ifndef PTG_TAIL_MIN_HALF_ROUNDS
// linear scenes: split tail from 1.5 rounds of wave slots on (measured with
// tools/shard_sim.py: 2/4/8-way shards of the bench frame 1.6/1.8/1.4 %
// faster than with their samples split into ~96k units)
#define PTG_TAIL_MIN_HALF_ROUNDS 3
#endif
#ifndef PTG_BVH_TAIL_MIN_HALF_ROUNDS
#define PTG_BVH_TAIL_MIN_HALF_ROUNDS 6  // BVH scenes: split tail from 3 rounds of wave slots on
#endif
#ifndef PTG_BVH_HEAD_CHUNK
#define PTG_BVH_HEAD_CHUNK 128  // BVH scenes below the split-tail threshold: head rows in chunks of this many samples (0: off; C5 8-way shard 50.4 -> 48.1 ms; 64/96 within 0.5 %, whole pixels +45 %)
#endif
#ifndef PTG_BVH_HEAD_TAIL_HALF_ROUNDS
#define PTG_BVH_HEAD_TAIL_HALF_ROUNDS 1  // ... and the last rows, this many half rounds of wave slots, in the auto chunk (1 beats 2 by 2.5 %, 3 by 5 %)
#endif
#ifndef PTG_BVH_TAIL_CHUNK
#define PTG_BVH_TAIL_CHUNK 0  // ... in chunks of this many samples (0: the auto chunk, 20 at C5 8-way; 10: +0.8 %, 32: +5 %)
#endif

namespace {

inline int check_params(const ptg_params *p)
{
    if (!p)
        return fail(PTG_ERR_INVALID_ARGUMENT, "params is NULL");
    if (p->width <= 0 || p->height <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (p->samples < 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "samples must be >= 0");
    if (p->num_subpixels < 1 || p->num_subpixels > 8)
        return fail(PTG_ERR_UNSUPPORTED, "num_subpixels must be in [1, 8]");
    if (p->band_rows < 1 || p->shard_count < 1 || p->shard_rank < 0 || p->shard_rank >= p->shard_count)
        return fail(PTG_ERR_INVALID_ARGUMENT, "invalid shard (band_rows >= 1, 0 <= rank < count)");
    if ((int64_t)p->width * p->height > (int64_t)1 << 28 || p->width >= (1 << 20))
        return fail(PTG_ERR_UNSUPPORTED, "image too large");
    return PTG_OK;
}

// Rows of one shard's slab: its share of the image's bands, whole bands.
inline int shard_slab_rows(int height, int band_rows, int shard_count)
{
    const int bands = (height + band_rows - 1) / band_rows;
    return ((bands + shard_count - 1) / shard_count) * band_rows;
}

// Frame and shard geometry, sampling constants and flags.
inline void plan_frame(const ptg_params *p, int s_begin, int s_end, KArgs &A)
{
    A.W = p->width;
    A.H = p->height;
    A.samps = p->samples;
    A.nsub = p->num_subpixels;
    A.lanes_per_pixel = p->num_subpixels * p->num_subpixels;
    A.pixels_per_wave = 64 / A.lanes_per_pixel;
    A.waves_per_row = (p->width + A.pixels_per_wave - 1) / A.pixels_per_wave;
    A.slab_rows = shard_slab_rows(p->height, p->band_rows, p->shard_count);
    A.band_rows = p->band_rows;
    A.shard_rank = p->shard_rank;
    A.shard_count = p->shard_count;
    A.invW = 1.0f / (float)p->width;
    A.invH = 1.0f / (float)p->height;
    A.inv_samps = p->samples > 0 ? 1.0f / (float)p->samples : 0.0f;
    A.sub_len = 1.0f / (float)p->num_subpixels;
    A.inv_sub2 = 1.0f / (float)(p->num_subpixels * p->num_subpixels);
    A.seed = p->seed;
    A.sample_begin = s_begin;
    A.sample_end = s_end;
    A.keep_acc = 0;
    A.count_tests = (p->flags & PTG_FLAG_COUNT_TESTS) != 0;
    A.count_nonfinite = (p->flags & PTG_FLAG_COUNT_NONFINITE) != 0;
    A.exact_math = (p->flags & PTG_FLAG_EXACT_MATH) != 0;
    if (!A.exact_math && !A.box_walls_out)
        A.box_mode = 0;  // the fast mode's box-mode wall test assumes rays outside the walls
    if (!(p->flags & PTG_FLAG_LIGHT_SAMPLING))
        A.n_lights = 0;  // (the scene's list stays in the context's base)
    A.stratified = (p->flags & PTG_FLAG_STRATIFIED) != 0;
    A.n_groups = A.slab_rows * A.waves_per_row;
}

// Auto chunk: split the samples only as far as needed for ~96k work units
// (about 16 waves per SIMD slot on 256 CUs), which keeps the grid-level tail
// small at any GPU count.  BVH scenes aim at PTG_BVH_UNIT_MULT times more
// units: their cost varies strongly over the image (sky rows vs the sphere
// field).  Linear scenes: PTG_UNIT_ROUNDS rounds of the device's wave slots
// -- C1's 7,500 pixel groups in 6-sample units, 22,500 units: 12 % faster
// than ~96k units of 2 samples, whose per-unit setup weighed.
inline int plan_auto_chunk(bool bvh, int wave_slots, int groups, int nsamp)
{
    const long long target = bvh ? PTG_BVH_UNIT_MULT * 98304 : (long long)PTG_UNIT_ROUNDS * wave_slots;
    long long want = (target + groups - 1) / groups;
    long long nch = want < 1 ? 1 : (want > nsamp ? nsamp : want);
    return nch > 0 ? (int)((nsamp + nch - 1) / nch) : 1;
}

// One level: every pixel group in chunks of `chunk` samples.  `one_shot`: the
// launch covers every sample of the frame and is not an accumulate pass.
inline void plan_single_level(KArgs &A, int chunk, int nsamp, bool one_shot)
{
    A.chunk = chunk;
    const int n_chunks = nsamp > 0 ? (nsamp + chunk - 1) / chunk : 0;
    // in-wave resolve only when one unit holds ALL samples of its pixels
    A.single_chunk = one_shot && n_chunks <= 1;
    A.n_units = (long long)A.n_groups * n_chunks;
    A.n_levels = 1;
    A.lvl_group[0] = 0;
    A.lvl_group[1] = A.n_groups;
    A.lvl_chunk[0] = chunk;
    A.lvl_unit[0] = 0;
    A.lvl_unit[1] = A.n_units;
    for (int l = 0; l < kMaxLevels; ++l) {
        A.lvl_coop[l] = 0;
        A.lvl_psplit[l] = 1;
        A.lvl_inwave[l] = 0;
    }
    A.lvl_inwave[0] = A.single_chunk;
    A.resolve_row0 = 0;
    A.needs_resolve = !A.single_chunk;
}

// Split tail: with whole-pixel units, the grid ends when its slowest last
// units end (a unit is ~1/16 of the frame per wave slot here).  The last
// rows -- about one round of the device's wave slots -- run instead as
// shorter units, accumulated and resolved by resolve_kernel; everything
// before keeps the in-wave resolve.  The tail's rows get shorter units
// towards the end (PTG_TAIL_LEVELS levels, each with twice the chunks of the
// one before), so the last units to start are the shortest.
inline void plan_split_tail(KArgs &A, bool bvh, int wave_slots, int nsamp)
{
    const long long tail_slots = (long long)(bvh ? PTG_BVH_TAIL_HALF_ROUNDS : PTG_LIN_TAIL_HALF_ROUNDS) * wave_slots / 2;
    int tail_rows = (int)((tail_slots + A.waves_per_row - 1) / A.waves_per_row);
    tail_rows = tail_rows < A.slab_rows ? tail_rows : A.slab_rows;
    const bool many = A.n_groups >= 5LL * wave_slots;
    // level row counts: halves of what is left, the last level takes the rest
    int rows_left = tail_rows, row = A.slab_rows - tail_rows;
    A.resolve_row0 = A.slab_rows;  // no accumulating level yet
    A.lvl_group[1] = row * A.waves_per_row;
    A.lvl_unit[1] = A.lvl_group[1];  // head: one unit per group
    int l = 1;
    constexpr int kLinWaves = kBlock / 64;
    for (; l <= PTG_TAIL_LEVELS && rows_left > 0; ++l) {
        const int rows = l == PTG_TAIL_LEVELS ? rows_left : (rows_left + 1) / 2;
        const int tc = (many ? (bvh ? PTG_BVH_TAIL_CHUNKS_MANY : PTG_TAIL_CHUNKS_MANY) : PTG_TAIL_CHUNKS) << (l - 1);
        const int ch = (nsamp + tc - 1) / tc;
        const int nch = (nsamp + ch - 1) / ch;
        // one chunk per wave of a (linear-kernel) workgroup: the level's
        // sums stay in LDS; its first unit starts a workgroup
        const bool coop = !bvh && nch == kLinWaves;
        // BVH kernel (one wave per workgroup, no cooperative level): the
        // pixel group split into as many units of interleaved pixels,
        // each with every sample -- the unit length of nch sample chunks,
        // resolved in the wave (C5: no HBM atomics, no resolve pass)
        const bool psplit = bvh && l == 1 && nch > 1 && A.pixels_per_wave >= nch;
        if (coop)
            A.lvl_unit[l] = (A.lvl_unit[l] + kLinWaves - 1) / kLinWaves * kLinWaves;
        else if (!psplit && A.resolve_row0 == A.slab_rows)
            A.resolve_row0 = row;
        A.lvl_coop[l] = coop ? 1 : 0;
        A.lvl_psplit[l] = psplit ? nch : 1;
        A.lvl_inwave[l] = psplit ? 1 : 0;
        row += rows;
        rows_left -= rows;
        A.lvl_chunk[l] = psplit ? nsamp : ch;
        A.lvl_group[l + 1] = row * A.waves_per_row;
        A.lvl_unit[l + 1] = A.lvl_unit[l] + (long long)(A.lvl_group[l + 1] - A.lvl_group[l]) * nch;
    }
    A.n_levels = l;
    A.n_units = A.lvl_unit[l];
    A.needs_resolve = A.resolve_row0 < A.slab_rows;
    if (!A.needs_resolve)
        A.resolve_row0 = 0;
}

// BVH frames/shards below their split-tail threshold (e.g. 8-way shards of
// C5): the head rows run in longer sample chunks -- fewer per-unit pool
// tails -- and about the last round of wave slots' rows in the auto chunk
// (A.chunk), so the grid still ends on short units.  Every unit accumulates;
// resolve_kernel finishes all rows.
inline void plan_bvh_head_tail(KArgs &A, int wave_slots, int nsamp)
{
    const long long tslots = (long long)PTG_BVH_HEAD_TAIL_HALF_ROUNDS * wave_slots / 2;
    const int tail_rows = (int)((tslots + A.waves_per_row - 1) / A.waves_per_row);
    if (tail_rows >= A.slab_rows)
        return;
    const int hc = PTG_BVH_HEAD_CHUNK < nsamp ? PTG_BVH_HEAD_CHUNK : nsamp;
    const int hn = (nsamp + hc - 1) / hc;
    const int row = A.slab_rows - tail_rows;
    A.lvl_chunk[0] = hc;
    A.lvl_group[1] = row * A.waves_per_row;
    A.lvl_unit[1] = (long long)A.lvl_group[1] * hn;
    const int tc = PTG_BVH_TAIL_CHUNK > 0 ? (PTG_BVH_TAIL_CHUNK < nsamp ? PTG_BVH_TAIL_CHUNK : nsamp) : A.chunk;
    const int tn = (nsamp + tc - 1) / tc;
    A.lvl_chunk[1] = tc;
    A.lvl_group[2] = A.n_groups;
    A.lvl_unit[2] = A.lvl_unit[1] + (long long)(A.n_groups - A.lvl_group[1]) * tn;
    A.n_levels = 2;
    A.n_units = A.lvl_unit[2];
    A.needs_resolve = 1;
}

// Launch geometry for samples [s_begin, s_end) of every sub-pixel.  `base`
// holds the scene and camera fields (ptg_context_create); the plan depends on
// base.n (linear or BVH kernel) and the device's wave slots (CUs x 32).
// work unit = pixel group x chunk of samples.
inline int fill_launch(const KArgs &base, int wave_slots, const ptg_params *p, KArgs &A, int &grid, int s_begin = 0,
                       int s_end = -1, bool accumulate_only = false)
{
    if (s_end < 0)
        s_end = p->samples;
    const int nsamp = s_end - s_begin;
    const bool bvh = base.n > kLinearMax;
    // every sample of the frame in this launch, resolved by it ...
    const bool one_shot = !accumulate_only && s_begin == 0 && s_end == p->samples;
    const bool whole_frame = one_shot && p->chunk_samples <= 0;  // ... with the auto chunk
    A = base;
    plan_frame(p, s_begin, s_end, A);
    // split tail from PTG_TAIL_MIN_HALF_ROUNDS/2 rounds of the device's wave
    // slots on, BVH scenes from PTG_BVH_TAIL_MIN_HALF_ROUNDS/2 (then the head
    // runs whole-pixel units even where ~96k units would split samples, e.g.
    // an 8-GPU shard).  The head's units are whole pixels, so the head needs
    // enough rounds to average out the rows' different costs: at 2 rounds
    // (8-way shards of the bench frame) the split tail gains 1.7-2.1 % on the
    // box scenes but loses 28 % on the 10,000-sphere scene
    // (tools/scene_shard_ab.sh); from 4 rounds on it gains on both.
    const long long tail_min =
        (long long)(bvh ? PTG_BVH_TAIL_MIN_HALF_ROUNDS : PTG_TAIL_MIN_HALF_ROUNDS) * wave_slots / 2;
    const bool split_tail = whole_frame && PTG_TAIL_CHUNKS > 1 && nsamp >= PTG_TAIL_CHUNKS && nsamp <= kMaxChunk &&
                            A.n_groups >= tail_min;
    int chunk = p->chunk_samples;
    if (split_tail)
        chunk = nsamp;  // the head: whole pixels
    else if (chunk <= 0)
        chunk = plan_auto_chunk(bvh, wave_slots, A.n_groups, nsamp);
    if (chunk > nsamp)
        chunk = nsamp > 0 ? nsamp : 1;
    if (chunk > kMaxChunk)  // the kernel's divmod_nv needs 64 * chunk <= 2^22 (the image does not depend on it)
        chunk = kMaxChunk;
    plan_single_level(A, chunk, nsamp, one_shot);
    if (split_tail && A.single_chunk)
        plan_split_tail(A, bvh, wave_slots, nsamp);
#if PTG_BVH_HEAD_CHUNK > 0
    else if (bvh && whole_frame && chunk < PTG_BVH_HEAD_CHUNK && chunk < nsamp)
        plan_bvh_head_tail(A, wave_slots, nsamp);
#endif
    const int waves_per_block = (bvh ? PTG_BVH_BLOCK : kBlock) / 64;
    const long long g = (A.n_units + waves_per_block - 1) / waves_per_block;  // 64-bit before any cast
    grid = 0;
    if (g > 0x7FFFFFFFLL)
        return fail(PTG_ERR_UNSUPPORTED, "too many work units (" + std::to_string(A.n_units) +
                                             "): raise chunk_samples or use 0 (auto)");
    grid = (int)g;
    return PTG_OK;
}

// An adaptive pass (ptg_accumulate_active_device): `units` work units of the
// active list (the caller's bound on them) x chunks of the add_samples new
// samples, chunk-major; unit k of chunk c is wave units * c + k of the grid
// when all `units` are active (the kernel takes the true count from the
// device).  chunk_samples is honoured, else the auto rule applies to the unit
// count; every chunk is within kMaxChunk.
struct ActivePlan {
    int chunk;          // samples per unit
    int n_chunks;       // ceil(add_samples / chunk)
    long long n_units;  // units * n_chunks
    int grid;           // workgroups
};
inline int plan_active(bool bvh, int wave_slots, long long units, int add_samples, int chunk_samples, ActivePlan &P)
{
    P = ActivePlan{1, 0, 0, 0};
    if (units <= 0 || add_samples <= 0)
        return PTG_OK;  // nothing to launch
    int chunk = chunk_samples;
    if (chunk <= 0)
        chunk = plan_auto_chunk(bvh, wave_slots, (int)(units < 0x7FFFFFFFLL ? units : 0x7FFFFFFFLL), add_samples);
    if (chunk > add_samples)
        chunk = add_samples;
    if (chunk > kMaxChunk)
        chunk = kMaxChunk;
    P.chunk = chunk;
    P.n_chunks = (add_samples + chunk - 1) / chunk;
    P.n_units = units * P.n_chunks;  // units <= 2^31, n_chunks <= 2^30: no overflow in 64 bits
    const int waves_per_block = (bvh ? PTG_BVH_BLOCK : kBlock) / 64;
    const long long g = (P.n_units + waves_per_block - 1) / waves_per_block;  // 64-bit before any cast
    if (g > 0x7FFFFFFFLL)
        return fail(PTG_ERR_UNSUPPORTED, "too many work units (" + std::to_string(P.n_units) +
                                             "): raise chunk_samples or use 0 (auto)");
    P.grid = (int)g;
    return PTG_OK;
}

}  // namespace
