// render_unit.hpp -- the render-loop megakernel: the camera ray (Lane, CamC,
// cam_of, camera_ray), the exact per-path quantisation, render_unit and the
// nine pool kernels that instantiate it (render / moments / gather, plain,
// _ls and _strat) with their waves-per-SIMD constants.  Included by
// ptg_render.hip inside its unnamed namespace, after shade.hpp; needs the
// scans' resumable pieces, shade, KArgs (kernel_args.hpp), sample_state and
// draw (pt_device.hpp), the Sobol' pairs (sobol_pairs.hpp) and the tunables
// and statistics macros of render_config.hpp.  Owns no switch.
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
#pragma once

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
