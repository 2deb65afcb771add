// probe_kernels.hpp -- the untimed kernels: the parity probe (trace_path,
// trace_kernel, trace_strat), the denoiser's first-hit features
// (features_kernel, and follow_features.hpp's kernel, included here between
// its neighbours), math_probe_kernel, sampler_pairs_kernel, unshard_kernel
// and tonemap_kernel.  Included by ptg_render.hip inside its unnamed
// namespace, last of the device headers; needs segment (shade.hpp), both
// whole-ray scans, camera_ray, cam_of and out_row_of (render_unit.hpp) and
// the Sobol' pairs (sobol_pairs.hpp).  Owns no switch.
#pragma once

constexpr int kTraceBlock = 256;  // parity probe kernel

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
