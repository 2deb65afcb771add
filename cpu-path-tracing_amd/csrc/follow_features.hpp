// follow_features.hpp -- ptg_features_follow_device's kernel (include/ptgpu.h
// "denoising"): the feature rays of features_kernel followed through mirrors
// and glass to the first diffuse surface.  Included by ptg_render.hip inside
// its unnamed namespace, after the scans and the helpers it uses (KArgs,
// cam_of, out_row_of, scene_scan, scene_scan_bvh, Math<true>); no code of its
// own outside this kernel, no LDS, no switch.
//
// No draw: a mirror's fuzz draw is multiplied by 0 (main.cpp:65) and the
// refraction direction is a function of d and the normal (main.cpp:72-96).
// The Fresnel draw that sends part of a dielectric's paths into a reflection
// is not taken: the ray refracts wherever it can.
#pragma once

// The next direction of a ray that hit a specular (glass false) or dielectric
// sphere, in shade<true>'s arithmetic: on the outward normal, nn the facing
// one.  Mirror: main.cpp:60-67 on `on`, d not normalised.  Dielectric:
// main.cpp:72-96 with the exact branch's roundings -- v1 = d rsqrt(d.d),
// cth = min(1, -v1.nn) as a select, s2 = sqrt0(1 - cth^2), perp = (nn cth +
// v1) ratio, d' = perp - nn sqrt(|1 - perp.perp|); ratio s2 > 1 reflects.
__device__ __forceinline__ f3 follow_direction(const bool glass, const bool front, const f3 on, const f3 nn,
                                               const f3 d)
{
    bool reflect = !glass;
    f3 nd = d;
    if (glass) {
        const float r1 = Math<true>::rsqrt(dot3(d, d));
        const f3 v1 = mk3(d.x * r1, d.y * r1, d.z * r1);
        const float x0 = -dot3(v1, nn);
        const float cth = 1.0f < x0 ? 1.0f : x0;
        const float s2 = Math<true>::sqrt0(__builtin_fmaf(-cth, cth, 1.0f));
        const float ratio = front ? 0.5f : 2.0f;
        reflect = ratio * s2 > 1.0f;
        const f3 perp = mk3(__builtin_fmaf(nn.x, cth, v1.x) * ratio, __builtin_fmaf(nn.y, cth, v1.y) * ratio,
                            __builtin_fmaf(nn.z, cth, v1.z) * ratio);
        const float s3 = Math<true>::sqrt(__builtin_fabsf(1.0f - dot3(perp, perp)));
        nd = mk3(__builtin_fmaf(nn.x, -s3, perp.x), __builtin_fmaf(nn.y, -s3, perp.y),
                 __builtin_fmaf(nn.z, -s3, perp.z));
    }
    if (reflect) {
        float k = dot3(on, d);
        k = k + k;
        nd = mk3(__builtin_fmaf(-k, on.x, d.x), __builtin_fmaf(-k, on.y, d.y), __builtin_fmaf(-k, on.z, d.z));
    }
    return nd;
}

// One thread per slab pixel, as features_kernel; 12 floats: {n.xyz, z},
// {P.xyz, hit}, {albedo.rgb, mean bounces}.  With max_bounces 0 every ray
// stops at its first hit with T = 1, and the sums are features_kernel's (1.0f
// * colour is the colour; z takes its one segment by the same fma).
template <bool kBvh>
__global__ __launch_bounds__(256) void features_follow_kernel(KArgs A, int max_bounces, float4 *__restrict__ feat)
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
    f3 n = mk3(0.0f, 0.0f, 0.0f), P = n, a = n;
    float z = 0.0f;
    int hits = 0, bsum = 0;
    for (int sy = 0; sy < A.nsub; ++sy)
        for (int sx = 0; sx < A.nsub; ++sx) {
            const float xin = __builtin_fmaf(C.b.w, 0.5f, (float)px + (float)sx * C.b.w);
            const float yin = __builtin_fmaf(C.b.w, 0.5f, (float)y + (float)sy * C.b.w);
            const float fs = xin * C.X.w;
            const float ft = yin * C.Y.w;
            f3 o = mk3(C.p.x, C.p.y, C.p.z);
            f3 d = mk3(__builtin_fmaf(C.Y.x, ft, __builtin_fmaf(C.X.x, fs, C.b.x)),
                       __builtin_fmaf(C.Y.y, ft, __builtin_fmaf(C.X.y, fs, C.b.y)),
                       __builtin_fmaf(C.Y.z, ft, __builtin_fmaf(C.X.z, fs, C.b.z)));
            f3 T = mk3(1.0f, 1.0f, 1.0f);
            float zr = z;  // the pixel's z with this ray's segments; kept only if the ray stops on a surface
            // at most max_bounces + 1 segments: b counts the bounces taken
            for (int b = 0; b <= max_bounces; ++b) {
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
                    break;  // sky
                // the hit point and the normals as shade<true> forms them
                const float4 s0 = hit->s0, s2 = hit->s2;
                const int mat = __float_as_int(hit->s1.w);
                const f3 p = mk3(__builtin_fmaf(d.x, t, o.x), __builtin_fmaf(d.y, t, o.y), __builtin_fmaf(d.z, t, o.z));
                const f3 on = mk3((p.x - s0.x) * s2.w, (p.y - s0.y) * s2.w, (p.z - s0.z) * s2.w);
                const bool front = dot3(on, d) < 0.0f;
                const f3 nn = mk3(front ? on.x : -on.x, front ? on.y : -on.y, front ? on.z : -on.z);
                zr = __builtin_fmaf(t, Math<true>::sqrt(dot3(d, d)), zr);
                const f3 Tc = mk3(T.x * s2.x, T.y * s2.y, T.z * s2.z);
                if ((mat != PTG_SPECULAR && mat != PTG_DIELECTRIC) || b == max_bounces) {
                    hits += 1;
                    bsum += b;
                    n = mk3(n.x + nn.x, n.y + nn.y, n.z + nn.z);
                    P = mk3(P.x + p.x, P.y + p.y, P.z + p.z);
                    a = mk3(a.x + Tc.x, a.y + Tc.y, a.z + Tc.z);
                    z = zr;
                    break;
                }
                T = Tc;
                d = follow_direction(mat == PTG_DIELECTRIC, front, on, nn, d);
                o = p;
            }
        }
    const float k = (float)(hits > 0 ? hits : 1);
    float4 *out = feat + (size_t)i * 3;
    out[0] = make_float4(n.x / k, n.y / k, n.z / k, z / k);
    out[1] = make_float4(P.x / k, P.y / k, P.z / k, (float)hits / (float)A.lanes_per_pixel);
    out[2] = hits > 0 ? make_float4(a.x / k, a.y / k, a.z / k, (float)bsum / k) : make_float4(1.0f, 1.0f, 1.0f, 0.0f);
}
