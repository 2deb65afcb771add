// denoise_filter.hpp -- the arithmetic of the variance-guided a-trous filter
// (include/ptgpu.h "denoising", DESIGN.md "Denoising"), per tap and per pixel,
// as __host__ __device__ inline functions: the kernels of ptg_denoise.hip and
// the host loop below (ptg_denoise_host, tests/denoise_check.cpp) call the
// same code.  All fp32 in a fixed operation order: explicit fmaf, correctly
// rounded '/', no exp, pow or approximate instruction -- compiled with
// -ffp-contract=off a CPU reproduces the device's bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/ptgpu.h"

#if defined(__HIPCC__)
#define PTG_DN_HD __host__ __device__ inline
#else
#define PTG_DN_HD inline
#endif

namespace ptg_dn {

constexpr int kMaxIterations = 8;
constexpr int kFeat = 12;       // floats per pixel: {n.xyz, z}, {P.xyz, hit}, {albedo.rgb, 0}
constexpr float kZMin = 1e-4f;  // the plane term's least distance

PTG_DN_HD float fmax_(float a, float b) { return a > b ? a : b; }
PTG_DN_HD float fabs_(float a) { return a < 0.0f ? -a : a; }
PTG_DN_HD int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// h = [1/16, 1/4, 3/8, 1/4, 1/16] at d = -2..2
PTG_DN_HD float tap_h(int d)
{
    const int a = d < 0 ? -d : d;
    return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f);
}

// Vbar_p: the 3x3 [1 2 1]x[1 2 1]/16 average of V_r + V_g + V_b, coordinates
// clamped to the image, rows top to bottom, left to right
PTG_DN_HD float vbar_pixel(const float *var, int W, int H, int x, int y)
{
    float acc = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = clampi(y + dy, H - 1);
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = clampi(x + dx, W - 1);
            const float *v = var + ((size_t)yy * W + xx) * 3;
            const float k = (dy == 0 ? 2.0f : 1.0f) * (dx == 0 ? 2.0f : 1.0f) * 0.0625f;
            acc = __builtin_fmaf(k, (v[0] + v[1]) + v[2], acc);
        }
    }
    return acc;
}

// What the weight reads of a pixel
struct Guide {
    float c[3];
    float vbar;
    float n[3], z;
    float P[3], hit;
    float a[3];
};

PTG_DN_HD Guide load_guide(const float *color, const float *vbar, const float *feat, size_t i)
{
    Guide g;
    const float *c = color + i * 3;
    const float *f = feat + i * kFeat;
    g.c[0] = c[0], g.c[1] = c[1], g.c[2] = c[2];
    g.vbar = vbar[i];
    g.n[0] = f[0], g.n[1] = f[1], g.n[2] = f[2], g.z = f[3];
    g.P[0] = f[4], g.P[1] = f[5], g.P[2] = f[6], g.hit = f[7];
    g.a[0] = f[8], g.a[1] = f[9], g.a[2] = f[10];
    return g;
}

PTG_DN_HD float sq3(float x, float y, float z) { return __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)); }

// The edge-stopping factor t^8 of tap q seen from p; step_spread = s * pixel_spread.
PTG_DN_HD float tap_t8(const Guide &p, const Guide &q, float step_spread, const ptg_denoise_params &k)
{
    const float d2 = sq3(p.c[0] - q.c[0], p.c[1] - q.c[1], p.c[2] - q.c[2]);
    float x = (k.k_color * d2) / ((p.vbar + q.vbar) + k.eps_color);
    const bool sky_p = p.hit == 0.0f, sky_q = q.hit == 0.0f;
    if (sky_p != sky_q)
        return 0.0f;
    if (!sky_p) {
        const float nd = __builtin_fmaf(p.n[2], q.n[2], __builtin_fmaf(p.n[1], q.n[1], p.n[0] * q.n[0]));
        x = __builtin_fmaf(k.k_normal, fmax_(0.0f, 1.0f - nd), x);
        const float pd = __builtin_fmaf(p.n[2], q.P[2] - p.P[2],
                                        __builtin_fmaf(p.n[1], q.P[1] - p.P[1], p.n[0] * (q.P[0] - p.P[0])));
        x = x + (k.k_plane * fabs_(pd)) / (step_spread * fmax_(p.z, kZMin));
        x = __builtin_fmaf(k.k_albedo, sq3(p.a[0] - q.a[0], p.a[1] - q.a[1], p.a[2] - q.a[2]), x);
        if (p.hit != q.hit)
            x = __builtin_fmaf(k.k_normal, fabs_(p.hit - q.hit), x);
    }
    const float t = fmax_(__builtin_fmaf(x, -0.125f, 1.0f), 0.0f);  // (a NaN x gives 0)
    const float t2 = t * t;
    const float t4 = t2 * t2;
    return t4 * t4;
}

// One pixel p = (x, y) of iteration s: its 25 taps in (dy, dx) order, taps
// outside the image skipped.  tap(dx, dy, xx, yy, q, vq) fetches what the tap
// at (xx, yy) = p + s (dx, dy) contributes -- its guide and its variance --
// from wherever the caller keeps the frame (global memory, an LDS tile, host
// memory): the arithmetic and its order are here, once.  Returns sum w.
template <class Tap>
PTG_DN_HD float filter_taps(const Guide &p, int W, int H, int x, int y, int s, const ptg_denoise_params &k, Tap tap,
                            float *c_out3, float *v_out3)
{
    const float step_spread = (float)s * k.pixel_spread;
    float sw = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f}, sv[3] = {0.0f, 0.0f, 0.0f};
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + s * dy;
        if (yy < 0 || yy >= H)
            continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + s * dx;
            if (xx < 0 || xx >= W)
                continue;
            Guide q;
            float vq[3];
            tap(dx, dy, xx, yy, q, vq);
            // the centre tap by definition at x = 0 (a mean normal is shorter than 1): sum w >= 9/64
            const float t8 = (dx | dy) == 0 ? 1.0f : tap_t8(p, q, step_spread, k);
            const float w = (tap_h(dx) * tap_h(dy)) * t8;
            const float w2 = w * w;
            sw = sw + w;
            for (int c = 0; c < 3; ++c) {
                sc[c] = __builtin_fmaf(w, q.c[c], sc[c]);
                sv[c] = __builtin_fmaf(w2, vq[c], sv[c]);
            }
        }
    }
    const float sw2 = sw * sw;
    for (int c = 0; c < 3; ++c) {
        c_out3[c] = sc[c] / sw;
        v_out3[c] = sv[c] / sw2;
    }
    return sw;
}

// The same with every tap read from the frames in (global or host) memory.
PTG_DN_HD float filter_pixel(const float *color, const float *var, const float *vbar, const float *feat, int W, int H,
                             int x, int y, int s, const ptg_denoise_params &k, float *c_out, float *v_out)
{
    const size_t ip = (size_t)y * W + x;
    const Guide p = load_guide(color, vbar, feat, ip);
    return filter_taps(
        p, W, H, x, y, s, k,
        [=](int, int, int xx, int yy, Guide &q, float *vq) {
            const size_t iq = (size_t)yy * W + xx;
            q = load_guide(color, vbar, feat, iq);
            vq[0] = var[iq * 3], vq[1] = var[iq * 3 + 1], vq[2] = var[iq * 3 + 2];
        },
        c_out + ip * 3, v_out + ip * 3);
}

// Argument rules shared by the device and the host entry point; NULL when fine.
inline const char *params_error(const ptg_denoise_params *k)
{
    if (!k)
        return "denoise: params is NULL";
    if (k->iterations < 0 || k->iterations > kMaxIterations)
        return "denoise: iterations must be in [0, 8]";
    if (!(k->eps_color > 0.0f) || !(k->eps_color < 1e30f))
        return "denoise: eps_color must be > 0";
    if (!(k->pixel_spread > 0.0f) || !(k->pixel_spread < 1e30f))
        return "denoise: pixel_spread must be > 0";
    for (float v : {k->k_color, k->k_normal, k->k_plane, k->k_albedo})
        if (!(v >= 0.0f) || !(v < 1e30f))
            return "denoise: k_color, k_normal, k_plane and k_albedo must be finite and >= 0";
    return nullptr;
}

// Scratch layout of a W x H frame, in floats: two colour and two variance
// frames (ping-pong), then Vbar
struct Scratch {
    size_t frame;  // W * H * 3
    size_t total;  // floats
};
inline Scratch scratch_of(int W, int H)
{
    const size_t px = (size_t)W * (size_t)H;
    return Scratch{px * 3, px * 13};
}

// The whole filter on host buffers: the definition the kernels are held to.
// work: scratch_of(W, H).total floats.  min_sum_w (optional) receives the
// smallest sum w over all pixels and iterations.
inline void filter_host(const float *color, const float *var, const float *feat, int W, int H,
                        const ptg_denoise_params &k, float *out, float *var_out, float *work, float *min_sum_w)
{
    const Scratch S = scratch_of(W, H);
    const size_t px = (size_t)W * H;
    float *cbuf[2] = {work, work + S.frame};
    float *vbuf[2] = {work + 2 * S.frame, work + 3 * S.frame};
    float *vbar = work + 4 * S.frame;
    float least = 1e30f;
    if (k.iterations == 0) {
        for (size_t i = 0; i < px * 3; ++i) {
            out[i] = color[i];
            if (var_out)
                var_out[i] = var[i];
        }
    }
    const float *cin = color, *vin = var;
    for (int it = 0; it < k.iterations; ++it) {
        const bool last = it + 1 == k.iterations;
        float *co = last ? out : cbuf[it & 1];
        float *vo = last && var_out ? var_out : vbuf[it & 1];
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                vbar[(size_t)y * W + x] = vbar_pixel(vin, W, H, x, y);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float sw = filter_pixel(cin, vin, vbar, feat, W, H, x, y, 1 << it, k, co, vo);
                least = sw < least ? sw : least;
            }
        cin = co;
        vin = vo;
    }
    if (min_sum_w)
        *min_sum_w = least;
}

inline void defaults(ptg_denoise_params *k)
{
    *k = ptg_denoise_params{};
    k->iterations = 5;
    k->k_color = 0.35f;
    k->k_normal = 32.0f;
    k->k_plane = 1.0f;
    k->k_albedo = 16.0f;
    k->eps_color = 1e-6f;
    k->pixel_spread = 1.0f / 1024.0f;
}

}  // namespace ptg_dn
