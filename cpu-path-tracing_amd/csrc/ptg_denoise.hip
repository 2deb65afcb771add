// ptg_denoise.hip -- the variance-guided a-trous filter of include/ptgpu.h
// ("denoising"): its kernels and the C ABI around them.  The arithmetic is
// denoise_filter.hpp's, shared with the host loop; this file needs no context
// -- the render-and-denoise drivers are csrc/ptg_frames.cpp's and
// csrc/ptg_multi.cpp's.
//
// Kernels: one thread per pixel, workgroups of 64 x 4 pixels (a wave's lanes
// contiguous in x).  dn_filter_tiled_kernel stages the taps in LDS (steps up
// to 16); dn_filter_kernel reads every tap from global memory through the
// caches -- the larger steps, and the A/B partner (DESIGN.md "Denoising").
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "denoise_filter.hpp"

extern "C" int ptg_set_error_(int code, const char *msg);

namespace {

using namespace ptg_dn;

int fail(int code, const std::string &msg) { return ptg_set_error_(code, msg.c_str()); }

#define PTG_DN_HIP(call)                                                                           \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(PTG_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)

constexpr int kTileX = 64, kTileY = 4;
constexpr int kMaxDevices = 64;

__global__ __launch_bounds__(kTileX *kTileY) void dn_vbar_kernel(const float *__restrict__ var,
                                                                 float *__restrict__ vbar, int W, int H)
{
    const int x = blockIdx.x * kTileX + threadIdx.x;
    const int y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= W || y >= H)
        return;
    vbar[(size_t)y * W + x] = vbar_pixel(var, W, H, x, y);
}

__global__ __launch_bounds__(kTileX *kTileY) void dn_filter_kernel(const float *__restrict__ color,
                                                                   const float *__restrict__ var,
                                                                   const float *__restrict__ vbar,
                                                                   const float *__restrict__ feat, int W, int H,
                                                                   int s, ptg_denoise_params k,
                                                                   float *__restrict__ c_out,
                                                                   float *__restrict__ v_out)
{
    const int x = blockIdx.x * kTileX + threadIdx.x;
    const int y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= W || y >= H)
        return;
    filter_pixel(color, var, vbar, feat, W, H, x, y, s, k, c_out, v_out);
}

// The tiled kernel.  The taps of step s form s^2 independent lattices: a
// workgroup takes 64 columns of 4 rows that are s apart (one y residue mod s),
// so its lanes are contiguous in x at any s, and stages in LDS what the 25
// taps of its pixels read: columns [x0 - 2s, x0 + 64 + 2s) of the 4 + 4
// lattice rows around them -- every global read a row segment.  17 words per
// tile pixel (colour, variance, Vbar, normal, point, hit, albedo), each word a
// plane of its own: a wave reads 64 consecutive floats of a plane per tap
// word, no bank conflict.  Positions outside the image are neither loaded
// nor read (filter_taps skips those taps).
constexpr int kTileRows = kTileY + 4;
constexpr int kTileWords = 17;
// steps 1 .. 16 (128 x 8 x 17 words = 68 KiB of the 160 KiB at step 16): at step 32 the tile is 102 KiB, one
// workgroup per CU, and the plain kernel is faster (0.29 against 0.36 ms at 1920x1080); step 64 would not fit
constexpr int kTiledMaxStep = 16;
__host__ __device__ constexpr int tile_width(int s) { return kTileX + 4 * s; }
constexpr size_t tile_bytes(int s) { return (size_t)kTileWords * kTileRows * tile_width(s) * sizeof(float); }

__global__ __launch_bounds__(kTileX *kTileY) void dn_filter_tiled_kernel(
    const float *__restrict__ color, const float *__restrict__ var, const float *__restrict__ vbar,
    const float *__restrict__ feat, int W, int H, int s, int row_groups, ptg_denoise_params k,
    float *__restrict__ c_out, float *__restrict__ v_out)
{
    extern __shared__ float tile[];
    const int TW = tile_width(s);
    const int plane = kTileRows * TW;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x0 = blockIdx.x * kTileX;
    const int ry = blockIdx.y / row_groups;                 // the lattice's y residue, 0 .. s - 1
    const int j0 = (blockIdx.y - ry * row_groups) * kTileY;  // first lattice row of the workgroup
    for (int tr = ty; tr < kTileRows; tr += kTileY) {
        const int gy = ry + s * (j0 + tr - 2);
        if (gy < 0 || gy >= H)
            continue;
        for (int tc = tx; tc < TW; tc += kTileX) {
            const int gx = x0 - 2 * s + tc;
            if (gx < 0 || gx >= W)
                continue;
            const size_t i = (size_t)gy * W + gx;
            float *t = tile + tr * TW + tc;
            const float *c = color + i * 3, *v = var + i * 3, *f = feat + i * kFeat;
            t[0 * plane] = c[0], t[1 * plane] = c[1], t[2 * plane] = c[2];
            t[3 * plane] = v[0], t[4 * plane] = v[1], t[5 * plane] = v[2];
            t[6 * plane] = vbar[i];
            t[7 * plane] = f[0], t[8 * plane] = f[1], t[9 * plane] = f[2];
            t[10 * plane] = f[4], t[11 * plane] = f[5], t[12 * plane] = f[6], t[13 * plane] = f[7];
            t[14 * plane] = f[8], t[15 * plane] = f[9], t[16 * plane] = f[10];
        }
    }
    __syncthreads();
    const int x = x0 + tx;
    const int y = ry + s * (j0 + ty);
    if (x >= W || y >= H)
        return;
    auto fetch = [&](int col, int row, Guide &q, float *vq) {
        const float *t = tile + row * TW + col;
        q.c[0] = t[0 * plane], q.c[1] = t[1 * plane], q.c[2] = t[2 * plane];
        vq[0] = t[3 * plane], vq[1] = t[4 * plane], vq[2] = t[5 * plane];
        q.vbar = t[6 * plane];
        q.n[0] = t[7 * plane], q.n[1] = t[8 * plane], q.n[2] = t[9 * plane];
        q.P[0] = t[10 * plane], q.P[1] = t[11 * plane], q.P[2] = t[12 * plane], q.hit = t[13 * plane];
        q.a[0] = t[14 * plane], q.a[1] = t[15 * plane], q.a[2] = t[16 * plane];
        q.z = 0.0f;  // (only the centre's distance is read)
    };
    const size_t ip = (size_t)y * W + x;
    Guide p;
    float vp[3];
    fetch(tx + 2 * s, ty + 2, p, vp);
    p.z = feat[ip * kFeat + 3];
    filter_taps(
        p, W, H, x, y, s, k,
        [&](int dx, int dy, int, int, Guide &q, float *vq) { fetch(tx + 2 * s + s * dx, ty + 2 + dy, q, vq); },
        c_out + ip * 3, v_out + ip * 3);
}

int check_frame(int32_t width, int32_t height)
{
    if (width <= 0 || height <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise: width and height must be positive");
    if ((int64_t)width * height > (int64_t)1 << 28)
        return fail(PTG_ERR_UNSUPPORTED, "denoise: image too large");
    return PTG_OK;
}

}  // namespace

extern "C" {

int ptg_denoise_defaults(ptg_denoise_params *out)
{
    if (!out)
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise_defaults: NULL argument");
    defaults(out);
    return PTG_OK;
}

int ptg_pixel_spread(const ptg_camera *cam, int32_t width, int32_t height, float *spread)
{
    if (!cam || !spread || width <= 0 || height <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "pixel_spread: NULL camera or output, or an empty frame");
    double xx = 0.0, yy = 0.0, cc = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double X = cam->cam_x_axis[c], Y = cam->cam_y_axis[c];
        const double mid = cam->lower_left_corner[c] - cam->position[c] + 0.5 * X + 0.5 * Y;
        xx += X * X, yy += Y * Y, cc += mid * mid;
    }
    const double px = std::sqrt(xx) / width, py = std::sqrt(yy) / height;
    const double v = (px > py ? px : py) / std::sqrt(cc);
    if (!(v > 0.0) || !std::isfinite(v))
        return fail(PTG_ERR_INVALID_ARGUMENT, "pixel_spread: degenerate camera");
    *spread = (float)v;
    return PTG_OK;
}

int ptg_denoise_scratch_bytes(int32_t width, int32_t height, size_t *bytes)
{
    if (!bytes)
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise_scratch_bytes: NULL argument");
    int rc = check_frame(width, height);
    if (rc)
        return rc;
    *bytes = scratch_of(width, height).total * sizeof(float);
    return PTG_OK;
}

// internal (tests, tools/denoise_cost.py): ptg_denoise_device with the filter kernel named: 0 the tiled kernel
// wherever its tile fits (what ptg_denoise_device launches), 1 the plain kernel only
int ptg_denoise_device_kernel_(const float *d_color, const float *d_var, const float *d_feat, int32_t width,
                               int32_t height, const ptg_denoise_params *params, float *d_out, float *d_var_out,
                               void *d_scratch, size_t scratch_bytes, void *stream, int kernel_choice)
{
    int rc = check_frame(width, height);
    if (rc)
        return rc;
    if (const char *why = params_error(params))
        return fail(PTG_ERR_INVALID_ARGUMENT, why);
    if (!d_color || !d_var || !d_feat || !d_out || !d_scratch)
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise: NULL buffer");
    const Scratch S = scratch_of(width, height);
    if (scratch_bytes < S.total * sizeof(float))
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise: scratch of " + std::to_string(scratch_bytes) + " bytes, " +
                                                  std::to_string(S.total * sizeof(float)) + " needed");
    if (kernel_choice < 0 || kernel_choice > 1)
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise: kernel choice 0 (tiled where it fits) or 1 (plain)");
    // once per process: a device is there; once per device: the tiled kernel may use more than the default 64 KiB
    // of dynamic LDS (step 16).  Later calls only queue copies and kernels.
    static std::atomic<int> n_devices{0};
    static std::atomic<bool> lds_raised[kMaxDevices];
    if (n_devices.load(std::memory_order_relaxed) <= 0) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            return fail(PTG_ERR_NO_DEVICE, "no HIP device visible");
        n_devices.store(count, std::memory_order_relaxed);
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (params->iterations == 0) {
        PTG_DN_HIP(hipMemcpyAsync(d_out, d_color, S.frame * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (d_var_out)
            PTG_DN_HIP(hipMemcpyAsync(d_var_out, d_var, S.frame * sizeof(float), hipMemcpyDeviceToDevice, s));
        return PTG_OK;
    }
    float *work = static_cast<float *>(d_scratch);
    float *cbuf[2] = {work, work + S.frame};
    float *vbuf[2] = {work + 2 * S.frame, work + 3 * S.frame};
    float *vbar = work + 4 * S.frame;
    const dim3 block(kTileX, kTileY);
    const dim3 grid((unsigned)((width + kTileX - 1) / kTileX), (unsigned)((height + kTileY - 1) / kTileY));
    const float *cin = d_color, *vin = d_var;
    for (int it = 0; it < params->iterations; ++it) {
        const bool last = it + 1 == params->iterations;
        float *co = last ? d_out : cbuf[it & 1];
        float *vo = last && d_var_out ? d_var_out : vbuf[it & 1];
        dn_vbar_kernel<<<grid, block, 0, s>>>(vin, vbar, width, height);
        const int step = 1 << it;
        const int row_groups = ((height + step - 1) / step + kTileY - 1) / kTileY;
        if (kernel_choice == 0 && step <= kTiledMaxStep && (long long)step * row_groups <= 65535) {
            if (tile_bytes(step) > 64 * 1024) {
                int dev = 0;
                PTG_DN_HIP(hipGetDevice(&dev));
                if (dev < 0 || dev >= kMaxDevices || !lds_raised[dev].load(std::memory_order_acquire)) {
                    PTG_DN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dn_filter_tiled_kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)tile_bytes(kTiledMaxStep)));
                    if (dev >= 0 && dev < kMaxDevices)
                        lds_raised[dev].store(true, std::memory_order_release);
                }
            }
            dn_filter_tiled_kernel<<<dim3(grid.x, (unsigned)(step * row_groups)), block, tile_bytes(step), s>>>(
                cin, vin, vbar, d_feat, width, height, step, row_groups, *params, co, vo);
        } else
            dn_filter_kernel<<<grid, block, 0, s>>>(cin, vin, vbar, d_feat, width, height, step, *params, co, vo);
        cin = co;
        vin = vo;
    }
    PTG_DN_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_denoise_device(const float *d_color, const float *d_var, const float *d_feat, int32_t width, int32_t height,
                       const ptg_denoise_params *params, float *d_out, float *d_var_out, void *d_scratch,
                       size_t scratch_bytes, void *stream)
{
    return ptg_denoise_device_kernel_(d_color, d_var, d_feat, width, height, params, d_out, d_var_out, d_scratch,
                                      scratch_bytes, stream, 0);
}

int ptg_denoise_host(const float *color, const float *var, const float *feat, int32_t width, int32_t height,
                     const ptg_denoise_params *params, float *out, float *var_out)
{
    int rc = check_frame(width, height);
    if (rc)
        return rc;
    if (const char *why = params_error(params))
        return fail(PTG_ERR_INVALID_ARGUMENT, why);
    if (!color || !var || !feat || !out)
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise: NULL buffer");
    std::vector<float> work(scratch_of(width, height).total);
    filter_host(color, var, feat, width, height, *params, out, var_out, work.data(), nullptr);
    return PTG_OK;
}

// Host helper: the feature frame of ptg_features_device, width * height * 12 floats in ptg_render's row
// order, copied to the host (shard_count 1).  Synchronous.
static int features_host(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                         int device, int32_t max_bounces, float *features)
{
    if (max_bounces < -1 || max_bounces > PTG_MAX_FOLLOW_BOUNCES)  // (-1: ptg_features)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: max_bounces must be 0..16");
    if (!features || !params || !cam)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: NULL output, camera or params");
    if (params->width <= 0 || params->height <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (params->shard_count != 1)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: shard_count must be 1 (a whole frame)");
    ptg_context *ctx = nullptr;
    int rc = ptg_context_create(spheres, n_spheres, cam, device, &ctx);
    if (rc)
        return rc;
    int32_t rows = 0;
    float *d_feat = nullptr;
    const size_t frame = (size_t)params->width * params->height * kFeat;
    rc = ptg_shard_rows(params->height, params->band_rows, 1, &rows);
    if (!rc && hipMalloc(&d_feat, (size_t)rows * params->width * kFeat * sizeof(float)) != hipSuccess)
        rc = fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the feature slab failed");
    if (!rc)
        rc = max_bounces < 0 ? ptg_features_device(ctx, params, d_feat, nullptr)
                             : ptg_features_follow_device(ctx, params, max_bounces, d_feat, nullptr);
    if (!rc) {
        const hipError_t e = hipMemcpy(features, d_feat, frame * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            rc = fail(PTG_ERR_HIP, std::string("features: ") + hipGetErrorString(e));
    }
    if (d_feat)
        (void)hipFree(d_feat);
    ptg_context_destroy(ctx);
    return rc;
}

int ptg_features(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                 int device, float *features)
{
    return features_host(spheres, n_spheres, cam, params, device, -1, features);
}

int ptg_features_follow(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                        const ptg_params *params, int device, int32_t max_bounces, float *features)
{
    if (max_bounces < 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: max_bounces must be 0..16");
    return features_host(spheres, n_spheres, cam, params, device, max_bounces, features);
}

// internal (the drivers in csrc/ptg_frames.cpp and csrc/ptg_multi.cpp): the filter's parameters a driver runs with -- `denoise`,
// or the defaults when it is NULL, with the camera's pixel_spread when it is NULL or gives 0 -- checked
int ptg_denoise_params_for_(const ptg_camera *cam, int32_t width, int32_t height, const ptg_denoise_params *denoise,
                            ptg_denoise_params *out)
{
    if (!cam || !out)
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise: NULL camera or output");
    if (denoise)
        *out = *denoise;
    else
        defaults(out);
    int rc;
    if ((!denoise || out->pixel_spread == 0.0f) && (rc = ptg_pixel_spread(cam, width, height, &out->pixel_spread)))
        return rc;
    if (const char *why = params_error(out))
        return fail(PTG_ERR_INVALID_ARGUMENT, why);
    if (out->follow_bounces < 0 || out->follow_bounces > PTG_MAX_FOLLOW_BOUNCES)
        return fail(PTG_ERR_INVALID_ARGUMENT, "denoise: follow_bounces must be 0..16");
    return PTG_OK;
}

// internal (the same drivers): the feature slab a driver's filter is guided by -- the first hit, or with
// follow_bounces 1..16 the first diffuse hit behind mirrors and glass
int ptg_features_for_(ptg_context *ctx, const ptg_params *params, const ptg_denoise_params *k, float *d_feat,
                      void *stream)
{
    return k->follow_bounces ? ptg_features_follow_device(ctx, params, k->follow_bounces, d_feat, stream)
                             : ptg_features_device(ctx, params, d_feat, stream);
}

}  // extern "C"
