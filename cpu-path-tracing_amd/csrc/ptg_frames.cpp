// ptg_frames.cpp -- the one-device whole-frame drivers of include/ptgpu.h: ptg_render_to_noise,
// ptg_render_adaptive and their filtered forms ptg_render_denoised, ptg_render_to_noise_denoised,
// ptg_render_adaptive_denoised.  Host code over the public device entry points of ptg_render.hip and
// ptg_denoise.hip: the loops and checks are frame_passes.hpp's, shared with csrc/ptg_multi.cpp; the drivers
// differ in how the frame is finished -- resolve (with each pixel's count after adaptive passes), and for the
// filtered forms variance slab, features, filter.
#include <hip/hip_runtime.h>

#include <vector>

#include "frame_passes.hpp"
#include "launch_plan.hpp"  // check_params

// csrc/ptg_denoise.hip: the filter parameters a driver runs with, checked; the feature slab they ask for
extern "C" int ptg_denoise_params_for_(const ptg_camera *cam, int32_t width, int32_t height,
                                       const ptg_denoise_params *denoise, ptg_denoise_params *out);
extern "C" int ptg_features_for_(ptg_context *ctx, const ptg_params *params, const ptg_denoise_params *k,
                                 float *d_feat, void *stream);

namespace {

using namespace ptg_frames;
using ptg_frames::fail;  // (launch_plan.hpp brings ptg::fail's namespace along)

#define FRAME_HIP(call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(PTG_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)

constexpr int kFeat = 12;  // floats per pixel of ptg_features_device

// The loops' steps from a context: everything on the null stream, in order; each check's statistics (32 bytes,
// a selection's 48) copied back synchronously.  d_stats: 6 statistics, then the 4 kernel counters.
struct ContextSteps {
    ptg_context *ctx;
    const ptg_params &p;
    unsigned long long *d_stats;
    bool count;

    int read(unsigned long long *st, size_t bytes)
    {
        FRAME_HIP(hipMemcpy(st, d_stats, bytes, hipMemcpyDeviceToHost));
        return PTG_OK;
    }
    int reset() { return ptg_reset_accumulation_device(ctx, &p, nullptr); }
    int accumulate(int32_t b, int32_t e) { return ptg_accumulate_device(ctx, &p, b, e, nullptr, nullptr); }
    int noise(int32_t done, double rel_error, double floor, unsigned long long *st)
    {
        FRAME_HIP(hipMemsetAsync(d_stats, 0, 4 * sizeof(*st), nullptr));
        const int rc = ptg_noise_device(ctx, &p, done, rel_error, floor, nullptr, nullptr, d_stats, nullptr);
        return rc ? rc : read(st, 4 * sizeof(*st));
    }
    int all_active() { return ptg_set_active_mask_device(ctx, &p, nullptr, nullptr, nullptr); }
    int accumulate_active(int32_t add, long long units)
    {
        return ptg_accumulate_active_device(ctx, &p, add, units, count ? d_stats + 6 : nullptr, nullptr);
    }
    int select(double rel_error, double floor, int32_t dilate, unsigned long long *st)
    {
        FRAME_HIP(hipMemsetAsync(d_stats, 0, 6 * sizeof(*st), nullptr));
        const int rc = ptg_select_active_device(ctx, &p, rel_error, floor, dilate, nullptr, d_stats, nullptr);
        return rc ? rc : read(st, 6 * sizeof(*st));
    }
};

// shard_count 1 and fp32, as every driver here needs them; `why` and `fp32` end the two messages
int check_whole_frame(const std::string &who, const ptg_params *p, const char *why, const char *fp32)
{
    if (p->shard_count != 1)
        return fail(PTG_ERR_INVALID_ARGUMENT, who + ": shard_count must be 1 (" + why + ")");
    if (p->flags & PTG_FLAG_REFERENCE_F64)
        return fail(PTG_ERR_UNSUPPORTED, who + ": " + fp32);
    return PTG_OK;
}
const char *const kOneDecides = "one device decides for the whole frame";
const char *const kFilterNeeds = "the filter needs the whole frame";
const char *const kProgressive = "progressive passes are fp32 only";

// One frame on one device, the arguments checked: the adaptive loop with `at`, else the noise-target loop (`nt`
// NULL: its passes unchecked); the frame finished through the filter `k` where there is one; ADDED into image_rgb.
int render_frame(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                 int device, const Passes &ps, const ptg_noise_target *nt, const ptg_adaptive_target *at,
                 const ptg_denoise_params *k, double *image_rgb, int32_t *sample_counts, ptg_noise_report *noise_report,
                 ptg_adaptive_report *adaptive_report)
{
    ptg_context *ctx = nullptr;
    int rc = ptg_context_create(spheres, n_spheres, cam, device, &ctx);
    if (rc)
        return rc;
    ptg_params p = *params;
    if (!at)
        p.flags |= PTG_FLAG_MOMENTS;
    const int W = p.width, H = p.height;
    const bool count = at && (p.flags & (PTG_FLAG_COUNT_TESTS | PTG_FLAG_COUNT_NONFINITE)) != 0;
    float *d_buf = nullptr;
    std::vector<float> host((size_t)H * W * 3);
    std::vector<int32_t> host_counts(sample_counts ? (size_t)H * W : 0);
    ptg_noise_report nrep{};
    ptg_adaptive_report arep{};
    auto run = [&]() -> int {
        int r;
        int32_t rows = 0;
        size_t scratch_bytes = 0;
        if ((r = ptg_shard_rows(H, p.band_rows, 1, &rows)) ||
            (k && (r = ptg_denoise_scratch_bytes(W, H, &scratch_bytes))))
            return r;
        // one allocation: the statistics and kernel counters, the colour slab, the counts, and for the filter the
        // features, the variance and output slabs and its scratch -- every part starts at a multiple of 64 floats
        // (256 B: ptg_features_device stores float4, the statistics are 64-bit atomics), whatever rows * W is
        const auto part = [](size_t floats) { return (floats + 63) / 64 * 64; };
        const size_t stats = part(2 * 10), slab = part((size_t)rows * W * 3), cnt = part((size_t)rows * W);
        const size_t feat = k ? part((size_t)rows * W * kFeat) : 0;
        const size_t total = stats + slab + cnt + (k ? feat + 2 * slab + part(scratch_bytes / sizeof(float)) : 0);
        if (hipMalloc(&d_buf, total * sizeof(float)) != hipSuccess)
            return fail(PTG_ERR_OUT_OF_MEMORY, k ? "hipMalloc of the denoiser's frames failed"
                                                 : "hipMalloc of the image slab failed");
        unsigned long long *d_stats = reinterpret_cast<unsigned long long *>(d_buf);
        float *d_color = d_buf + stats, *d_out = d_color;
        int32_t *d_cnt = reinterpret_cast<int32_t *>(d_color + slab);
        FRAME_HIP(hipMemsetAsync(d_stats, 0, 10 * sizeof(unsigned long long), nullptr));
        ContextSteps steps{ctx, p, d_stats, count};
        int32_t done = 0;
        if ((r = at ? adaptive_passes(steps, p, ps, *at, arep) : noise_passes(steps, ps, nt, nrep, done)) ||
            (r = at ? ptg_resolve_active_device(ctx, &p, d_color, nullptr)
                    : ptg_resolve_device(ctx, &p, done, d_color, nullptr)))
            return r;
        if (k) {
            float *d_feat = d_color + slab + cnt, *d_var = d_feat + feat, *d_scratch = d_var + 2 * slab;
            d_out = d_var + slab;
            if ((r = at ? ptg_noise_active_device(ctx, &p, 1.0, d_var, nullptr, nullptr)
                        : ptg_noise_device(ctx, &p, done, 0.0, 1.0, d_var, nullptr, nullptr, nullptr)) ||
                (r = ptg_features_for_(ctx, &p, k, d_feat, nullptr)) ||
                (r = ptg_denoise_device(d_color, d_var, d_feat, W, H, k, d_out, nullptr, d_scratch, scratch_bytes,
                                        nullptr)))
                return r;
        }
        if (sample_counts) {
            if ((r = ptg_read_sample_counts_device(ctx, &p, d_cnt, nullptr)))
                return r;
            FRAME_HIP(hipMemcpy(host_counts.data(), d_cnt, host_counts.size() * sizeof(int32_t),
                                hipMemcpyDeviceToHost));
        }
        if (count)
            FRAME_HIP(hipMemcpy(arep.counters, d_stats + 6, sizeof(arep.counters), hipMemcpyDeviceToHost));
        // shard_count 1: slab row j is image row j, the rows past the image stay behind
        FRAME_HIP(hipMemcpy(host.data(), d_out, host.size() * sizeof(float), hipMemcpyDeviceToHost));
        return PTG_OK;
    };
    rc = run();
    if (d_buf)
        (void)hipFree(d_buf);
    ptg_context_destroy(ctx);
    if (rc)
        return rc;
    add_image(image_rgb, host.data(), host.size());
    if (sample_counts)
        std::memcpy(sample_counts, host_counts.data(), host_counts.size() * sizeof(int32_t));
    if (noise_report)
        *noise_report = nrep;
    if (adaptive_report)
        *adaptive_report = arep;
    return PTG_OK;
}

// ptg_render_denoised, and with a target ptg_render_to_noise_denoised (whose target errors carry the unfiltered
// driver's name)
int render_denoised(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                    int device, const ptg_denoise_params *denoise, const ptg_noise_target *target, double *image_rgb,
                    ptg_noise_report *report)
{
    if (!image_rgb || !params || !cam)
        return fail(PTG_ERR_INVALID_ARGUMENT, "render_denoised: NULL image, camera or params");
    if (params->width <= 0 || params->height <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (params->samples < 2)
        return fail(PTG_ERR_INVALID_ARGUMENT, "render_denoised: samples must be >= 2 (the variance needs two)");
    int rc;
    Passes ps;
    ps.ends[0] = params->samples;
    ps.n = 1;
    ptg_denoise_params k;
    if ((rc = check_whole_frame("render_denoised", params, kFilterNeeds,
                                "fp32 only (no progressive passes in the reference-arithmetic mode)")) ||
        (target && (rc = check_target("render_to_noise", target_of(*target), params->samples, ps))) ||
        (rc = ptg_denoise_params_for_(cam, params->width, params->height, denoise, &k)))
        return rc;
    return render_frame(spheres, n_spheres, cam, params, device, ps, target, nullptr, &k, image_rgb, nullptr, report,
                        nullptr);
}

}  // namespace

extern "C" {

int ptg_render_to_noise(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                        int device, const ptg_noise_target *target, double *image_rgb, ptg_noise_report *report)
{
    if (!image_rgb || !target)
        return ptg_frames::fail(PTG_ERR_INVALID_ARGUMENT, "render_to_noise: NULL image or target");
    int rc;
    Passes ps;
    if ((rc = check_params(params)) || (rc = check_whole_frame("render_to_noise", params, kOneDecides, kProgressive)) ||
        (rc = check_target("render_to_noise", target_of(*target), params->samples, ps)))
        return rc;
    return render_frame(spheres, n_spheres, cam, params, device, ps, target, nullptr, nullptr, image_rgb, nullptr,
                        report, nullptr);
}

int ptg_render_adaptive(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                        int device, const ptg_adaptive_target *target, double *image_rgb, int32_t *sample_counts,
                        ptg_adaptive_report *report)
{
    if (!image_rgb || !target)
        return ptg_frames::fail(PTG_ERR_INVALID_ARGUMENT, "render_adaptive: NULL image or target");
    int rc;
    Passes ps;
    if ((rc = check_params(params)) || (rc = check_whole_frame("render_adaptive", params, kOneDecides, kProgressive)) ||
        (rc = check_target("render_adaptive", target_of(*target), params->samples, ps)))
        return rc;
    return render_frame(spheres, n_spheres, cam, params, device, ps, nullptr, target, nullptr, image_rgb,
                        sample_counts, nullptr, report);
}

int ptg_render_denoised(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                        int device, const ptg_denoise_params *denoise, double *image_rgb)
{
    return render_denoised(spheres, n_spheres, cam, params, device, denoise, nullptr, image_rgb, nullptr);
}

int ptg_render_to_noise_denoised(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                                 const ptg_params *params, int device, const ptg_noise_target *target,
                                 const ptg_denoise_params *denoise, double *image_rgb, ptg_noise_report *report)
{
    if (!target)
        return ptg_frames::fail(PTG_ERR_INVALID_ARGUMENT, "render_to_noise_denoised: NULL target");
    return render_denoised(spheres, n_spheres, cam, params, device, denoise, target, image_rgb, report);
}

int ptg_render_adaptive_denoised(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                                 const ptg_params *params, int device, const ptg_adaptive_target *target,
                                 const ptg_denoise_params *denoise, double *image_rgb, int32_t *sample_counts,
                                 ptg_adaptive_report *report)
{
    const char *const who = "render_adaptive_denoised";
    if (!image_rgb || !params || !cam || !target)
        return ptg_frames::fail(PTG_ERR_INVALID_ARGUMENT,
                                "render_adaptive_denoised: NULL image, camera, params or target");
    if (params->width <= 0 || params->height <= 0)
        return ptg_frames::fail(PTG_ERR_INVALID_ARGUMENT, "width and height must be positive");
    int rc;
    Passes ps;
    ptg_denoise_params k;
    if ((rc = check_whole_frame(who, params, kFilterNeeds, kProgressive)) ||
        (rc = check_target(who, target_of(*target), params->samples, ps)) ||
        (rc = ptg_denoise_params_for_(cam, params->width, params->height, denoise, &k)))
        return rc;
    return render_frame(spheres, n_spheres, cam, params, device, ps, nullptr, target, &k, image_rgb, sample_counts,
                        nullptr, report);
}

}  // extern "C"
