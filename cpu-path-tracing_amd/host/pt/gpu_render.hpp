// pt/gpu_render.hpp -- the drop-in for the reference's row loop
// (src/main.cpp:214-236).  Where main() did
//
//     tf::Executor executor{}; tf::Taskflow taskflow{};
//     for (int y = 0; y < height; y++) taskflow.emplace([...] { ... render_subpixel ... });
//     executor.run(taskflow).wait();
//
// it now calls
//
//     pt::gpu::render_image(some_scene, cam, image, width, height, samps, num_subpixels);
//
// with the same scene, camera, zero-initialised std::vector<pt::vec3> image and
// ints; the image afterwards holds what the loop would leave in it (the same
// estimator, fp32 arithmetic, counter-RNG draws).  Errors surface as a
// negative ptg_status, like the C ABI (the reference has no error channel).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ptgpu.h"
#include "types.hpp"

namespace pt {

static_assert(sizeof(vec3) == 24, "pt::vec3 must be 3 packed doubles");
static_assert(sizeof(sphere) == sizeof(ptg_sphere), "pt::sphere layout != ptg_sphere");
static_assert(offsetof(sphere, position) == offsetof(ptg_sphere, position), "pt::sphere layout");
static_assert(offsetof(sphere, emission) == offsetof(ptg_sphere, emission), "pt::sphere layout");
static_assert(offsetof(sphere, color) == offsetof(ptg_sphere, color), "pt::sphere layout");
static_assert(offsetof(sphere, reflection) == offsetof(ptg_sphere, material), "pt::sphere layout");
static_assert(sizeof(reflection_type) == sizeof(int32_t), "reflection_type must be an int");
static_assert(sizeof(camera) == sizeof(ptg_camera), "pt::camera layout != ptg_camera");
static_assert(offsetof(camera, lens_radius) == offsetof(ptg_camera, lens_radius), "pt::camera layout");

namespace gpu {

inline constexpr std::uint64_t default_seed = 0x5EED0001ull;

// main.cpp:214-236 replacement.  `samps` is per sub-pixel (main.cpp:206).
inline int render_image(scene const &scn, camera const &cam, std::vector<vec3> &image, int width, int height,
                        int samps, int num_subpixels = 2, std::uint64_t seed = default_seed, int device = -1,
                        int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = samps;
    p.num_subpixels = num_subpixels;
    p.seed = seed;
    p.band_rows = 1;  // single-row bands: equal shards whenever shard_count divides H
    p.shard_rank = 0;
    p.shard_count = 1;
    // e.g. PTG_FLAG_EXACT_MATH: bit for bit the CPU oracle's image; PTG_FLAG_LIGHT_SAMPLING, PTG_FLAG_STRATIFIED
    // (fewer samples for the same noise): every entry point of pt::gpu passes them on
    p.flags = flags;
    return ptg_render(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                      reinterpret_cast<ptg_camera const *>(&cam), &p, device,
                      reinterpret_cast<double *>(image.data()));
}

// render_image that stops as soon as the noise target is met (ptg_render_to_noise):
// `samps` is the most it takes; the image equals render_image's at samps =
// report.samples_done.  target: {rel_error, floor, max_fraction, min_samples}.
inline int render_image_to_noise(scene const &scn, camera const &cam, std::vector<vec3> &image, int width, int height,
                                 int samps, ptg_noise_target const &target, ptg_noise_report &report,
                                 int num_subpixels = 2, std::uint64_t seed = default_seed, int device = -1,
                                 int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = samps;
    p.num_subpixels = num_subpixels;
    p.seed = seed;
    p.band_rows = 1;
    p.shard_rank = 0;
    p.shard_count = 1;
    p.flags = flags;
    return ptg_render_to_noise(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                               reinterpret_cast<ptg_camera const *>(&cam), &p, device, &target,
                               reinterpret_cast<double *>(image.data()), &report);
}

// render_image_to_noise whose later passes sample only the pixels still over the
// target or within target.dilate pixels of one (ptg_render_adaptive): a pixel's
// value equals render_image's at samps = its own count.  sample_counts
// (optional) receives width * height counts in the image's row order.
inline int render_image_adaptive(scene const &scn, camera const &cam, std::vector<vec3> &image, int width, int height,
                                 int samps, ptg_adaptive_target const &target, ptg_adaptive_report &report,
                                 std::vector<std::int32_t> *sample_counts = nullptr, int num_subpixels = 2,
                                 std::uint64_t seed = default_seed, int device = -1, int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    if (sample_counts)
        sample_counts->assign(image.size(), 0);
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = samps;
    p.num_subpixels = num_subpixels;
    p.seed = seed;
    p.band_rows = 1;
    p.shard_rank = 0;
    p.shard_count = 1;
    p.flags = flags;
    return ptg_render_adaptive(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                               reinterpret_cast<ptg_camera const *>(&cam), &p, device, &target,
                               reinterpret_cast<double *>(image.data()),
                               sample_counts ? sample_counts->data() : nullptr, &report);
}

// The two above on several GPUs of this process (ptg_render_to_noise_multi /
// ptg_render_adaptive_multi): device k renders the interleaved rows
// r = k mod N, the frame is decided as a whole; image, counts and report equal
// the one-device overloads' bit for bit for any device list.
inline int render_image_to_noise(scene const &scn, camera const &cam, std::vector<vec3> &image, int width, int height,
                                 int samps, ptg_noise_target const &target, ptg_noise_report &report,
                                 std::vector<int> const &devices, int num_subpixels = 2,
                                 std::uint64_t seed = default_seed, int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = samps;
    p.num_subpixels = num_subpixels;
    p.seed = seed;
    p.band_rows = 1;
    p.shard_rank = 0;
    p.shard_count = 1;
    p.flags = flags;
    return ptg_render_to_noise_multi(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                                     reinterpret_cast<ptg_camera const *>(&cam), &p, devices.data(),
                                     static_cast<int>(devices.size()), &target,
                                     reinterpret_cast<double *>(image.data()), &report);
}

inline int render_image_adaptive(scene const &scn, camera const &cam, std::vector<vec3> &image, int width, int height,
                                 int samps, ptg_adaptive_target const &target, ptg_adaptive_report &report,
                                 std::vector<int> const &devices, std::vector<std::int32_t> *sample_counts = nullptr,
                                 int num_subpixels = 2, std::uint64_t seed = default_seed, int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    if (sample_counts)
        sample_counts->assign(image.size(), 0);
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = samps;
    p.num_subpixels = num_subpixels;
    p.seed = seed;
    p.band_rows = 1;
    p.shard_rank = 0;
    p.shard_count = 1;
    p.flags = flags;
    return ptg_render_adaptive_multi(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                                     reinterpret_cast<ptg_camera const *>(&cam), &p, devices.data(),
                                     static_cast<int>(devices.size()), &target,
                                     reinterpret_cast<double *>(image.data()),
                                     sample_counts ? sample_counts->data() : nullptr, &report);
}

// render_image followed by the variance-guided a-trous filter
// (ptg_render_denoised): samps >= 2 per sub-pixel, one device.  denoise
// nullptr: the defaults with the camera's pixel spread; iterations 0 gives
// render_image's image bit for bit.
inline int render_image_denoised(scene const &scn, camera const &cam, std::vector<vec3> &image, int width, int height,
                                 int samps, ptg_denoise_params const *denoise = nullptr, int num_subpixels = 2,
                                 std::uint64_t seed = default_seed, int device = -1, int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = samps;
    p.num_subpixels = num_subpixels;
    p.seed = seed;
    p.band_rows = 1;
    p.shard_rank = 0;
    p.shard_count = 1;
    p.flags = flags;
    return ptg_render_denoised(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                               reinterpret_cast<ptg_camera const *>(&cam), &p, device, denoise,
                               reinterpret_cast<double *>(image.data()));
}

// render_image_to_noise whose frame, at the samples it stopped at, goes through
// the filter (ptg_render_to_noise_denoised; nothing is rendered twice).
inline int render_image_to_noise_denoised(scene const &scn, camera const &cam, std::vector<vec3> &image, int width,
                                          int height, int samps, ptg_noise_target const &target,
                                          ptg_noise_report &report, ptg_denoise_params const *denoise = nullptr,
                                          int num_subpixels = 2, std::uint64_t seed = default_seed, int device = -1,
                                          int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = samps;
    p.num_subpixels = num_subpixels;
    p.seed = seed;
    p.band_rows = 1;
    p.shard_rank = 0;
    p.shard_count = 1;
    p.flags = flags;
    return ptg_render_to_noise_denoised(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                                        reinterpret_cast<ptg_camera const *>(&cam), &p, device, &target, denoise,
                                        reinterpret_cast<double *>(image.data()), &report);
}

namespace detail {
inline ptg_params frame_params(int width, int height, int samps, int num_subpixels, std::uint64_t seed, int flags)
{
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = samps;
    p.num_subpixels = num_subpixels;
    p.seed = seed;
    p.band_rows = 1;
    p.shard_rank = 0;
    p.shard_count = 1;
    p.flags = flags;
    return p;
}
}  // namespace detail

// render_image_adaptive whose frame goes through the filter, guided by the
// variance of each pixel at its own sample count
// (ptg_render_adaptive_denoised); report and counts are render_image_adaptive's.
inline int render_image_adaptive_denoised(scene const &scn, camera const &cam, std::vector<vec3> &image, int width,
                                          int height, int samps, ptg_adaptive_target const &target,
                                          ptg_adaptive_report &report, std::vector<std::int32_t> *sample_counts = nullptr,
                                          ptg_denoise_params const *denoise = nullptr, int num_subpixels = 2,
                                          std::uint64_t seed = default_seed, int device = -1, int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    if (sample_counts)
        sample_counts->assign(image.size(), 0);
    ptg_params const p = detail::frame_params(width, height, samps, num_subpixels, seed, flags);
    return ptg_render_adaptive_denoised(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                                        reinterpret_cast<ptg_camera const *>(&cam), &p, device, &target, denoise,
                                        reinterpret_cast<double *>(image.data()),
                                        sample_counts ? sample_counts->data() : nullptr, &report);
}

// The three denoised drivers on several GPUs of this process
// (ptg_render_denoised_multi / ptg_render_to_noise_denoised_multi /
// ptg_render_adaptive_denoised_multi): the shards' colour and variance slabs
// are gathered on the first device, which filters the frame once; the image
// equals the one-device overloads' bit for bit for any device list.
inline int render_image_denoised(scene const &scn, camera const &cam, std::vector<vec3> &image, int width, int height,
                                 int samps, std::vector<int> const &devices, ptg_denoise_params const *denoise = nullptr,
                                 int num_subpixels = 2, std::uint64_t seed = default_seed, int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    ptg_params const p = detail::frame_params(width, height, samps, num_subpixels, seed, flags);
    return ptg_render_denoised_multi(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                                     reinterpret_cast<ptg_camera const *>(&cam), &p, devices.data(),
                                     static_cast<int>(devices.size()), denoise,
                                     reinterpret_cast<double *>(image.data()));
}

inline int render_image_to_noise_denoised(scene const &scn, camera const &cam, std::vector<vec3> &image, int width,
                                          int height, int samps, ptg_noise_target const &target,
                                          ptg_noise_report &report, std::vector<int> const &devices,
                                          ptg_denoise_params const *denoise = nullptr, int num_subpixels = 2,
                                          std::uint64_t seed = default_seed, int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    ptg_params const p = detail::frame_params(width, height, samps, num_subpixels, seed, flags);
    return ptg_render_to_noise_denoised_multi(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()),
                                              scn.spheres.size(), reinterpret_cast<ptg_camera const *>(&cam), &p,
                                              devices.data(), static_cast<int>(devices.size()), &target, denoise,
                                              reinterpret_cast<double *>(image.data()), &report);
}

inline int render_image_adaptive_denoised(scene const &scn, camera const &cam, std::vector<vec3> &image, int width,
                                          int height, int samps, ptg_adaptive_target const &target,
                                          ptg_adaptive_report &report, std::vector<int> const &devices,
                                          std::vector<std::int32_t> *sample_counts = nullptr,
                                          ptg_denoise_params const *denoise = nullptr, int num_subpixels = 2,
                                          std::uint64_t seed = default_seed, int flags = 0)
{
    if (image.size() != static_cast<std::size_t>(width) * static_cast<std::size_t>(height))
        return PTG_ERR_INVALID_ARGUMENT;
    if (sample_counts)
        sample_counts->assign(image.size(), 0);
    ptg_params const p = detail::frame_params(width, height, samps, num_subpixels, seed, flags);
    return ptg_render_adaptive_denoised_multi(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()),
                                              scn.spheres.size(), reinterpret_cast<ptg_camera const *>(&cam), &p,
                                              devices.data(), static_cast<int>(devices.size()), &target, denoise,
                                              reinterpret_cast<double *>(image.data()),
                                              sample_counts ? sample_counts->data() : nullptr, &report);
}

// The first-hit feature frame (ptg_features): width * height * 12 floats in the
// image's row order, {n.xyz, z}, {P.xyz, hit}, {albedo.rgb, 0} per pixel.
// follow_bounces 1..16: ptg_features_follow, the first diffuse hit behind
// mirrors and glass, the last word the mean number of bounces.  (The denoised
// drivers above take the same choice as denoise->follow_bounces.)
inline int feature_frame(scene const &scn, camera const &cam, std::vector<float> &features, int width, int height,
                         int num_subpixels = 2, int device = -1, int follow_bounces = 0)
{
    features.assign(static_cast<std::size_t>(width) * static_cast<std::size_t>(height) * 12, 0.0f);
    ptg_params p{};
    p.width = width;
    p.height = height;
    p.samples = 1;
    p.num_subpixels = num_subpixels;
    p.seed = default_seed;
    p.band_rows = 1;
    p.shard_rank = 0;
    p.shard_count = 1;
    if (follow_bounces)
        return ptg_features_follow(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                                   reinterpret_cast<ptg_camera const *>(&cam), &p, device, follow_bounces,
                                   features.data());
    return ptg_features(reinterpret_cast<ptg_sphere const *>(scn.spheres.data()), scn.spheres.size(),
                        reinterpret_cast<ptg_camera const *>(&cam), &p, device, features.data());
}

}  // namespace gpu
}  // namespace pt
