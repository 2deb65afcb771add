/*
 * ptgpu.h -- C ABI of the MI355X render loop (libptgpu.so).
 *
 * Drop-in for the per-pixel hot path of AlexandruIca/cpu-path-tracing:
 * the taskflow row loop src/main.cpp:214-236 and everything it calls
 * (render_subpixel main.cpp:179-197, radiance main.cpp:104-158, the scene scan
 * main.cpp:30-42, the BRDF samplers main.cpp:44-97, camera::get_ray
 * camera.cpp:32-38, sphere::intersect sphere.cpp:6-30, get_hit_record_at
 * hit_record.cpp:3-12, rand_state random_state.cpp:3-17) runs as one HIP
 * megakernel on gfx950.  Plain C types only: pointers, sizes, PODs.
 *
 * Conventions (reference: everything noexcept, no error codes):
 *   every entry point returns PTG_OK (0) or a negative ptg_status and never
 *   throws; ptg_last_error() returns a thread-local description of the last
 *   failure.  Calls are not re-entrant on one context.
 */
#ifndef PTGPU_H
#define PTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: flags = 0 now selects the fast arithmetic mode (hardware
 * transcendentals, not reproducible on a CPU); version 1's flags = 0 was the
 * oracle-exact mode, now PTG_FLAG_EXACT_MATH.  Also added since 1:
 * ptg_multi_*, ptg_math_probe_device.  A caller built against 1 that needs
 * the old bit-exact image must pass PTG_FLAG_EXACT_MATH. */
#define PTG_ABI_VERSION 2

typedef enum ptg_status {
    PTG_OK = 0,
    PTG_ERR_INVALID_ARGUMENT = -1,
    PTG_ERR_HIP = -2,
    PTG_ERR_NO_DEVICE = -3,
    PTG_ERR_UNSUPPORTED = -4,
    PTG_ERR_OUT_OF_MEMORY = -5
} ptg_status;

/* reflection.hpp:7-12 */
typedef enum ptg_material { PTG_DIFFUSE = 0, PTG_SPECULAR = 1, PTG_DIELECTRIC = 2 } ptg_material;

/* Field-for-field mirror of pt::sphere (sphere.hpp:10-17): 88 bytes, so a
 * std::vector<pt::sphere>::data() can be passed as-is. */
typedef struct ptg_sphere {
    double radius;
    double position[3];
    double emission[3];
    double color[3];
    int32_t material; /* ptg_material (pt::reflection_type) */
    int32_t reserved_;
} ptg_sphere;

/* Field-for-field mirror of pt::camera (camera.hpp:23-33): 176 bytes, the
 * output of pt::camera::with_config (camera.cpp:3-17). */
typedef struct ptg_camera {
    double position[3];
    double lower_left_corner[3];
    double cam_x_axis[3];
    double cam_y_axis[3];
    double u[3];
    double v[3];
    double w[3];
    double lens_radius;
} ptg_camera;

/* The ints main.cpp:202-206 hands to the loop, plus the counter-RNG seed
 * (replacing std::random_device, random_state.cpp:5), the row-band shard and
 * the work-unit size.
 *
 * Sample accumulation (main.cpp:192 `r = r + c * (1/samps)`, sequential
 * double) is restated order-independently: every path's radiance is
 * quantised to a u64 fixed-point value q(c) = trunc(c * 2^32) (c clamped to
 * [0, 2^30]) and summed exactly; the sub-pixel mean is
 * (float)((double)sum * 2^-32 / samps).  The image therefore does not depend
 * on scheduling, chunking or sharding.
 *
 * The sum of a (pixel, sub-pixel, channel) is exact while samples x the
 * largest clipped component stays below 2^32 (the sum below 2^64).  A
 * component clipped to 2^30 adds 2^62: at most 3 such samples per sum;
 * a fourth wraps the u64 sum and the sub-pixel goes dark with no error.  The
 * same bound holds for the second-moment sums of PTG_FLAG_MOMENTS, whose
 * squares are clipped to 2^30 from components above 2^15.  A caller finds out
 * with PTG_FLAG_COUNT_NONFINITE: a fourth counter of 0 means that no component
 * was clipped (by 0 or by 2^30; exactly 2^30 is in range and not counted). */
typedef struct ptg_params {
    int32_t width;          /* main.cpp:204 */
    int32_t height;         /* main.cpp:205 */
    int32_t samples;        /* per sub-pixel (main.cpp:206: spp / num_subpixels^2) */
    int32_t num_subpixels;  /* per axis (main.cpp:202); 1..8 */
    uint64_t seed;          /* counter RNG key; the image does not depend on sharding */
    int32_t band_rows;      /* shard: output rows per band (>= 1) */
    int32_t shard_rank;     /* this shard renders bands b with b % shard_count == shard_rank */
    int32_t shard_count;    /* 1 = whole image */
    int32_t chunk_samples;  /* samples per sub-pixel per work unit (0 = auto); results do not depend on it */
    int32_t flags;          /* PTG_FLAG_* */
} ptg_params;

/* flags: with PTG_FLAG_COUNT_TESTS, d_segments of ptg_render_device /
 * ptg_accumulate_device points to 3 counters: += scene scans, sphere tests
 * executed (ray-sphere quadratics), and BVH box tests (scenes of > 64
 * spheres) or, of the sphere tests, the box-wall tests (linear scenes) --
 * the inputs of the roofline model.  Linear scenes count each lane's own
 * tests (box mode tests about one wall per segment, not every wall); the
 * survey's model count is scans x spheres. */
#define PTG_FLAG_COUNT_TESTS 1
/* with PTG_FLAG_COUNT_NONFINITE (implies the counters above), d_segments points
 * to 4 counters; the 4th += paths whose radiance has a component that is NaN,
 * negative or above 2^30 -- values the exact accumulation would clip (NaN and
 * negative to 0).  None are expected in the shipped scenes: the -m gpu tests
 * assert 0 there, and the oracle's count on scenes built to be out of range
 * (tests/test_gpu_radiance_range.py). */
#define PTG_FLAG_COUNT_NONFINITE 2
/* PTG_FLAG_REFERENCE_F64: render with the reference's own double-precision
 * arithmetic, operation for operation (src/main.cpp:30-197 and the pt
 * library: linear strict-< scan, (-hb -+ sq)/a roots, correctly rounded
 * sin/cos (csrc/sincos_cr.hpp: glibc's bits on all but 0.15 % of the angles
 * a draw can give), libm-style pow, sequential r += c/samps) instead of the
 * fp32 megakernel --
 * a parity mode (csrc/ref64.hpp), several times slower.  Only the counter-RNG
 * draws differ from the reference (as in every mode).  ptg_render keeps the
 * doubles; ptg_render_device rounds them into its float slab.  Not for
 * progressive passes or trace_samples (PTG_ERR_UNSUPPORTED). */
#define PTG_FLAG_REFERENCE_F64 4
/* PTG_FLAG_EXACT_MATH (ABI 2; the default of ABI 1): the fp32 kernel with deterministic square root,
 * reciprocal square root, division and sin/cos sequences (~1 ulp) that the
 * oracle (oracle/pt_oracle.c, Mode B) executes too -- the image then equals
 * the CPU restatement bit for bit.  Without it (the default) the kernel uses
 * the GPU's own v_sqrt/v_rsq/v_rcp/v_sin/v_cos instructions, about as
 * accurate but not reproducible on a CPU: the image is within the north
 * star's per-pixel RMSE of the reference arithmetic (DESIGN.md "arithmetic
 * modes").  Either way a frame does not depend on sharding, work-unit sizes,
 * progressive passes or the GPU count. */
#define PTG_FLAG_EXACT_MATH 8
/* PTG_FLAG_MOMENTS: a progressive pass (ptg_accumulate_device) also sums the
 * second moment of every path exactly: per (pixel, sub-pixel, channel)
 * S2 += q(cl(c) * cl(c)), cl the clip of q (NaN and negative to 0, above 2^30
 * to 2^30), the product one fp32 multiply -- the input of ptg_noise_device.
 * The image is not affected.  No effect outside ptg_accumulate_device. */
#define PTG_FLAG_MOMENTS 16
/* PTG_FLAG_LIGHT_SAMPLING: next-event estimation for small emissive spheres
 * (smallpt's "explicit" scheme).  Without the flag nothing changes: the same
 * draws, the same images.  Honoured by every entry point that renders
 * (one-shot, progressive with or without PTG_FLAG_MOMENTS, adaptive,
 * render_to_noise, trace_samples, the ptg_multi_* family, and
 * PTG_FLAG_REFERENCE_F64, which runs the same estimator in double).
 *
 * Light list (ptg_light_list): every sphere with an emission component > 0
 * that is not "huge" (radius >= 1000, or plane-like for the camera), any
 * material, in scene index order; at most 16 (more: PTG_ERR_UNSUPPORTED from
 * the entry points given the flag).  With no light the frame equals the frame
 * without the flag bit for bit.
 *
 * At a diffuse hit that continues the path (point p, facing normal nn, T
 * already multiplied by the hit's colour), with L > 0 lights, BEFORE the
 * BRDF's two draws:
 *   1. L > 1: one draw u picks light k = min(L - 1, floor(u L)); L = 1: no draw
 *   2. two draws u1, u2 (always, whatever the geometry)
 *   3. w = C_k - p, d2 = w.w; if d2 > R^2 and the hit sphere is not light k:
 *        q = R^2 / d2, omc = q / (1 + sqrt(1 - q))      (1 - cos theta_max)
 *        a = u1 omc, ct = 1 - a, st = sqrt(a (2 - a)), phi = 2 pi u2
 *        sw = w / |w|, su = norm((|sw.x| > 0.1 ? y : x) x sw), sv = sw x su
 *        l = su cos(phi) st + sv sin(phi) st + sw ct,  cs = nn.l
 *        if cs > 0: a shadow segment, an ordinary nearest-hit scan from p
 *        along l (counted like any scan); if its winner is light k:
 *        E += T * Le_k * (cs 2 omc L)
 *        (the scan's tie rule holds here too: a listed light with a sphere of
 *        equal geometry at a lower scene index is occluded by it everywhere
 *        and adds nothing, as it is never seen without the flag)
 *   4. the path's next hit skips the emission of a sphere on the light list
 *      when it meets that sphere on its FRONT face (that one hit only; also
 *      when step 3 added nothing).  A listed sphere met from inside (back
 *      face) counts: p then lies in or on the inside of that sphere (a dome
 *      light, a lamp of emissive glass), where step 3 adds nothing for it --
 *      and a point outside a sphere can only meet it from the front.  After
 *      a mirror or dielectric bounce and at the camera ray emission counts
 *      as without the flag; huge emitters and the sky always count.
 * In double (PTG_FLAG_REFERENCE_F64, the oracle) the sin and cos of step 3
 * and of the BRDF's direction that follows are, with L > 0, computed in plain
 * double operations (ref64.hpp sincos_plain = the oracle's po_sincos_plain,
 * within 1 ulp of libm's), not by a math library: cs carries the sampled
 * geometry into the path's value, so a library's last bit would show in the
 * image, and the two sides are to agree to the bit.  The fp32 kernels keep
 * their own table.
 * Both estimators are unbiased for the same integral, so their RAW means
 * agree; the image clamps every sub-pixel mean to [0, 1], and the plain
 * estimator's heavier tails are clipped more often -- clamped images of
 * bright scenes (simple_scene) therefore differ slightly in the mean between
 * the two.  Compare estimators on the raw sums (ptg_read_moments_device). */
#define PTG_FLAG_LIGHT_SAMPLING 32
#define PTG_MAX_LIGHTS 16
/* PTG_FLAG_STRATIFIED: stratified sampling.  Four pairs of draws per path
 * come from an Owen-scrambled, index-shuffled Sobol' (0,2)-sequence in the
 * path's sample index s instead of the xorshift stream.  Without the flag
 * nothing changes: the same draws, the same kernels, the same images.
 * Honoured wherever PTG_FLAG_LIGHT_SAMPLING is (every entry point that
 * renders, trace_samples, the ptg_multi_* family, PTG_FLAG_REFERENCE_F64) and
 * combines with it.  A frame still does not depend on sharding, work-unit
 * sizes, progressive passes or the GPU count: a pixel that holds n samples
 * holds samples [0, n), and a (0,2)-sequence is stratified on every
 * power-of-two prefix of that index.
 *
 * The definition (csrc/sobol_pairs.hpp), integer arithmetic on uint32 but for
 * the 64-bit seed mix:
 *   lk(x, seed):  x += seed; x ^= x*0x6c50b47c; x ^= x*0xb82f1e52;
 *                 x ^= x*0xc7afe638; x ^= x*0x8d22f6e6
 *   brev:         32-bit bit reversal
 *   P(i):         for (k, m) in (1,0x55555555),(2,0x33333333),(4,0x0F0F0F0F),
 *                 (8,0x00FF00FF),(16,0x0000FFFF): i ^= (i >> k) & m
 *                 (= brev of the second Sobol' dimension of i, direction
 *                 numbers v = 1<<31; v ^= v>>1 per index bit)
 *   seeds of pair j of a sub-pixel, key = key_hash(seed, pixel_sub) as for
 *   the xorshift stream, mix64 its mixer:
 *                 h = mix64(key ^ (j+1)*0xD1B54A32D192ED03)
 *                 sa = hi32(h), sb = lo32(h), sc = hi32(mix64(h))
 *   pair j, sample s:
 *                 i  = brev(lk(brev(s), sa))       (the shuffled index)
 *                 m0 = brev(lk(i, sb)) >> 8        (van der Corput, scrambled)
 *                 m1 = brev(lk(P(i), sc)) >> 8     (Sobol' dimension 2, scrambled)
 * m0 and m1 are 24-bit integers used exactly where a draw's 24-bit integer
 * is: u = m 2^-24.  Every aligned block of 2^k samples of a pair puts one
 * point in each elementary interval of area 2^-k.
 *
 * Which draws, by pair number:
 *   0. the sub-pixel jitter (main.cpp:186-188)
 *   1. the first try of the lens disk's rejection loop (camera.cpp:19-30);
 *      retries stay xorshift
 *   2. the diffuse sampler's (phi, r) at the camera ray's own hit, when that
 *      hit is diffuse
 *   3. with PTG_FLAG_LIGHT_SAMPLING, that same hit's (u1, u2) of step 2 of the
 *      light-sampling step; the light choice of step 1 stays xorshift
 * Every other draw is xorshift from sample_state(key, s) as without the flag,
 * and a replaced draw does not advance the xorshift state.  A first hit on a
 * mirror or glass gets no stratified bounce.
 *
 * ptg_noise_device and the adaptive selection assume independent samples, so
 * with the flag they overstate the error: noise-target and adaptive frames
 * stop later rather than earlier, and no image is wrong. */
#define PTG_FLAG_STRATIFIED 64

typedef struct ptg_context ptg_context;

/* ---- metadata -------------------------------------------------------- */
int ptg_abi_version(void);
const char *ptg_last_error(void);
int ptg_device_count(int *count);

/* ---- drop-in entry point ---------------------------------------------
 * Replaces main.cpp:214-236.  Synchronous.  image_rgb is the caller-owned
 * std::vector<pt::vec3> viewed as width*height*3 doubles in the reference's
 * row order (row (H-1-y)*W + x, main.cpp:181); like the loop, the call ADDS
 * sum_sub clamp(mean)/num_subpixels^2 (main.cpp:195-196) into it.  With
 * shard_count > 1 only the shard's bands are added.  device = -1: current. */
int ptg_render(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
               const ptg_params *params, int device, double *image_rgb);

/* ---- single-process multi-GPU drop-in ---------------
 * The same contract as ptg_render (params->shard_count must be 1: the call
 * shards the frame itself), rendered on n_devices distinct GPUs of this
 * process: device k renders the interleaved row bands b with
 * b % n_devices == k (band_rows from params), ONE ncclGather (RCCL over xGMI,
 * rccl.h:745) collects the slabs on devices[0], which un-shards the frame.
 * The image equals ptg_render's bit for bit (the RNG is keyed by the global
 * pixel).  Replaces main.cpp:214-236 for a caller owning several GPUs.
 * fp32 kernel only: PTG_FLAG_REFERENCE_F64 is refused (PTG_ERR_UNSUPPORTED;
 * ptg_render keeps that mode's doubles).  The caller's current HIP device is
 * restored on return.  ptg_render_multi = ptg_multi_create + ptg_multi_render
 * + ptg_multi_destroy. */
int ptg_render_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                     const ptg_params *params, const int *devices, int n_devices, double *image_rgb);

/* A persistent multi-GPU context: per device the scene in HBM, a stream and
 * the slab, the RCCL communicator of the device set (ncclCommInitAll once),
 * the root's gather buffer and image -- repeated and progressive frames
 * reuse them.  Not re-entrant. */
typedef struct ptg_multi ptg_multi;
int ptg_multi_create(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const int *devices,
                     int n_devices, ptg_multi **out);
int ptg_multi_destroy(ptg_multi *m);
/* ptg_render_multi's frame on the context (synchronous; adds into image_rgb
 * like main.cpp:196). */
int ptg_multi_render(ptg_multi *m, const ptg_params *params, double *image_rgb);
/* Progressive passes over all devices (README.md:9): reset, then sample
 * passes [begin, end) queued on every device (asynchronous), then a resolve
 * of the samples so far -- each device resolves its bands, ONE gather, the
 * un-shard -- written (not added) to image_rgb as W*H*3 floats in the
 * reference's row order (synchronous).  After passes covering [0, samples)
 * the resolve equals ptg_render's image bit for bit. */
int ptg_multi_reset_accumulation(ptg_multi *m, const ptg_params *params);
int ptg_multi_accumulate(ptg_multi *m, const ptg_params *params, int32_t sample_begin, int32_t sample_end);
int ptg_multi_resolve(ptg_multi *m, const ptg_params *params, int32_t samples_done, float *image_rgb);
/* The frame kept in HBM (the benchmark step over several GPUs): every device
 * renders its bands, ONE gather, the un-shard into the root's image buffer;
 * returns when all devices are done, with no host copy of the image.  With
 * PTG_FLAG_COUNT_TESTS in params->flags, counters (optional, host, 4 values)
 * receives the counters of ptg_render_device summed over the devices.
 * ptg_multi_frame_timing then gives, from HIP events of that frame, each
 * device's render time (render_ms[n_devices]) and the root's time from the
 * start of its render to the end of the un-shard (frame_ms);
 * ptg_multi_image copies the frame (W*H*3 floats, reference row order) to the
 * host.  After a failure inside the RCCL group the communicators are aborted
 * (no partial collective runs) and every later frame call returns
 * PTG_ERR_HIP; destroy the context. */
int ptg_multi_frame_device(ptg_multi *m, const ptg_params *params, unsigned long long *counters);
int ptg_multi_frame_timing(const ptg_multi *m, float *render_ms, int n_devices, float *frame_ms);
/* The last ptg_multi_frame_device frame only: params must have the frame's
 * width, height and band_rows (PTG_ERR_INVALID_ARGUMENT otherwise, and after
 * any other frame call on the context). */
int ptg_multi_image(ptg_multi *m, const ptg_params *params, float *image_rgb);
/* What the context's RCCL group actually is (the proof behind a multi-GPU
 * measurement): per shard k, ranks[k] = ncclCommCount of its communicator
 * (0: no communicator -- local shards gathered by device copies, or an
 * aborted group), comm_devices[k] = the HIP device its communicator runs on
 * (ncclCommCuDevice; the shard's device for local shards), user_ranks[k] =
 * ncclCommUserRank (-1 without a communicator).  n_devices must equal the
 * context's shard count. */
int ptg_multi_comm_info(const ptg_multi *m, int32_t *ranks, int32_t *comm_devices, int32_t *user_ranks,
                        int n_devices);
/* PCI bus id of a HIP device ("dddd:bb:dd.f", hipDeviceGetPCIBusId) into
 * buf (len >= 16 recommended).  Distinct devices of a node have distinct ids. */
int ptg_device_pci_bus_id(int device, char *buf, int len);

/* ---- device-resident path (bench, multi-GPU) --------------------------
 * A context holds the prepared scene in HBM on one device. */
int ptg_context_create(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int device,
                       ptg_context **out);
int ptg_context_destroy(ptg_context *ctx);

/* How ptg_render_device would launch this frame (host-side, nothing is
 * launched): info[0] box mode on (the linear scan's nearest-wall-first rule;
 * the fast mode turns it off when a ray could start inside a wall),
 * [1] box_walls_out (no ray can start inside a box wall: the fast mode's
 * outside-only wall roots apply), [2] BVH scan (> 64 spheres), [3] work units,
 * [4] workgroups, [5] unit levels, [6] an HBM accumulator + resolve pass,
 * [7] wall-pair mask (x 1, y 2, z 4).  n_info <= PTG_LAUNCH_INFO_COUNT values
 * are written (extra entries 0). */
#define PTG_LAUNCH_INFO_COUNT 8
int ptg_launch_info(ptg_context *ctx, const ptg_params *params, int64_t *info, int n_info);

/* Rows in one shard's slab: ceil(bands / shard_count) * band_rows. */
int ptg_shard_rows(int32_t height, int32_t band_rows, int32_t shard_count, int32_t *rows);

/* Asynchronous render on `stream` (hipStream_t; NULL = default stream).
 * d_slab: device buffer of ptg_shard_rows(...) * width * 3 floats; slab row j
 * holds output row ((j / band_rows) * shard_count + shard_rank) * band_rows +
 * j % band_rows (rows >= height are left untouched).  Pixel values are
 * written (not accumulated).  d_segments: optional device uint64 that
 * receives += the number of scene scans (radiance segments) executed. */
int ptg_render_device(ptg_context *ctx, const ptg_params *params, float *d_slab,
                      unsigned long long *d_segments, void *stream);

/* ---- progressive accumulation (README.md:9 "make the rendering process
 * progressive") ----------------------------------------
 * Sample passes add exact per-sub-pixel sums into the context's accumulator;
 * a resolve turns the sums so far into an image (clamped means over
 * samples_done samples) without consuming them.  After passes that together
 * cover samples [0, params->samples), ptg_resolve_device(..., samples, ...)
 * equals ptg_render_device bit for bit.  Reset before a new frame.
 * After ptg_accumulate_active_device passes ("adaptive sampling" below) the
 * pixels hold different sample counts: ptg_accumulate_device,
 * ptg_resolve_device and ptg_noise_device then return
 * PTG_ERR_INVALID_ARGUMENT until the next reset. */
int ptg_reset_accumulation_device(ptg_context *ctx, const ptg_params *params, void *stream);
int ptg_accumulate_device(ptg_context *ctx, const ptg_params *params, int32_t sample_begin, int32_t sample_end,
                          unsigned long long *d_segments, void *stream);
int ptg_resolve_device(ptg_context *ctx, const ptg_params *params, int32_t samples_done, float *d_slab,
                       void *stream);

/* ---- per-pixel noise estimates (DESIGN.md "noise estimates") ----------
 * Passes with PTG_FLAG_MOMENTS keep, beside the exact sums S1 of q(c), the
 * exact sums S2 of q(cl(c)^2) in a second accumulator the context owns
 * (allocated on first use, cleared by ptg_reset_accumulation_device).  After
 * n = samples_done >= 2 samples, all in double and in (sy, sx) order:
 *   m1 = S1 2^-32 / n, m2 = S2 2^-32 / n,
 *   v = max(0, m2 - m1 m1) / (n - 1)          variance of the sub-pixel mean
 *   V_c = inv_sub2^2 sum_sub min(v, 1/4)      inv_sub2 = (float)1 / nsub^2; the
 *        image clamps every sub-pixel mean to [0, 1], whose variance is at
 *        most 1/4
 *   p_c = the pixel value of ptg_resolve_device
 *   rho = (float)(sqrt((V_r + V_g + V_b) / 3) / max((p_r + p_g + p_b) / 3, floor))
 * d_var (slab_rows * width * 3 floats: (float)V_c), d_rho (slab_rows * width
 * floats: the relative standard error rho) and d_stats are each optional;
 * slab rows past the image are left untouched.  d_stats: 4 uint64 the caller
 * zeroes, [0] += pixels with rho > rel_error, [1] += trunc(min(rho, 4096) *
 * 2^20), [2] = max(the bits of rho), [3] += pixels visited -- integers, so
 * deterministic, and the stats of shards add (max for [2]).
 * PTG_ERR_INVALID_ARGUMENT when samples_done < 2 or > samples, floor <= 0,
 * rel_error < 0, no PTG_FLAG_MOMENTS pass has run since the last reset, or a
 * pass since the last reset ran without the flag.  Asynchronous on stream. */
int ptg_noise_device(ptg_context *ctx, const ptg_params *params, int32_t samples_done, double rel_error,
                     double floor, float *d_var, float *d_rho, unsigned long long *d_stats, void *stream);

/* The raw sums of the slab, copied to d_sum (S1) and d_sumsq (S2), each
 * optional: slab_rows * width * num_subpixels^2 * 3 uint64, index
 * ((slab_row * width + x) * num_subpixels^2 + sy * num_subpixels + sx) * 3 + c.
 * Sums of frames with different seeds may be added by the caller.  d_sumsq
 * under the conditions of ptg_noise_device.  Asynchronous on stream. */
int ptg_read_moments_device(ptg_context *ctx, const ptg_params *params, unsigned long long *d_sum,
                            unsigned long long *d_sumsq, void *stream);

/* Host only: the pass ends of a render-until-converged frame: min_samples,
 * 2 min_samples, 4 min_samples, ... below samples, then samples (so the last
 * entry is samples; min_samples > samples gives the one entry samples).
 * min_samples >= 2, samples >= 2.  *n receives the count; cap is the room in
 * ends (PTG_ERR_INVALID_ARGUMENT when too small; PTG_NOISE_MAX_PASSES always
 * suffices). */
#define PTG_NOISE_MAX_PASSES 32
int ptg_noise_schedule(int32_t min_samples, int32_t samples, int32_t *ends, int32_t cap, int32_t *n);

typedef struct ptg_noise_target {
    double rel_error;    /* a pixel is over the target when rho > rel_error (>= 0) */
    double floor;        /* rho's denominator is max(pixel mean, floor) (> 0) */
    double max_fraction; /* stop when at most this fraction of the pixels is over; in [0, 1) */
    int32_t min_samples; /* first check after this many samples per sub-pixel (>= 2) */
    int32_t reserved_;
} ptg_noise_target;

typedef struct ptg_noise_report {
    int32_t samples_done; /* samples per sub-pixel in the image */
    int32_t passes;
    int32_t converged;    /* the last check met the target */
    int32_t reserved_;
    uint64_t pixels;
    uint64_t pixels_over; /* of the last check */
    double max_rho, mean_rho; /* of the last check; the mean is of min(rho, 4096) in 2^-20 steps */
    int32_t pass_samples[PTG_NOISE_MAX_PASSES];  /* samples done after pass k */
    uint64_t pass_over[PTG_NOISE_MAX_PASSES];    /* pixels over the target after pass k */
} ptg_noise_report;

/* Render until the noise target is met, at most params->samples samples per
 * sub-pixel.  Synchronous; params->shard_count must be 1.  Resets, then runs
 * the passes of ptg_noise_schedule(target->min_samples, params->samples) with
 * PTG_FLAG_MOMENTS; after each pass one ptg_noise_device check (stats only,
 * 32 bytes copied back); stops when pixels over <= max_fraction * pixels.
 * Then resolves and ADDS into image_rgb like the drop-in entry point: sample
 * draws do not depend on params->samples, so the image equals that entry
 * point's at samples = report->samples_done bit for bit.  report is optional. */
int ptg_render_to_noise(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                        const ptg_params *params, int device, const ptg_noise_target *target, double *image_rgb,
                        ptg_noise_report *report);

/* ---- adaptive sampling (DESIGN.md "adaptive sampling") ------------------
 * Later passes only for the pixels still noisy.  The context keeps, beside
 * the two accumulators, an int32 sample count n_p per slab pixel (allocated on
 * first use, zeroed by ptg_reset_accumulation_device) and an active list.
 * The guarantee: after any sequence of the calls below, pixel p holds exactly
 * samples [0, n_p) of each of its sub-pixels -- S1 and S2 are the sums over
 * those samples, and its resolved value equals ptg_render_device's at
 * samples = n_p bit for bit, whatever the chunking, the sharding (dilate 0)
 * or the grouping of the active pixels into work units.
 * All asynchronous on stream; slabs in slab-row order, like d_rho.  While
 * adaptive passes are in the sums (until the next reset),
 * ptg_accumulate_device, ptg_resolve_device and ptg_noise_device return
 * PTG_ERR_INVALID_ARGUMENT (their one n no longer describes the sums), and
 * the entry points below do after a ptg_accumulate_device pass;
 * ptg_read_moments_device keeps working (adaptive passes always sum both
 * moments; PTG_FLAG_MOMENTS is not needed).
 *
 * ptg_set_active_mask_device: the active list from a byte mask (also the
 * region-of-interest entry point): pixel (slab_row, x) is active when
 * d_mask[slab_row * width + x] != 0; d_mask NULL: every pixel of the image.
 * d_info (optional) receives 2 values: active pixels, active work units (a
 * slab row's active pixels in ascending x, cut into units of 64 /
 * num_subpixels^2 pixels; units never span rows).
 *
 * ptg_select_active_device: rho as ptg_noise_device defines it, with each
 * pixel's own n_p in place of samples_done (n_p < 2: rho = +inf).  A pixel is
 * over when rho > rel_error, and active when some pixel of its
 * (2 dilate + 1)^2 window, clipped to the image, is over.  dilate in [0, 8];
 * dilate > 0 with shard_count > 1 is PTG_ERR_UNSUPPORTED (the neighbouring
 * rows live in other shards).  d_rho optional.  d_stats (optional): 6 uint64
 * the caller zeroes, [0]..[3] as ptg_noise_device's (so [0] counts the pixels
 * over, not the pixels active), [4] += active pixels, [5] += active units.
 * floor > 0 and rel_error >= 0, as there.
 *
 * ptg_accumulate_active_device: every pixel of the active list receives its
 * next add_samples samples [n_p, n_p + add_samples), summed into S1 and S2,
 * and its count rises by add_samples.  max_units <= 0: the launch is sized
 * for the most units the slab can hold; a caller that read the unit count
 * back ([5] or d_info[1]) passes it, and a sparse list launches a small grid
 * (the kernel takes the true count from the device; units past max_units are
 * left out of the pass, neither sampled nor counted).  An empty list does no
 * work and is not an error.  PTG_ERR_INVALID_ARGUMENT when add_samples < 0,
 * without an active list since the last reset, with a list built for another
 * frame geometry, or when the adds since the last reset would pass 2^30.
 * d_segments as ptg_accumulate_device's.
 *
 * ptg_resolve_active_device: ptg_resolve_device's arithmetic with each
 * pixel's own n_p (n_p = 0: 0); the sums are kept.
 * ptg_read_sample_counts_device: the counts, slab_rows * width int32. */
int ptg_set_active_mask_device(ptg_context *ctx, const ptg_params *params, const uint8_t *d_mask,
                               unsigned long long *d_info, void *stream);
int ptg_select_active_device(ptg_context *ctx, const ptg_params *params, double rel_error, double floor,
                             int32_t dilate, float *d_rho, unsigned long long *d_stats, void *stream);
int ptg_accumulate_active_device(ptg_context *ctx, const ptg_params *params, int32_t add_samples, long long max_units,
                                 unsigned long long *d_segments, void *stream);
int ptg_resolve_active_device(ptg_context *ctx, const ptg_params *params, float *d_slab, void *stream);
int ptg_read_sample_counts_device(ptg_context *ctx, const ptg_params *params, int32_t *d_counts, void *stream);

/* The selection in two steps, for a frame sharded over several contexts
 * (ptg_multi_select_active; one rank per GPU would all-gather between them):
 *
 * ptg_select_over_device: step 1 of ptg_select_active_device on its own: the
 * shard's over bytes to d_over (slab_rows * width bytes, 1 where rho >
 * rel_error, 0 in slab rows past the image), rho to d_rho (optional),
 * d_stats[0..3] (optional, 6 uint64 the caller zeroes; [4] and [5] are left to
 * the second step).  No list is built.  Arguments and state rules as
 * ptg_select_active_device's.
 *
 * ptg_set_active_gathered_device: this shard's active list from the over
 * bytes of the WHOLE frame: d_over_gathered holds shard_count slabs of
 * slab_rows * width bytes, rank-major, as all-gather lays them out
 * (ptg_unshard_device's convention): the pixel (r, x) of the image lives in
 * slab (r / band_rows) % shard_count, at slab row (r / band_rows /
 * shard_count) * band_rows + r % band_rows.  A pixel of this shard is active
 * when some byte of its (2 dilate + 1)^2 window, clipped to the image, is set
 * -- the rows of the window are read from the slabs they live in, so any
 * shard_count is accepted with dilate in [0, 8]; slab rows past the image are
 * never read.  d_stats (optional): [4] += active pixels, [5] += active units.
 * With shard_count 1 the list equals ptg_select_active_device's. */
int ptg_select_over_device(ptg_context *ctx, const ptg_params *params, double rel_error, double floor,
                           uint8_t *d_over, float *d_rho, unsigned long long *d_stats, void *stream);
int ptg_set_active_gathered_device(ptg_context *ctx, const ptg_params *params, const uint8_t *d_over_gathered,
                                   int32_t dilate, unsigned long long *d_stats, void *stream);

typedef struct ptg_adaptive_target {
    double rel_error;    /* a pixel is over the target when rho > rel_error (>= 0) */
    double floor;        /* rho's denominator is max(pixel mean, floor) (> 0) */
    double max_fraction; /* stop when at most this fraction of the pixels is over; in [0, 1) */
    int32_t min_samples; /* every pixel gets this many samples per sub-pixel before the first check (>= 2) */
    int32_t dilate;      /* a pixel stays active while a pixel of its (2 dilate + 1)^2 window is over; 0..8 */
} ptg_adaptive_target;

typedef struct ptg_adaptive_report {
    int32_t passes;
    int32_t converged;    /* the last check met the target */
    int32_t max_samples;  /* the largest sample count per sub-pixel: the last pass's end */
    int32_t reserved_;
    uint64_t pixels;
    uint64_t pixels_over; /* of the last check */
    double max_rho, mean_rho; /* of the last check, as ptg_noise_report's (+inf counts as 4096 in the mean) */
    uint64_t total_samples;   /* sum over the pixels of n_p (samples per sub-pixel) */
    uint64_t counters[4];     /* ptg_render_device's d_segments counters, with PTG_FLAG_COUNT_TESTS (else 0) */
    int32_t pass_added[PTG_NOISE_MAX_PASSES];   /* samples pass k added to each of its active pixels */
    uint64_t pass_over[PTG_NOISE_MAX_PASSES];   /* pixels over the target after pass k */
    uint64_t pass_active[PTG_NOISE_MAX_PASSES]; /* pixels active after pass k (over, dilated) */
} ptg_adaptive_report;

/* ptg_render_to_noise with adaptive passes.  Synchronous; shard_count must be
 * 1.  With e_0 < e_1 < ... the ends of ptg_noise_schedule(target->min_samples,
 * params->samples): pass 0 gives every pixel e_0 samples; after each pass one
 * ptg_select_active_device (48 bytes copied back); it stops when pixels over
 * <= max_fraction * pixels or at the last end; otherwise the active pixels
 * get e_(k+1) - e_k more samples.  Then resolves and ADDS into image_rgb like
 * the drop-in entry point; a pixel's value equals that entry point's at
 * samples = its count bit for bit.  sample_counts (optional): width * height
 * int32 in the reference's row order; report optional. */
int ptg_render_adaptive(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                        const ptg_params *params, int device, const ptg_adaptive_target *target, double *image_rgb,
                        int32_t *sample_counts, ptg_adaptive_report *report);

/* ---- noise-target and adaptive frames on several GPUs ------------------
 * The entry points above on a ptg_multi (params->shard_count must be 1: the
 * context shards the frame itself; PTG_FLAG_REFERENCE_F64 is
 * PTG_ERR_UNSUPPORTED; the caller's current HIP device is restored on
 * return).  Sums are exact, the statistics are integers that add across the
 * shards ([2]: max) and the RNG is keyed by the global pixel, so for any
 * device count, band_rows and dilate the image, the per-pixel sample counts,
 * every report field and the kernel counters equal the one-device entry
 * point's bit for bit.  The shards work concurrently on their own streams;
 * each check synchronises with the host once, to read 48 bytes per shard.
 * The contexts' state rules carry over: ptg_multi_accumulate /
 * ptg_multi_resolve / ptg_multi_noise refuse while adaptive passes are in the
 * sums, and the *_active entry points after a ptg_multi_accumulate pass,
 * until ptg_multi_reset_accumulation.
 *
 * ptg_multi_noise: ptg_noise_device's four statistics (host, required) of
 * the whole frame after ptg_multi_accumulate passes with PTG_FLAG_MOMENTS.
 * ptg_multi_set_active_mask: the active list from a host byte mask of
 * width * height bytes in the image's row order (NULL: every pixel); each
 * shard receives its rows.  The region-of-interest entry point.
 * ptg_multi_select_active: ptg_select_active_device for the frame: every
 * shard's ptg_select_over_device, ONE all-gather of the over bytes onto every
 * device (RCCL: one ncclAllGather per rank inside one group; a failure there
 * aborts the communicators as the frame gather's does), every shard's
 * ptg_set_active_gathered_device.  stats (host, optional): the six of
 * ptg_select_active_device for the frame.  Each shard's own unit count sizes
 * its next ptg_multi_accumulate_active pass.
 * ptg_multi_accumulate_active: the next add_samples samples of every active
 * pixel (asynchronous).  ptg_multi_resolve_active: each pixel averaged over
 * its own count, W*H*3 floats written like ptg_multi_resolve.
 * ptg_multi_read_sample_counts: width * height int32 in the image's row order. */
int ptg_multi_noise(ptg_multi *m, const ptg_params *params, int32_t samples_done, double rel_error, double floor,
                    unsigned long long *stats);
int ptg_multi_set_active_mask(ptg_multi *m, const ptg_params *params, const uint8_t *mask);
int ptg_multi_select_active(ptg_multi *m, const ptg_params *params, double rel_error, double floor, int32_t dilate,
                            unsigned long long *stats);
int ptg_multi_accumulate_active(ptg_multi *m, const ptg_params *params, int32_t add_samples);
int ptg_multi_resolve_active(ptg_multi *m, const ptg_params *params, float *image_rgb);
int ptg_multi_read_sample_counts(ptg_multi *m, const ptg_params *params, int32_t *counts);
/* ptg_render_to_noise / ptg_render_adaptive on the context: the same
 * schedule, stop rule and report, the frame decided as a whole; both ADD into
 * image_rgb like the drop-in entry point.  ptg_render_to_noise_multi /
 * ptg_render_adaptive_multi = ptg_multi_create + the call + ptg_multi_destroy
 * on n_devices distinct GPUs, as ptg_render_multi. */
int ptg_multi_render_to_noise(ptg_multi *m, const ptg_params *params, const ptg_noise_target *target,
                              double *image_rgb, ptg_noise_report *report);
int ptg_multi_render_adaptive(ptg_multi *m, const ptg_params *params, const ptg_adaptive_target *target,
                              double *image_rgb, int32_t *sample_counts, ptg_adaptive_report *report);
int ptg_render_to_noise_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                              const ptg_params *params, const int *devices, int n_devices,
                              const ptg_noise_target *target, double *image_rgb, ptg_noise_report *report);
int ptg_render_adaptive_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                              const ptg_params *params, const int *devices, int n_devices,
                              const ptg_adaptive_target *target, double *image_rgb, int32_t *sample_counts,
                              ptg_adaptive_report *report);

/* ---- denoising (DESIGN.md "Denoising") --------------------------------
 * An edge-avoiding a-trous filter over a frame, guided by first-hit features
 * and by the per-pixel variance of ptg_noise_device.  Additive: no draw, image
 * or plan of the entry points above changes.
 *
 * ptg_features_device: 12 floats per slab pixel, in ptg_render_device's slab
 * layout (slab rows past the image are left untouched): {n.xyz, z},
 * {P.xyz, hit}, {albedo.rgb, 0}.  Each of the pixel's num_subpixels^2
 * sub-pixels sends ONE deterministic camera ray -- the renderer's camera ray
 * with both jitter draws 0.5 and no lens offset -- through the renderer's own
 * nearest-hit scan in its exact arithmetic.  Per hitting ray: the facing
 * normal n, the point P = o + t d, the distance z = t |d| and the sphere's
 * colour; hit is the fraction of the rays that hit a sphere, the others are
 * means over the hitting rays (n is not re-normalised), 0 when none hits
 * except the albedo, which is (1, 1, 1) for the sky.  No RNG: the result does
 * not depend on seed, samples or flags.  d_feat must be 16-byte aligned
 * (PTG_ERR_INVALID_ARGUMENT otherwise).  Asynchronous on stream. */
int ptg_features_device(ptg_context *ctx, const ptg_params *params, float *d_feat, void *stream);

/* The same slab (layout, alignment rule, shard handling, rows past the image
 * untouched, the frame planned as an exact-mode frame), with each ray followed
 * through mirrors and glass to the first diffuse surface.  A mirror's fuzz draw
 * is multiplied by 0 and a refraction direction is deterministic, so no draw is
 * taken.  max_bounces is 0..PTG_MAX_FOLLOW_BOUNCES (PTG_ERR_INVALID_ARGUMENT
 * outside).  Per ray, with T = (1, 1, 1), b = 0 and the pixel's running z:
 *   scan (the renderer's exact scan): a miss makes the ray sky whatever b is,
 *     and it adds nothing to any sum; a hit at t gives p = fma(d, t, o), the
 *     outward normal on, front = on.d < 0 and the facing normal nn as the
 *     exact shading forms them, and z' = fma(t, sqrt(d.d), z') for every
 *     segment of the ray, starting from the pixel's z (a ray that ends in the
 *     sky leaves the pixel's z as it was);
 *   stop when the sphere is diffuse or b == max_bounces: n += nn, P += p,
 *     albedo += T * colour, bounce sum += b, hits += 1 (a ray out of bounces
 *     on a mirror reports that mirror);
 *   else follow: T = T * colour, o = p, b += 1, and d by the exact shading's
 *     arithmetic -- specular: d - 2 (on.d) on; dielectric: v1 = d rsqrt(d.d),
 *     cth = min(1, -v1.nn), s2 = sqrt0(1 - cth^2), ratio = front ? 0.5 : 2; with
 *     ratio s2 > 1 (total internal reflection) the mirror formula, else
 *     perp = (nn cth + v1) ratio, d = perp - nn sqrt(|1 - perp.perp|).  There is
 *     no Fresnel reflection branch.  Directions stay un-normalised where the
 *     renderer leaves them so.
 * Per pixel the 12 floats keep their places: means over the stopping rays,
 * hit their share of the rays, albedo (1, 1, 1) for a sky pixel, and word 11
 * (0 in ptg_features_device) the mean b of the stopping rays;
 * ptg_denoise_device does not read word 11.  With max_bounces = 0 the slab
 * equals ptg_features_device's bit for bit. */
#define PTG_MAX_FOLLOW_BOUNCES 16
int ptg_features_follow_device(ptg_context *ctx, const ptg_params *params, int32_t max_bounces, float *d_feat,
                               void *stream);

typedef struct ptg_denoise_params {
    int32_t iterations;  /* 0..8 (0 copies the input); iteration i has step 1 << i */
    int32_t follow_bounces;  /* the drivers' guide: 0 ptg_features_device, 1..16 ptg_features_follow_device */
    float k_color;       /* weight of |c_p - c_q|^2 / (Vbar_p + Vbar_q + eps_color) */
    float k_normal;      /* weight of max(0, 1 - n_p.n_q), and of |hit_p - hit_q| */
    float k_plane;       /* weight of |n_p.(P_q - P_p)| / (step pixel_spread max(z_p, 1e-4)) */
    float k_albedo;      /* weight of |a_p - a_q|^2 */
    float eps_color;     /* > 0 */
    float pixel_spread;  /* world size of a pixel at distance 1 (ptg_pixel_spread); > 0 */
    float reserved_[8];
} ptg_denoise_params;

/* The defaults (host only).  pixel_spread is 1/1024, a 53 degree field of
 * view 1024 pixels across: callers with a camera set it from ptg_pixel_spread. */
int ptg_denoise_defaults(ptg_denoise_params *out);
/* Host only: max(|X| / width, |Y| / height) / |base + X/2 + Y/2| of the
 * camera's image plane (X, Y its axes, base its lower left corner less the
 * position): what one pixel spans at distance 1 along the central ray. */
int ptg_pixel_spread(const ptg_camera *cam, int32_t width, int32_t height, float *spread);
/* Host only: the scratch ptg_denoise_device needs for a width x height frame. */
int ptg_denoise_scratch_bytes(int32_t width, int32_t height, size_t *bytes);

/* The filter, all fp32 in a fixed operation order with explicit fmaf and
 * correctly rounded division (csrc/denoise_filter.hpp), so ptg_denoise_host
 * reproduces every bit on a CPU.  Whole frames with row stride width (a
 * shard_count = 1 slab, or a gathered frame): d_color, d_var, d_out, d_var_out
 * (optional) width * height * 3 floats, d_feat width * height * 12.  The
 * outputs must not overlap the inputs.
 *   before iteration i: Vbar_p = the 3x3 [1 2 1]x[1 2 1]/16 average of
 *     V_r + V_g + V_b, coordinates clamped to the image, of the input
 *     variance (i = 0) or of the previous iteration's output variance
 *   iteration i, s = 1 << i, taps q = p + s (dx, dy), dx, dy in -2..2, inside
 *   the image, h = [1/16, 1/4, 3/8, 1/4, 1/16]:
 *     x = k_color |c_p - c_q|^2 / (Vbar_p + Vbar_q + eps_color)
 *       + k_normal max(0, 1 - n_p.n_q)
 *       + k_plane |n_p.(P_q - P_p)| / (s pixel_spread max(z_p, 1e-4))
 *       + k_albedo |a_p - a_q|^2
 *       + (hit_p == hit_q ? 0 : k_normal |hit_p - hit_q|)
 *     with hit_p = 0 or hit_q = 0 (sky): the colour term alone when both are
 *     0, else the tap is skipped
 *     t = max(0, 1 - x / 8), w = h(dx) h(dy) t^8 (three squarings): a tap
 *     with x >= 8 contributes exactly 0
 *     c'_p = sum w c_q / sum w, V'_p = sum w^2 V_q / (sum w)^2 per channel
 *     (the centre tap is taken at x = 0 -- a mean normal may be shorter
 *     than 1 -- so sum w >= 9/64)
 *   after the last iteration d_out = c', d_var_out = V'.
 * Asynchronous on stream, no allocation inside: d_scratch of at least
 * ptg_denoise_scratch_bytes.  PTG_ERR_INVALID_ARGUMENT for a NULL buffer,
 * iterations outside 0..8, eps_color or pixel_spread <= 0, a negative or
 * non-finite k, or too small a scratch. */
int ptg_denoise_device(const float *d_color, const float *d_var, const float *d_feat, int32_t width, int32_t height,
                       const ptg_denoise_params *params, float *d_out, float *d_var_out, void *d_scratch,
                       size_t scratch_bytes, void *stream);
/* The same arithmetic as a host loop over host buffers (no device, no
 * scratch): the filter's CPU statement, what the tests compare the kernels
 * with.  Synchronous. */
int ptg_denoise_host(const float *color, const float *var, const float *feat, int32_t width, int32_t height,
                     const ptg_denoise_params *params, float *out, float *var_out);

/* Render and denoise.  Synchronous; params->shard_count must be 1 and
 * params->samples >= 2.  Reset, ONE PTG_FLAG_MOMENTS pass over
 * [0, samples), resolve, ptg_noise_device for the variance slab,
 * ptg_features_device, ptg_denoise_device; then ADDS into image_rgb in
 * ptg_render's row order.  denoise NULL: the defaults with the camera's
 * pixel_spread (also taken from the camera when the given one is 0).
 * denoise->follow_bounces, here and in every driver below (the ptg_multi
 * ones included): 0 takes ptg_features_device, 1..16
 * ptg_features_follow_device with that max_bounces, anything else is
 * PTG_ERR_INVALID_ARGUMENT; ptg_denoise_device and ptg_denoise_host ignore it.
 * PTG_FLAG_EXACT_MATH and PTG_FLAG_LIGHT_SAMPLING are honoured;
 * PTG_FLAG_REFERENCE_F64 is PTG_ERR_UNSUPPORTED.  With iterations = 0 the
 * image equals ptg_render's at the same samples bit for bit. */
int ptg_render_denoised(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                        const ptg_params *params, int device, const ptg_denoise_params *denoise,
                        double *image_rgb);
/* ptg_render_to_noise, then the filter on the frame it stopped at: the same
 * schedule, checks, stop rule and report; the passes carry the moments
 * anyway, so nothing is rendered twice.  The image equals
 * ptg_render_denoised's at samples = report->samples_done bit for bit.
 * samples >= 2; report optional. */
int ptg_render_to_noise_denoised(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                                 const ptg_params *params, int device, const ptg_noise_target *target,
                                 const ptg_denoise_params *denoise, double *image_rgb, ptg_noise_report *report);
/* ---- denoising adaptive frames and frames on several GPUs ---------------
 * ptg_noise_active_device: the variance slab and rho of ptg_noise_device with
 * each pixel's own sample count n_p in place of samples_done -- the V and rho
 * ptg_select_over_device uses internally, the filter's guide for a frame whose
 * pixels stopped at different counts.  d_var (slab_rows * width * 3 floats)
 * and d_rho (slab_rows * width floats) are each optional; slab rows past the
 * image are left untouched; asynchronous on stream; the sums, the counts and
 * the active list are left alone.  n_p < 2 is defined, not an error: rho =
 * +inf as in the select step, and per channel V is the value the definition
 * yields when every sub-pixel's variance sits at the 1/4 cap,
 * (float)(inv_sub2^2 (num_subpixels^2 0.25)) in its double arithmetic:
 * nothing is known beyond the clamp's bound.  State rules as
 * ptg_select_active_device's (PTG_ERR_INVALID_ARGUMENT after a
 * ptg_accumulate_device pass until the next reset, and for floor <= 0); any
 * shard_count.  ptg_noise_device keeps refusing adaptive sums. */
int ptg_noise_active_device(ptg_context *ctx, const ptg_params *params, double floor, float *d_var, float *d_rho,
                            void *stream);

/* ptg_render_adaptive, then the filter on the frame it stopped at: the same
 * schedule, stop rule, report and counts; then ptg_resolve_active_device,
 * ptg_noise_active_device, ptg_features_device, ptg_denoise_device, and the
 * ADD into image_rgb in ptg_render's row order.  denoise NULL or pixel_spread
 * 0 as in ptg_render_denoised.  With iterations = 0 the image, the counts and
 * the report equal ptg_render_adaptive's bit for bit.  PTG_FLAG_EXACT_MATH and
 * PTG_FLAG_LIGHT_SAMPLING are honoured; PTG_FLAG_REFERENCE_F64 is
 * PTG_ERR_UNSUPPORTED. */
int ptg_render_adaptive_denoised(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                                 const ptg_params *params, int device, const ptg_adaptive_target *target,
                                 const ptg_denoise_params *denoise, double *image_rgb, int32_t *sample_counts,
                                 ptg_adaptive_report *report);

/* On a ptg_multi (params->shard_count 1, PTG_FLAG_REFERENCE_F64 refused, the
 * caller's device restored, a broken context refused, as for the entry points
 * of "several GPUs" above).  The pieces act on the sums the context holds and
 * keep them: every shard resolves its slab and writes its variance slab
 * (ptg_noise_device / ptg_noise_active_device), the root receives the colour
 * slabs and the variance slabs -- two gathers through the one path; on RCCL
 * one ncclGather per rank inside a group each, a failure there aborts the
 * communicators and breaks the context as the frame gather's does -- and
 * un-shards both; the features of the whole frame come from the root's own
 * context (they depend on the scene, the camera and the global pixel only, so
 * nothing is moved; the root shard's sums, counts and active list are not
 * touched); ONE filter on the root.  W*H*3 floats are written like
 * ptg_multi_resolve.
 *   ptg_multi_resolve_denoised: after ptg_multi_accumulate passes with
 *     PTG_FLAG_MOMENTS; ptg_multi_noise's rules, samples_done >= 2.
 *   ptg_multi_resolve_active_denoised: while adaptive passes are in the sums;
 *     ptg_multi_resolve_active's rules.
 * The drivers ADD into image_rgb like their unfiltered siblings
 * (ptg_multi_render at samples >= 2 with the moments kept,
 * ptg_multi_render_to_noise, ptg_multi_render_adaptive), whose report, counts
 * and kernel counters they return; the *_multi forms are create + the call +
 * destroy on n_devices distinct GPUs.
 * The guarantee: for any device count, band_rows and dilate the filtered
 * image equals the one-device driver's (ptg_render_denoised,
 * ptg_render_to_noise_denoised, ptg_render_adaptive_denoised) bit for bit:
 * every input of the filter is bit-identical across shardings and the filter
 * is one fixed fp32 sequence over the whole frame. */
int ptg_multi_resolve_denoised(ptg_multi *m, const ptg_params *params, int32_t samples_done,
                               const ptg_denoise_params *denoise, float *image_rgb);
int ptg_multi_resolve_active_denoised(ptg_multi *m, const ptg_params *params, const ptg_denoise_params *denoise,
                                      float *image_rgb);
int ptg_multi_render_denoised(ptg_multi *m, const ptg_params *params, const ptg_denoise_params *denoise,
                              double *image_rgb);
int ptg_multi_render_to_noise_denoised(ptg_multi *m, const ptg_params *params, const ptg_noise_target *target,
                                       const ptg_denoise_params *denoise, double *image_rgb, ptg_noise_report *report);
int ptg_multi_render_adaptive_denoised(ptg_multi *m, const ptg_params *params, const ptg_adaptive_target *target,
                                       const ptg_denoise_params *denoise, double *image_rgb, int32_t *sample_counts,
                                       ptg_adaptive_report *report);
int ptg_render_denoised_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                              const ptg_params *params, const int *devices, int n_devices,
                              const ptg_denoise_params *denoise, double *image_rgb);
int ptg_render_to_noise_denoised_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                                       const ptg_params *params, const int *devices, int n_devices,
                                       const ptg_noise_target *target, const ptg_denoise_params *denoise,
                                       double *image_rgb, ptg_noise_report *report);
int ptg_render_adaptive_denoised_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                                       const ptg_params *params, const int *devices, int n_devices,
                                       const ptg_adaptive_target *target, const ptg_denoise_params *denoise,
                                       double *image_rgb, int32_t *sample_counts, ptg_adaptive_report *report);

/* Host helper: ptg_features_device's frame copied to the host, width *
 * height * 12 floats in ptg_render's row order (row r is the reference's
 * y = height - 1 - r).  Synchronous; params->shard_count must be 1. */
int ptg_features(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                 int device, float *features);
/* The same for ptg_features_follow_device. */
int ptg_features_follow(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                        const ptg_params *params, int device, int32_t max_bounces, float *features);

/* Reassemble shard_count gathered slabs (rank-major, as all-gather lays them
 * out) into the width*height*3 image. */
int ptg_unshard_device(const float *d_gathered, float *d_image, int32_t width, int32_t height,
                       int32_t band_rows, int32_t shard_count, void *stream);

/* Output stage (utils.cpp:11-16 + main.cpp:240-247): 8-bit gamma-1/2.2
 * values round(pow(clamp(x), 1/2.2) * 255) of `count` floats. */
int ptg_tonemap_device(const float *d_image, uint8_t *d_out, size_t count, void *stream);

/* Scene preparation, host only (no device needed): for each sphere the
 * anchor axis chosen for a huge sphere (0..2; -1 = camera-facing anchor, or
 * not huge) and the order of the linear scan (scan_order[j] = scene index of
 * the sphere tested j-th; scenes of <= 64 spheres).  Exact ties between
 * candidate roots (two spheres of equal geometry: one pasted twice, a lamp's
 * shell on a body of the same radius) go to the sphere tested first: the
 * spheres of one kind are tested in scene index order, so among equal spheres
 * that is the lowest scene index.  Scenes of more than 64 spheres (BVH):
 * every root is divided and the smallest t wins, the lowest scene index on
 * exact ties -- whatever order the walk visits the spheres in, so the frame
 * does not depend on the order of the scene's spheres beyond the order inside
 * each group of equal spheres.  The sphere that loses a tie is never seen. */
int ptg_scene_layout(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int32_t *anchor_axis,
                     int32_t *scan_order);

/* PTG_FLAG_LIGHT_SAMPLING's light list, host only: the scene indices of the
 * emissive spheres that are not huge, ascending.  *n_lights receives their
 * number; ids (cap entries, may be NULL when cap is 0) the first
 * min(cap, *n_lights) of them.  More than PTG_MAX_LIGHTS: *n_lights is set
 * and the call returns PTG_ERR_UNSUPPORTED, as rendering with the flag does. */
int ptg_light_list(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int32_t *ids, int cap,
                   int *n_lights);

/* Parity probe: trace individual samples.  d_coords holds n records
 * {x, y, sx, sy, sample} (int32 each); d_out n*3 floats (radiance of that
 * one path, main.cpp:191); d_segs n int32 (scene scans of that path). */
int ptg_trace_samples_device(ptg_context *ctx, const ptg_params *params, const int32_t *d_coords, size_t n,
                             float *d_out, int32_t *d_segs, void *stream);

/* Accuracy probe of the kernels' arithmetic primitives in either mode
 * (exact != 0: PTG_FLAG_EXACT_MATH's sequences; 0: the hardware
 * instructions), n operands on the device: op PTG_PROBE_SQRT out[i] =
 * sqrt(in[i]); PTG_PROBE_RSQRT 1/sqrt(in[i]); PTG_PROBE_DIV in[2i] /
 * in[2i+1] (divisor > 0); PTG_PROBE_SINCOS the bits of in[i] are a 24-bit
 * integer m, out[2i], out[2i+1] = cos, sin of 2 pi m 2^-24 (main.cpp:55's
 * phi).  The arithmetic the render kernels execute, not a separate
 * implementation (tests/test_gpu_fast_math.py). */
#define PTG_PROBE_SQRT 0
#define PTG_PROBE_RSQRT 1
#define PTG_PROBE_DIV 2
#define PTG_PROBE_SINCOS 3
int ptg_math_probe_device(ptg_context *ctx, int32_t op, int32_t exact, const float *d_in, float *d_out, size_t n,
                          void *stream);

/* Probe of PTG_FLAG_STRATIFIED's sampler: for n records {x, y, sx, sy,
 * sample} (int32 each, as ptg_trace_samples_device takes them) d_out receives
 * 8 uint32 per record, {m0, m1} of pairs 0..3 of that path under params'
 * seed, width and num_subpixels -- the integers the render kernels form,
 * whatever params->flags says. */
int ptg_sampler_pairs_device(ptg_context *ctx, const ptg_params *params, const int32_t *d_coords, size_t n,
                             uint32_t *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTGPU_H */
