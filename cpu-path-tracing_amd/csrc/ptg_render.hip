// ptg_render.hip -- the one translation unit of the MI355X render loop: the
// host side of the C ABI (include/ptgpu.h) -- ptg_context and its accumulator
// bookkeeping, the kernel launchers and the entry points.  The device code is
// in the headers included below inside the unnamed namespace, by topic;
// render_unit.hpp says how the render loop maps onto CDNA4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ptgpu.h"
#include "bvh_build.hpp"
#include "frame_passes.hpp"  // add_image: the ADD into the caller's image
#include "kernel_args.hpp"  // KArgs and the constants shared with the host side
#include "launch_plan.hpp"  // check_params, fill_launch and their tunables
#include "pt_device.hpp"
#include "ptg_error.hpp"
#include "ref64.hpp"
#include "scene_prep.hpp"  // scene records, scan order, box mode, the uploads
#include "sobol_pairs.hpp"  // PTG_FLAG_STRATIFIED: the scrambled Sobol' pairs

using namespace ptg;

namespace {

#define PTG_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(PTG_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)

// the device code, in this order (each header says what it needs from before it)
#include "render_config.hpp"  // tunables, debug-statistics switches
#include "scan_linear.hpp"    // scene_scan, box mode
#include "scan_bvh.hpp"       // the BVH walk and leaf phase, scene_scan_bvh
#include "shade.hpp"          // shade, segment, light sampling
#include "render_unit.hpp"    // camera_ray, render_unit, the nine pool kernels
#include "accum_kernels.hpp"  // resolve, noise, active-list kernels
#include "probe_kernels.hpp"  // trace, features (follow_features.hpp), probes, unshard, tonemap

}  // namespace

struct ptg_context {
    int device;
    int n;
    int wave_slots;     // CUs x 32 resident waves (split-tail sizing)
    LinRec *d_lin;      // linear scenes
    ShadeRec *d_shade;  // BVH scenes
    void *d_bvh;  // one allocation: nodes | leaf geometry | leaf ids | big geometry | big ids
    float2 *d_trig;  // sin/cos table (trig_table)
    unsigned long long *d_acc;  // exact per-sub-pixel sums; kept zero between frames by resolve
    size_t acc_elems;
    bool acc_dirty;  // progressive sums may be in d_acc (accumulate / keep_acc resolve since the last reset)
    KArgs base;  // camera + scene fields filled
    ptg_sphere *d_sph64;  // the scene as given (PTG_FLAG_REFERENCE_F64)
    ptg_camera cam64;
    // PTG_FLAG_MOMENTS: exact per-sub-pixel sums of squares, laid out like d_acc; allocated on first use
    unsigned long long *d_acc2;
    size_t acc2_elems;
    bool moments_pass;  // a pass since the last reset added to d_acc2 ...
    bool plain_pass;    // ... or ran without the flag (d_acc2 then lacks its samples: no noise estimate)
    // adaptive sampling (ptg_*_active_device), allocated on first use: per slab pixel its sample count, the
    // over-target bytes, the active list (per slab row, stride W, its active x ascending), per slab row its
    // active pixels and first unit, the unit table (n_groups entries) and the device record {pixels, units}
    int32_t *d_counts;
    uint8_t *d_over;
    int *d_list, *d_row_count, *d_row_unit0;
    int4 *d_units;
    unsigned long long *d_rec;
    size_t ad_pixels, ad_rows, ad_groups;  // what the buffers above have room for
    ptg_params list_frame;  // the frame the active list was built for ...
    bool list_valid;        // ... if any since the last reset
    bool uniform_pass;      // a ptg_accumulate_device pass since the last reset: no adaptive entry point
    bool adaptive_pass;     // a ptg_accumulate_active_device pass since the last reset: no uniform n describes the sums
    long long adaptive_added;  // the adds since the last reset: no count is above their sum
    // PTG_FLAG_LIGHT_SAMPLING: the scene's light list (scene indices; more than kMaxLights: the flag is
    // refused) and its device records (base.lights, base.n_lights)
    int n_lights;
    int light_ids[kMaxLights];
    LightRec *d_lights;
};

namespace {

int set_device(int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PTG_ERR_NO_DEVICE, "no HIP device visible");
    if (device >= count)
        return fail(PTG_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    if (device >= 0)
        PTG_HIP(hipSetDevice(device));
    return PTG_OK;
}

// ptg_context_create: one of the context's device tables, allocated and filled
template <typename T>
int upload(T *&dst, const void *src, size_t bytes, const char *what)
{
    if (hipMalloc(&dst, bytes) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, std::string("hipMalloc of ") + what + " failed");
    PTG_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return PTG_OK;
}

#if PTG_BLOCK_STATS
// a 256 x 16 block-counter array (ptg_dbg_stats, ptg_dbg_stats2) summed over its slots, then zeroed
template <typename Sym>
int read_block_stats(const Sym &sym, unsigned long long *out16)
{
    std::vector<unsigned long long> h(256 * 16);
    PTG_HIP(hipDeviceSynchronize());
    PTG_HIP(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(sym), h.size() * sizeof(h[0])));
    for (int i = 0; i < 16; ++i) {
        out16[i] = 0;
        for (int b = 0; b < 256; ++b)
            out16[i] += h[b * 16 + i];
    }
    std::vector<unsigned long long> z(h.size(), 0ull);
    PTG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(sym), z.data(), z.size() * sizeof(z[0])));
    return PTG_OK;
}
#endif

}  // namespace

extern "C" {

// internal (csrc/ptg_multi.cpp): set the thread-local error of ptg_last_error
int ptg_set_error_(int code, const char *msg) { return fail(code, msg ? msg : ""); }

int ptg_abi_version(void) { return PTG_ABI_VERSION; }

#if PTG_UNIT_TRACE
// debug builds only: the per-unit trace of the launches since the last call
// (3 values per unit, see ptg_unit_trace; then zeroed)
int ptg_unit_trace_(unsigned long long *out, int n_units)
{
    const size_t n = (size_t)std::min(n_units, kTraceUnits) * 3;
    PTG_HIP(hipDeviceSynchronize());
    PTG_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(ptg_unit_trace), n * sizeof(unsigned long long)));
    std::vector<unsigned long long> z(n, 0ull);
    PTG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ptg_unit_trace), z.data(), n * sizeof(unsigned long long)));
    return PTG_OK;
}
#endif
#if PTG_BLOCK_STATS
// debug builds only: the 16 block counters summed over their 256 slots (then zeroed)
int ptg_debug_stats2_(unsigned long long *out16) { return read_block_stats(ptg_dbg_stats2, out16); }
int ptg_debug_stats_(unsigned long long *out16) { return read_block_stats(ptg_dbg_stats, out16); }
#endif

const char *ptg_last_error(void) { return g_last_error.c_str(); }

int ptg_device_count(int *count)
{
    if (!count)
        return fail(PTG_ERR_INVALID_ARGUMENT, "count is NULL");
    *count = 0;
    if (hipGetDeviceCount(count) != hipSuccess)
        *count = 0;
    return PTG_OK;
}

int ptg_shard_rows(int32_t height, int32_t band_rows, int32_t shard_count, int32_t *rows)
{
    if (!rows || height <= 0 || band_rows <= 0 || shard_count <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "invalid shard geometry");
    *rows = shard_slab_rows(height, band_rows, shard_count);
    return PTG_OK;
}

int ptg_context_create(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int device,
                       ptg_context **out)
{
    if (!out || !cam || (n_spheres && !spheres))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (n_spheres > (size_t)(1 << 24))
        return fail(PTG_ERR_UNSUPPORTED, "too many spheres");
    for (size_t i = 0; i < n_spheres; ++i)
        if (!sphere_ok(spheres[i]))
            return fail(PTG_ERR_INVALID_ARGUMENT, "sphere " + std::to_string(i) + " is invalid");
    int rc = set_device(device);
    if (rc)
        return rc;
    int dev = 0;
    PTG_HIP(hipGetDevice(&dev));
    ptg_context *ctx = new ptg_context();  // zeroed, base included
    ctx->device = dev;
    {
        hipDeviceProp_t prop;
        ctx->wave_slots = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount * 32 : 8192;
    }
    const int n = ctx->n = (int)n_spheres;
    ctx->cam64 = *cam;
    KArgs &A = ctx->base;
    // prepare (scene_prep.hpp): the upload tables; the scan layout goes straight into A
    const bool linear = n <= kLinearMax;
    const SceneRecs sc = prepare_scene(spheres, n, cam);
    std::vector<LinRec> lin;
    BvhUpload bvh;
    if (linear)
        lin = prepare_linear_upload(spheres, n, cam, sc, A);
    else
        bvh = prepare_bvh_upload(spheres, n, cam, sc.geo);
    float trig[2 * kTrigEntries];
    trig_table(trig);
    // allocate and upload.  linear scenes: d_lin; BVH scenes: d_shade (scene index order) + d_bvh
    rc = linear ? upload(ctx->d_lin, lin.data(), lin.size() * sizeof(LinRec), "the scene")
                : upload(ctx->d_shade, sc.shade.data(), (size_t)n * sizeof(ShadeRec), "the scene");
    if (!rc)
        rc = upload(ctx->d_trig, trig, sizeof(trig), "the sin/cos table");
    if (!rc && n)
        rc = upload(ctx->d_sph64, spheres, (size_t)n * sizeof(ptg_sphere), "the scene (f64)");
    if (!rc && !linear)
        rc = upload(ctx->d_bvh, bvh.blob.data(), bvh.blob.size(), "the BVH");
    // the light list (light sampling); too long a list is refused where the flag is given
    const std::vector<int> light_ids = light_list_of(spheres, n, cam);
    ctx->n_lights = (int)light_ids.size();
    if (!rc && ctx->n_lights > 0 && ctx->n_lights <= kMaxLights) {
        std::vector<int> id_of(n);
        for (int i = 0; i < n; ++i)
            id_of[i] = i;
        if (linear) {  // the scan reports scan positions
            KArgs scratch{};
            const std::vector<int> order = scan_order_of(spheres, n, cam, sc, scratch);
            for (int j = 0; j < n; ++j)
                id_of[order[j]] = j;
        }
        const std::vector<LightRec> lrecs = light_records(spheres, light_ids, id_of);
        for (int k = 0; k < ctx->n_lights; ++k)
            ctx->light_ids[k] = light_ids[k];
        rc = upload(ctx->d_lights, lrecs.data(), lrecs.size() * sizeof(LightRec), "the light list");
    }
    if (rc) {
        ptg_context_destroy(ctx);
        return rc;
    }
    // the scene and camera fields of every launch's KArgs
    A.trig = ctx->d_trig;
    A.lin = ctx->d_lin;
    A.shade = ctx->d_shade;
    A.n = n;
    A.room_nmr = room_neg_margin(A);
    A.lights = ctx->d_lights;
    A.n_lights = ctx->d_lights ? ctx->n_lights : 0;
    if (!linear) {
        const unsigned char *blob = static_cast<const unsigned char *>(ctx->d_bvh);
        A.bvh_qnodes = reinterpret_cast<const uint4 *>(blob + bvh.off_q);
        A.bvh_cont = reinterpret_cast<const int *>(blob + bvh.off_cont);
        A.bvh_sph = reinterpret_cast<const float4 *>(blob + bvh.off_geo);
        A.bvh_id = reinterpret_cast<const int *>(blob + bvh.off_id);
        A.big_geo = reinterpret_cast<const GeoRec *>(blob + bvh.off_bgeo);
        A.big_id = reinterpret_cast<const int *>(blob + bvh.off_bid);
        for (int c = 0; c < 3; ++c) {
            A.q_lo[c] = bvh.q_lo[c];
            A.q_scale[c] = bvh.q_scale[c];
        }
        A.n_nodes = bvh.n_nodes;
        A.n_big = bvh.n_big;
    }
    prepare_camera(cam, A);
    *out = ctx;
    return PTG_OK;
}

int ptg_scene_layout(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int32_t *anchor_axis,
                     int32_t *scan_order)
{
    if (!cam || (n_spheres && (!spheres || !anchor_axis || !scan_order)))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_spheres > (size_t)(1 << 24))
        return fail(PTG_ERR_UNSUPPORTED, "too many spheres");
    const int n = (int)n_spheres;
    const SceneRecs sc = prepare_scene(spheres, n, cam);
    KArgs ends{};
    std::vector<int> order;
    if (n <= kLinearMax)
        order = scan_order_of(spheres, n, cam, sc, ends);
    for (int i = 0; i < n; ++i)
        anchor_axis[i] = sc.axis[i];
    for (int k = 0; k < 3 && n <= kLinearMax; ++k)
        if (ends.pairs[k])  // the pair leads axis k's group
            anchor_axis[order[k == 0 ? 0 : ends.end_ax[k - 1]]] = anchor_axis[order[(k == 0 ? 0 : ends.end_ax[k - 1]) + 1]] = k + 3;
    for (int i = 0; i < n; ++i)
        scan_order[i] = n <= kLinearMax ? order[i] : i;
    return PTG_OK;
}

int ptg_light_list(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int32_t *ids, int cap,
                   int *n_lights)
{
    if (!cam || !n_lights || (n_spheres && !spheres) || cap < 0 || (cap && !ids))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_spheres > (size_t)(1 << 24))
        return fail(PTG_ERR_UNSUPPORTED, "too many spheres");
    const std::vector<int> list = light_list_of(spheres, (int)n_spheres, cam);
    *n_lights = (int)list.size();
    for (int k = 0; k < cap && k < (int)list.size(); ++k)
        ids[k] = list[k];
    if ((int)list.size() > kMaxLights)
        return fail(PTG_ERR_UNSUPPORTED, "light sampling: " + std::to_string(list.size()) +
                                             " small emitters, at most " + std::to_string(kMaxLights));
    return PTG_OK;
}

int ptg_context_destroy(ptg_context *ctx)
{
    if (!ctx)
        return PTG_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->d_lin)
        (void)hipFree(ctx->d_lin);
    if (ctx->d_shade)
        (void)hipFree(ctx->d_shade);
    if (ctx->d_trig)
        (void)hipFree(ctx->d_trig);
    if (ctx->d_bvh)
        (void)hipFree(ctx->d_bvh);
    if (ctx->d_acc)
        (void)hipFree(ctx->d_acc);
    if (ctx->d_acc2)
        (void)hipFree(ctx->d_acc2);
    if (ctx->d_sph64)
        (void)hipFree(ctx->d_sph64);
    if (ctx->d_lights)
        (void)hipFree(ctx->d_lights);
    for (void *q : {(void *)ctx->d_counts, (void *)ctx->d_over, (void *)ctx->d_list, (void *)ctx->d_row_count,
                    (void *)ctx->d_row_unit0, (void *)ctx->d_units, (void *)ctx->d_rec})
        if (q)
            (void)hipFree(q);
    delete ctx;
    return PTG_OK;
}

}  // extern "C"

namespace {

size_t acc_elems_for(const KArgs &A) { return (size_t)A.slab_rows * A.W * A.lanes_per_pixel * 3; }

// the second accumulator zero and no pass on record
int forget_moments(ptg_context *ctx, hipStream_t stream)
{
    if (ctx->d_acc2 && ctx->moments_pass)  // (only such passes write to it)
        PTG_HIP(hipMemsetAsync(ctx->d_acc2, 0, ctx->acc2_elems * sizeof(unsigned long long), stream));
    ctx->moments_pass = ctx->plain_pass = false;
    // the adaptive frame with them: counts zero, no list, no pass of either kind on record
    if (ctx->d_counts && (ctx->adaptive_pass || ctx->adaptive_added))
        PTG_HIP(hipMemsetAsync(ctx->d_counts, 0, ctx->ad_pixels * sizeof(int32_t), stream));
    ctx->list_valid = ctx->uniform_pass = ctx->adaptive_pass = false;
    ctx->adaptive_added = 0;
    return PTG_OK;
}

// exact accumulator: allocated (zeroed) on first use at a size; resolve_kernel
// keeps it zero between one-shot frames.  The zeroing is queued on the launch
// stream: a hipMemset on the null stream is not ordered before kernels on a
// non-blocking stream (ptg_render_multi's), whose first frame could then add
// into a buffer being cleared (seen once as a differing box_mirror frame)
int ensure_acc(ptg_context *ctx, size_t need, hipStream_t stream)
{
    if (need <= ctx->acc_elems)
        return PTG_OK;
    if (ctx->d_acc)
        PTG_HIP(hipFree(ctx->d_acc));
    ctx->d_acc = nullptr;
    ctx->acc_elems = 0;
    if (hipMalloc(&ctx->d_acc, need * sizeof(unsigned long long)) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the accumulator failed");
    PTG_HIP(hipMemsetAsync(ctx->d_acc, 0, need * sizeof(unsigned long long), stream));
    ctx->acc_elems = need;
    ctx->acc_dirty = false;  // (a progressive frame in the old buffer is lost: reset before reuse)
    return forget_moments(ctx, stream);
}

// PTG_FLAG_MOMENTS passes: the second accumulator at the first one's size
// (ensure_acc first), zeroed on allocation like it
int ensure_acc2(ptg_context *ctx, hipStream_t stream)
{
    if (ctx->acc_elems <= ctx->acc2_elems)
        return PTG_OK;
    if (ctx->d_acc2)
        PTG_HIP(hipFree(ctx->d_acc2));
    ctx->d_acc2 = nullptr;
    ctx->acc2_elems = 0;
    if (hipMalloc(&ctx->d_acc2, ctx->acc_elems * sizeof(unsigned long long)) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the second-moment accumulator failed");
    PTG_HIP(hipMemsetAsync(ctx->d_acc2, 0, ctx->acc_elems * sizeof(unsigned long long), stream));
    ctx->acc2_elems = ctx->acc_elems;
    return PTG_OK;
}

// Both accumulators zero, no progressive frame in them (reset; a one-shot
// frame that needs the first accumulator after progressive passes)
int clear_accumulation(ptg_context *ctx, hipStream_t stream)
{
    if (ctx->d_acc)
        PTG_HIP(hipMemsetAsync(ctx->d_acc, 0, ctx->acc_elems * sizeof(unsigned long long), stream));
    ctx->acc_dirty = false;
    return forget_moments(ctx, stream);
}

// ptg_noise_device / ptg_read_moments_device: the second accumulator holds
// the squares of exactly the samples the first one holds
int check_moments(const ptg_context *ctx, const KArgs &A, const char *who)
{
    if (!ctx->moments_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": no PTG_FLAG_MOMENTS pass since the last reset");
    if (ctx->plain_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": a pass since the last reset ran without PTG_FLAG_MOMENTS");
    if (!ctx->d_acc2 || ctx->acc2_elems < acc_elems_for(A) || ctx->acc_elems < acc_elems_for(A))
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": the passes were of a smaller frame");
    return PTG_OK;
}

// While adaptive passes are in the sums, the pixels hold different numbers of
// samples: the entry points that take one n for the slab refuse ...
int refuse_after_adaptive(const ptg_context *ctx, const char *who)
{
    if (ctx->adaptive_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": adaptive passes since the last reset (the pixels "
                                              "hold different sample counts: use the *_active entry points, or reset)");
    return PTG_OK;
}

// ... and the adaptive ones after a uniform pass, which the count slab does not know of
int refuse_after_uniform(const ptg_context *ctx, const char *who)
{
    if (ctx->uniform_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": a ptg_accumulate_device pass since the last reset "
                                              "(the sample counts do not describe its sums: reset first)");
    return PTG_OK;
}

// PTG_FLAG_LIGHT_SAMPLING on a scene with more small emitters than the light list holds
int check_lights(const ptg_context *ctx, const ptg_params *p)
{
    if ((p->flags & PTG_FLAG_LIGHT_SAMPLING) && ctx->n_lights > kMaxLights)
        return fail(PTG_ERR_UNSUPPORTED, "light sampling: " + std::to_string(ctx->n_lights) +
                                             " small emitters, at most " + std::to_string(kMaxLights));
    return PTG_OK;
}

// The device entry points' common start, after their argument checks: the
// context's device current and the launch plan for samples [s_begin, s_end);
// with_acc: the exact accumulator at the plan's size as well.
int begin_launch(ptg_context *ctx, const ptg_params *p, KArgs &A, int &grid, hipStream_t s, bool with_acc,
                 int s_begin = 0, int s_end = -1, bool accumulate_only = false)
{
    PTG_HIP(hipSetDevice(ctx->device));
    int rc = check_lights(ctx, p);
    if (!rc)
        rc = fill_launch(ctx->base, ctx->wave_slots, p, A, grid, s_begin, s_end, accumulate_only);
    return rc || !with_acc ? rc : ensure_acc(ctx, acc_elems_for(A), s);
}

// a run-time bool as a compile-time one: f(std::true_type{}) or f(std::false_type{})
template <class F>
void with_bool(bool b, F &&f)
{
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// The pool kernel of a launch (render_unit.hpp), one of 96.  Which of the
// three it is follows from the arguments: render without acc2, moments with
// it, gather with the active list's G as well.  Its family: _strat with
// PTG_FLAG_STRATIFIED, else _ls with lights to sample (n_lights is 0 without
// PTG_FLAG_LIGHT_SAMPLING), else plain.  Block size and LDS bytes follow kBvh:
// linear scenes stage n + 4 records (the exact mode's sin/cos table has its
// own LDS), BVH scenes none.
int launch_pool(const KArgs &A, int grid, bool count, hipStream_t s, unsigned long long *acc2 = nullptr,
                const GatherArgs *G = nullptr)
{
    if (grid <= 0)
        return PTG_OK;
    const bool is_bvh = A.n > kLinearMax;
    const size_t lds = is_bvh ? 0 : (size_t)(A.n + 2 + 2) * sizeof(LinRec);
    with_bool(A.stratified != 0, [&](auto st) {
        with_bool(A.n_lights > 0, [&](auto ls) {
            with_bool(count, [&](auto cn) {
                with_bool(is_bvh, [&](auto bv) {
                    with_bool(A.exact_math != 0, [&](auto ex) {
                        constexpr bool kL = decltype(ls)::value, kC = decltype(cn)::value, kB = decltype(bv)::value,
                                       kE = decltype(ex)::value;
                        constexpr int kBl = kBlockOf<kB>;
                        if constexpr (decltype(st)::value) {
                            if (G)
                                gather_strat<kC, kB, kE, kL><<<grid, kBl, lds, s>>>(A, acc2, *G);
                            else if (acc2)
                                moments_strat<kC, kB, kE, kL><<<grid, kBl, lds, s>>>(A, acc2);
                            else
                                render_strat<kC, kB, kE, kL><<<grid, kBl, lds, s>>>(A);
                        } else if constexpr (kL) {
                            if (G)
                                gather_ls<kB, kE, kC><<<grid, kBl, lds, s>>>(A, acc2, *G);
                            else if (acc2)
                                moments_ls<kB, kE, kC><<<grid, kBl, lds, s>>>(A, acc2);
                            else
                                render_ls<kC, kB, kE><<<grid, kBl, lds, s>>>(A);
                        } else {
                            if (G)
                                gather_kernel<kB, kE, kC><<<grid, kBl, lds, s>>>(A, acc2, *G);
                            else if (acc2)
                                moments_kernel<kB, kE, kC><<<grid, kBl, lds, s>>>(A, acc2);
                            else
                                render_kernel<kC, kB, kE><<<grid, kBl, lds, s>>>(A);
                        }
                    });
                });
            });
        });
    });
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

// ptg_features_device / ptg_features_follow_device after their argument
// checks: the launch plan of the frame's geometry only (the scan's fields are
// those of the exact mode whatever the flags) and a lane per slab pixel
int begin_features(ptg_context *ctx, const ptg_params *params, KArgs &A, unsigned &blocks, hipStream_t s)
{
    int grid = 0;
    ptg_params geo = *params;
    geo.samples = 1;
    geo.chunk_samples = 0;
    geo.flags = PTG_FLAG_EXACT_MATH;
    const int rc = begin_launch(ctx, &geo, A, grid, s, /*with_acc=*/false);
    if (!rc)
        blocks = (unsigned)(((long long)A.slab_rows * A.W + 255) / 256);
    return rc;
}

// the grid of a kernel that strides over `items`, `per_block` of them per
// block and pass: one block each, at most kNoiseBlocks
unsigned strided_blocks(long long items, int per_block = 256)
{
    const long long blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < kNoiseBlocks ? blocks : kNoiseBlocks);
}

// PTG_FLAG_REFERENCE_F64: the reference's double arithmetic (ref64.hpp), one
// lane per sub-pixel; out64 or out32 receives the slab
int launch_ref64(const ptg_context *ctx, const KArgs &A, double *out64, float *out32,
                 unsigned long long *d_segments, hipStream_t s)
{
    ref64::Args R{};
    R.spheres = ctx->d_sph64;
    R.n = ctx->n;
    R.cam = ctx->cam64;
    R.W = A.W;
    R.H = A.H;
    R.samps = A.samps;
    R.nsub = A.nsub;
    R.lanes_per_pixel = A.lanes_per_pixel;
    R.pixels_per_wave = A.pixels_per_wave;
    R.waves_per_row = A.waves_per_row;
    R.slab_rows = A.slab_rows;
    R.band_rows = A.band_rows;
    R.shard_rank = A.shard_rank;
    R.shard_count = A.shard_count;
    R.seed = A.seed;
    R.out64 = out64;
    R.out32 = out32;
    R.segments = d_segments;
    R.n_lights = A.n_lights;  // (0 without PTG_FLAG_LIGHT_SAMPLING: plan_frame)
    R.stratified = A.stratified;
    for (int k = 0; k < A.n_lights; ++k)
        R.lights[k] = ctx->light_ids[k];
    const long long waves = (long long)A.slab_rows * A.waves_per_row;
    const long long blocks = (waves + 3) / 4;
    if (blocks > 0x7FFFFFFFLL)
        return fail(PTG_ERR_UNSUPPORTED, "image too large for the reference-arithmetic mode");
    if (blocks > 0)
        ref64::render_kernel<<<(unsigned)blocks, 256, 0, s>>>(R);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

// The adaptive buffers at the frame's size (allocated on first use; a larger
// frame replaces them: counts zero, no list)
int ensure_adaptive(ptg_context *ctx, const KArgs &A, hipStream_t stream)
{
    const size_t pixels = (size_t)A.slab_rows * A.W, rows = (size_t)A.slab_rows, groups = (size_t)A.n_groups;
    if (pixels <= ctx->ad_pixels && rows <= ctx->ad_rows && groups <= ctx->ad_groups)
        return PTG_OK;
    if (ctx->adaptive_pass)
        return fail(PTG_ERR_INVALID_ARGUMENT, "the adaptive passes since the last reset were of a smaller frame");
    for (void **q : {(void **)&ctx->d_counts, (void **)&ctx->d_over, (void **)&ctx->d_list, (void **)&ctx->d_row_count,
                     (void **)&ctx->d_row_unit0, (void **)&ctx->d_units, (void **)&ctx->d_rec}) {
        if (*q)
            PTG_HIP(hipFree(*q));
        *q = nullptr;
    }
    ctx->ad_pixels = ctx->ad_rows = ctx->ad_groups = 0;
    ctx->list_valid = false;
    if (hipMalloc(&ctx->d_counts, pixels * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&ctx->d_over, pixels) != hipSuccess || hipMalloc(&ctx->d_list, pixels * sizeof(int)) != hipSuccess ||
        hipMalloc(&ctx->d_row_count, rows * sizeof(int)) != hipSuccess ||
        hipMalloc(&ctx->d_row_unit0, rows * sizeof(int)) != hipSuccess ||
        hipMalloc(&ctx->d_units, groups * sizeof(int4)) != hipSuccess ||
        hipMalloc(&ctx->d_rec, 2 * sizeof(unsigned long long)) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the adaptive-sampling buffers failed");
    PTG_HIP(hipMemsetAsync(ctx->d_counts, 0, pixels * sizeof(int32_t), stream));
    PTG_HIP(hipMemsetAsync(ctx->d_rec, 0, 2 * sizeof(unsigned long long), stream));
    ctx->ad_pixels = pixels;
    ctx->ad_rows = rows;
    ctx->ad_groups = groups;
    return PTG_OK;
}

// the slab geometry of two frames is the same (the active list and the counts are indexed by it)
bool same_slab(const ptg_params &a, const ptg_params &b)
{
    return a.width == b.width && a.height == b.height && a.num_subpixels == b.num_subpixels &&
           a.band_rows == b.band_rows && a.shard_rank == b.shard_rank && a.shard_count == b.shard_count;
}

// The adaptive entry points' common start: argument checks done, no uniform
// pass in the sums, the launch plan's frame fields, both accumulators and the
// adaptive buffers at the frame's size.
int begin_adaptive(ptg_context *ctx, const ptg_params *p, KArgs &A, hipStream_t s, const char *who)
{
    if (p->flags & PTG_FLAG_REFERENCE_F64)
        return fail(PTG_ERR_UNSUPPORTED, std::string(who) + ": progressive passes are fp32 only");
    int rc = refuse_after_uniform(ctx, who), grid = 0;
    if (rc || (rc = begin_launch(ctx, p, A, grid, s, /*with_acc=*/true)) || (rc = ensure_acc2(ctx, s)))
        return rc;
    A.acc = ctx->d_acc;
    return ensure_adaptive(ctx, A, s);
}

// List-building steps 2 and 3 after step 1: list_rows_kernel on `flags`, or,
// gathered, list_rows_gathered_kernel on the whole frame's rank-major slabs
int build_list(ptg_context *ctx, const ptg_params *p, const KArgs &A, const uint8_t *flags, int dilate,
               unsigned long long *d_info, unsigned long long *d_stats, hipStream_t s, bool gathered = false)
{
    if (A.slab_rows > 0) {
        if (gathered)
            list_rows_gathered_kernel<<<A.slab_rows, 256, 0, s>>>(A, flags, dilate, ctx->d_list, ctx->d_row_count);
        else
            list_rows_kernel<<<A.slab_rows, 256, 0, s>>>(A, flags, dilate, ctx->d_list, ctx->d_row_count);
        PTG_HIP(hipGetLastError());
    }
    list_units_kernel<<<1, 256, 0, s>>>(A.slab_rows, A.pixels_per_wave, ctx->d_row_count, ctx->d_row_unit0, ctx->d_rec,
                                        d_info, d_stats);
    PTG_HIP(hipGetLastError());
    if (A.slab_rows > 0) {
        list_fill_kernel<<<A.slab_rows, 256, 0, s>>>(A.pixels_per_wave, ctx->d_row_count, ctx->d_row_unit0, ctx->d_units);
        PTG_HIP(hipGetLastError());
    }
    ctx->list_frame = *p;
    ctx->list_valid = true;
    return PTG_OK;
}

int launch_resolve(const KArgs &A, hipStream_t s)
{
    long long pixels = (long long)(A.slab_rows - A.resolve_row0) * A.W;
    if (pixels <= 0)
        return PTG_OK;
    resolve_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, s>>>(A);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

}  // namespace

extern "C" {

int ptg_render_device(ptg_context *ctx, const ptg_params *params, float *d_slab, unsigned long long *d_segments,
                      void *stream)
{
    if (!ctx || !d_slab)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/false)))
        return rc;
    if (params->flags & PTG_FLAG_REFERENCE_F64)
        return launch_ref64(ctx, A, nullptr, d_slab, d_segments, s);
    // several units per pixel, a split tail accumulated in HBM, or no samples at all
    const bool resolve = A.needs_resolve || grid == 0;
    if ((rc = ensure_acc(ctx, resolve ? acc_elems_for(A) : 0, s)))
        return rc;
    A.out = d_slab;
    A.acc = ctx->d_acc;
    A.segments = d_segments;
    if (resolve && ctx->acc_dirty) {
        // progressive sums left by accumulate / keep_acc resolve: a one-shot
        // frame starts from zero (its resolve leaves the buffer zero again)
        if ((rc = clear_accumulation(ctx, s)))
            return rc;
    }
    if ((rc = launch_pool(A, grid, d_segments != nullptr, s)))
        return rc;
    return resolve ? launch_resolve(A, s) : PTG_OK;
}

int ptg_launch_info(ptg_context *ctx, const ptg_params *params, int64_t *info, int n_info)
{
    if (!ctx || !info || n_info < 1)
        return fail(PTG_ERR_INVALID_ARGUMENT, "launch_info: NULL argument");
    int rc = check_params(params);
    if (rc)
        return rc;
    KArgs A;
    int grid = 0;
    if ((rc = fill_launch(ctx->base, ctx->wave_slots, params, A, grid)))
        return rc;
    const bool bvh = ctx->n > kLinearMax;
    const int64_t v[PTG_LAUNCH_INFO_COUNT] = {
        bvh ? 0 : A.box_mode, bvh ? 0 : A.box_walls_out, bvh ? 1 : 0, A.n_units, grid, A.n_levels,
        A.needs_resolve ? 1 : 0, (int64_t)(A.pairs[0] | (A.pairs[1] << 1) | (A.pairs[2] << 2))};
    for (int i = 0; i < n_info; ++i)
        info[i] = i < PTG_LAUNCH_INFO_COUNT ? v[i] : 0;
    return PTG_OK;
}

int ptg_accumulate_device(ptg_context *ctx, const ptg_params *params, int32_t sample_begin, int32_t sample_end,
                          unsigned long long *d_segments, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (sample_begin < 0 || sample_end < sample_begin || sample_end > params->samples)
        return fail(PTG_ERR_INVALID_ARGUMENT, "sample range must satisfy 0 <= begin <= end <= samples");
    if (params->flags & PTG_FLAG_REFERENCE_F64)
        return fail(PTG_ERR_UNSUPPORTED, "progressive passes are fp32 only (the reference-arithmetic mode sums "
                                         "its samples sequentially, main.cpp:192)");
    if ((rc = refuse_after_adaptive(ctx, "accumulate")))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true, sample_begin, sample_end,
                           /*accumulate_only=*/true)))
        return rc;
    const bool moments = (params->flags & PTG_FLAG_MOMENTS) != 0;
    if (moments && (rc = ensure_acc2(ctx, s)))
        return rc;
    A.acc = ctx->d_acc;
    A.segments = d_segments;
    ctx->acc_dirty = true;
    if (grid > 0)  // (an empty pass adds no samples to either accumulator)
        (moments ? ctx->moments_pass : ctx->plain_pass) = ctx->uniform_pass = true;
    return launch_pool(A, grid, d_segments != nullptr, s, moments ? ctx->d_acc2 : nullptr);
}

int ptg_resolve_device(ptg_context *ctx, const ptg_params *params, int32_t samples_done, float *d_slab, void *stream)
{
    if (!ctx || !d_slab)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (samples_done < 0 || samples_done > params->samples)
        return fail(PTG_ERR_INVALID_ARGUMENT, "samples_done must be in [0, samples]");
    if ((rc = refuse_after_adaptive(ctx, "resolve")))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true)))
        return rc;
    A.samps = samples_done;  // mean over the samples accumulated so far
    A.keep_acc = 1;
    A.resolve_row0 = 0;  // every row (the one-shot split tail does not apply here)
    A.acc = ctx->d_acc;
    A.out = d_slab;
    return launch_resolve(A, s);
}

int ptg_reset_accumulation_device(ptg_context *ctx, const ptg_params *params, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true)))
        return rc;
    return clear_accumulation(ctx, s);
}

int ptg_noise_device(ptg_context *ctx, const ptg_params *params, int32_t samples_done, double rel_error, double floor,
                     float *d_var, float *d_rho, unsigned long long *d_stats, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (samples_done < 2 || samples_done > params->samples)
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise: samples_done must be in [2, samples]");
    if (!(floor > 0.0) || !(rel_error >= 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise: floor must be > 0 and rel_error >= 0");
    if ((rc = refuse_after_adaptive(ctx, "noise")))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true)) || (rc = check_moments(ctx, A, "noise")))
        return rc;
    A.samps = samples_done;
    A.acc = ctx->d_acc;
    const long long pixels = (long long)A.slab_rows * A.W;
    if (pixels <= 0 || (!d_var && !d_rho && !d_stats))
        return PTG_OK;
    noise_kernel<<<strided_blocks(pixels), 256, 0, s>>>(A, ctx->d_acc2, rel_error, floor, d_var, d_rho, d_stats);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_read_moments_device(ptg_context *ctx, const ptg_params *params, unsigned long long *d_sum,
                            unsigned long long *d_sumsq, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/true)))
        return rc;
    const size_t bytes = acc_elems_for(A) * sizeof(unsigned long long);
    if (d_sumsq) {
        if ((rc = check_moments(ctx, A, "read_moments")))
            return rc;
        PTG_HIP(hipMemcpyAsync(d_sumsq, ctx->d_acc2, bytes, hipMemcpyDeviceToDevice, s));
    }
    if (d_sum)
        PTG_HIP(hipMemcpyAsync(d_sum, ctx->d_acc, bytes, hipMemcpyDeviceToDevice, s));
    return PTG_OK;
}

int ptg_set_active_mask_device(ptg_context *ctx, const ptg_params *params, const uint8_t *d_mask,
                               unsigned long long *d_info, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "set_active_mask")))
        return rc;
    return build_list(ctx, params, A, d_mask, 0, d_info, nullptr, s);
}

int ptg_select_active_device(ptg_context *ctx, const ptg_params *params, double rel_error, double floor,
                             int32_t dilate, float *d_rho, unsigned long long *d_stats, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (!(floor > 0.0) || !(rel_error >= 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, "select_active: floor must be > 0 and rel_error >= 0");
    if (dilate < 0 || dilate > 8)
        return fail(PTG_ERR_INVALID_ARGUMENT, "select_active: dilate must be in [0, 8]");
    if (dilate > 0 && params->shard_count > 1)
        return fail(PTG_ERR_UNSUPPORTED, "select_active: dilate > 0 needs shard_count 1 (the neighbouring rows "
                                         "live in other shards)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "select_active")))
        return rc;
    const long long pixels = (long long)A.slab_rows * A.W;
    select_over_kernel<<<strided_blocks(pixels), 256, 0, s>>>(A, ctx->d_acc2, ctx->d_counts, rel_error, floor,
                                                               ctx->d_over, d_rho, d_stats);
    PTG_HIP(hipGetLastError());
    return build_list(ctx, params, A, ctx->d_over, dilate, nullptr, d_stats, s);
}

int ptg_select_over_device(ptg_context *ctx, const ptg_params *params, double rel_error, double floor,
                           uint8_t *d_over, float *d_rho, unsigned long long *d_stats, void *stream)
{
    if (!ctx || !d_over)
        return fail(PTG_ERR_INVALID_ARGUMENT, "select_over: NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (!(floor > 0.0) || !(rel_error >= 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, "select_over: floor must be > 0 and rel_error >= 0");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "select_over")))
        return rc;
    const long long pixels = (long long)A.slab_rows * A.W;
    select_over_kernel<<<strided_blocks(pixels), 256, 0, s>>>(A, ctx->d_acc2, ctx->d_counts, rel_error, floor, d_over,
                                                               d_rho, d_stats);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_noise_active_device(ptg_context *ctx, const ptg_params *params, double floor, float *d_var, float *d_rho,
                            void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (!(floor > 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise_active: floor must be > 0");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "noise_active")))
        return rc;
    const long long pixels = (long long)A.slab_rows * A.W;
    if (pixels <= 0 || (!d_var && !d_rho))
        return PTG_OK;
    noise_active_kernel<<<strided_blocks(pixels), 256, 0, s>>>(A, ctx->d_acc2, ctx->d_counts, floor, d_var, d_rho);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_set_active_gathered_device(ptg_context *ctx, const ptg_params *params, const uint8_t *d_over_gathered,
                                   int32_t dilate, unsigned long long *d_stats, void *stream)
{
    if (!ctx || !d_over_gathered)
        return fail(PTG_ERR_INVALID_ARGUMENT, "set_active_gathered: NULL context or over bytes");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (dilate < 0 || dilate > kMaxDilate)
        return fail(PTG_ERR_INVALID_ARGUMENT, "set_active_gathered: dilate must be in [0, 8]");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "set_active_gathered")))
        return rc;
    return build_list(ctx, params, A, d_over_gathered, dilate, nullptr, d_stats, s, /*gathered=*/true);
}

int ptg_accumulate_active_device(ptg_context *ctx, const ptg_params *params, int32_t add_samples, long long max_units,
                                 unsigned long long *d_segments, void *stream)
{
    if (!ctx)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (add_samples < 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "accumulate_active: add_samples must be >= 0");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "accumulate_active")))
        return rc;
    if (!ctx->list_valid)
        return fail(PTG_ERR_INVALID_ARGUMENT, "accumulate_active: no active list since the last reset "
                                              "(ptg_set_active_mask_device or ptg_select_active_device first)");
    if (!same_slab(ctx->list_frame, *params))
        return fail(PTG_ERR_INVALID_ARGUMENT, "accumulate_active: the active list was built for another frame");
    if (ctx->adaptive_added + add_samples > (1LL << 30))
        return fail(PTG_ERR_INVALID_ARGUMENT, "accumulate_active: a sample count could pass 2^30 (" +
                                                  std::to_string(ctx->adaptive_added) + " added since the last reset)");
    if (add_samples == 0)
        return PTG_OK;
    const long long bound = max_units <= 0 || max_units > A.n_groups ? (long long)A.n_groups : max_units;
    ActivePlan P;
    if ((rc = plan_active(A.n > kLinearMax, ctx->wave_slots, bound, add_samples, params->chunk_samples, P)))
        return rc;
    // the kernel's frame: local samples [0, add_samples) in chunks of P.chunk, every unit accumulates
    A.sample_begin = 0;
    A.sample_end = add_samples;
    plan_single_level(A, P.chunk, add_samples, /*one_shot=*/false);
    A.n_units = P.n_units;
    A.segments = d_segments;
    const GatherArgs G{ctx->d_units, ctx->d_list, ctx->d_counts, ctx->d_rec, bound, P.n_chunks};
    ctx->acc_dirty = true;
    ctx->adaptive_pass = ctx->moments_pass = true;
    ctx->adaptive_added += add_samples;
    if ((rc = launch_pool(A, P.grid, d_segments != nullptr, s, ctx->d_acc2, &G)))
        return rc;
    bump_counts_kernel<<<strided_blocks(bound, /*per_block=*/4), 256, 0, s>>>(  // a wave per unit
        A.W, ctx->d_units, ctx->d_list, ctx->d_rec, bound, add_samples, ctx->d_counts);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_resolve_active_device(ptg_context *ctx, const ptg_params *params, float *d_slab, void *stream)
{
    if (!ctx || !d_slab)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "resolve_active")))
        return rc;
    A.out = d_slab;
    const long long pixels = (long long)A.slab_rows * A.W;
    if (pixels <= 0)
        return PTG_OK;
    resolve_active_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, s>>>(A, ctx->d_counts);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_read_sample_counts_device(ptg_context *ctx, const ptg_params *params, int32_t *d_counts, void *stream)
{
    if (!ctx || !d_counts)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL context or output");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    if ((rc = begin_adaptive(ctx, params, A, s, "read_sample_counts")))
        return rc;
    PTG_HIP(hipMemcpyAsync(d_counts, ctx->d_counts, (size_t)A.slab_rows * A.W * sizeof(int32_t),
                           hipMemcpyDeviceToDevice, s));
    return PTG_OK;
}

int ptg_noise_schedule(int32_t min_samples, int32_t samples, int32_t *ends, int32_t cap, int32_t *n)
{
    if (!ends || !n)
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise_schedule: NULL argument");
    *n = 0;
    if (min_samples < 2 || samples < 2)
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise_schedule: min_samples and samples must be >= 2 (a variance "
                                              "needs two samples)");
    int32_t k = 0;
    for (int64_t e = min_samples; e < samples; e *= 2, ++k)
        if (k < cap)
            ends[k] = (int32_t)e;
    if (k < cap)
        ends[k] = samples;
    ++k;
    if (k > cap)
        return fail(PTG_ERR_INVALID_ARGUMENT, "noise_schedule: " + std::to_string(k) + " passes, room for " +
                                                  std::to_string(cap));
    *n = k;
    return PTG_OK;
}

int ptg_trace_samples_device(ptg_context *ctx, const ptg_params *params, const int32_t *d_coords, size_t n,
                             float *d_out, int32_t *d_segs, void *stream)
{
    if (!ctx || (n && (!d_coords || !d_out || !d_segs)))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (n == 0)
        return PTG_OK;
    if (params->flags & PTG_FLAG_REFERENCE_F64)
        return fail(PTG_ERR_UNSUPPORTED, "trace_samples probes the fp32 kernel");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/false)))
        return rc;
    int blocks = (int)((n + kTraceBlock - 1) / kTraceBlock);
    const bool bvh = A.n > kLinearMax;
    // one of 16: trace_strat or trace_kernel, with lights to sample or without (launch_pool's rule)
    with_bool(A.stratified != 0, [&](auto st) {
        with_bool(A.n_lights > 0, [&](auto ls) {
            with_bool(bvh, [&](auto bv) {
                with_bool(A.exact_math != 0, [&](auto ex) {
                    constexpr bool kB = decltype(bv)::value, kE = decltype(ex)::value, kL = decltype(ls)::value;
                    if constexpr (decltype(st)::value)
                        trace_strat<kB, kE, kL><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs);
                    else
                        trace_kernel<kB, kE, kL><<<blocks, kTraceBlock, 0, s>>>(A, d_coords, (int)n, d_out, d_segs);
                });
            });
        });
    });
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_sampler_pairs_device(ptg_context *ctx, const ptg_params *params, const int32_t *d_coords, size_t n,
                             uint32_t *d_out, void *stream)
{
    if (!ctx || (n && (!d_coords || !d_out)))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = check_params(params);
    if (rc)
        return rc;
    if (n > (size_t)INT32_MAX / 8)
        return fail(PTG_ERR_UNSUPPORTED, "too many records");
    if (n == 0)
        return PTG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    int grid = 0;
    if ((rc = begin_launch(ctx, params, A, grid, s, /*with_acc=*/false)))
        return rc;
    sampler_pairs_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(A, d_coords, (int)n, d_out);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_features_device(ptg_context *ctx, const ptg_params *params, float *d_feat, void *stream)
{
    if (!ctx || !d_feat)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: NULL context or output");
    if (reinterpret_cast<uintptr_t>(d_feat) % 16)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: the output must be 16-byte aligned");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    unsigned blocks = 0;
    if ((rc = begin_features(ctx, params, A, blocks, s)))
        return rc;
    if (A.n > kLinearMax)
        features_kernel<true><<<blocks, 256, 0, s>>>(A, reinterpret_cast<float4 *>(d_feat));
    else
        features_kernel<false><<<blocks, 256, 0, s>>>(A, reinterpret_cast<float4 *>(d_feat));
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_features_follow_device(ptg_context *ctx, const ptg_params *params, int32_t max_bounces, float *d_feat,
                               void *stream)
{
    if (max_bounces < 0 || max_bounces > PTG_MAX_FOLLOW_BOUNCES)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: max_bounces must be 0..16");
    if (!ctx || !d_feat)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: NULL context or output");
    if (reinterpret_cast<uintptr_t>(d_feat) % 16)
        return fail(PTG_ERR_INVALID_ARGUMENT, "features: the output must be 16-byte aligned");
    int rc = check_params(params);
    if (rc)
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KArgs A;
    unsigned blocks = 0;
    if ((rc = begin_features(ctx, params, A, blocks, s)))
        return rc;
    if (A.n > kLinearMax)
        features_follow_kernel<true><<<blocks, 256, 0, s>>>(A, max_bounces, reinterpret_cast<float4 *>(d_feat));
    else
        features_follow_kernel<false><<<blocks, 256, 0, s>>>(A, max_bounces, reinterpret_cast<float4 *>(d_feat));
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_math_probe_device(ptg_context *ctx, int32_t op, int32_t exact, const float *d_in, float *d_out, size_t n,
                          void *stream)
{
    if (!ctx || (n && (!d_in || !d_out)))
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (op < PTG_PROBE_SQRT || op > PTG_PROBE_SINCOS)
        return fail(PTG_ERR_INVALID_ARGUMENT, "unknown probe op");
    if (n > (size_t)INT32_MAX / 2)
        return fail(PTG_ERR_UNSUPPORTED, "too many operands");
    if (n == 0)
        return PTG_OK;
    PTG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (exact)
        math_probe_kernel<true><<<blocks, 256, 0, s>>>(op, d_in, d_out, (int)n, ctx->d_trig);
    else
        math_probe_kernel<false><<<blocks, 256, 0, s>>>(op, d_in, d_out, (int)n, ctx->d_trig);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_unshard_device(const float *d_gathered, float *d_image, int32_t width, int32_t height, int32_t band_rows,
                       int32_t shard_count, void *stream)
{
    if (!d_gathered || !d_image || width <= 0 || height <= 0 || band_rows <= 0 || shard_count <= 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "invalid unshard arguments");
    if (height > 65535)
        return fail(PTG_ERR_UNSUPPORTED, "height > 65535");
    int32_t slab_rows = 0;
    ptg_shard_rows(height, band_rows, shard_count, &slab_rows);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int bx = std::max(1, std::min(64, (width * 3 + 255) / 256));
    unshard_kernel<<<dim3(bx, height), 256, 0, s>>>(d_gathered, d_image, width, band_rows, shard_count, slab_rows);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_tonemap_device(const float *d_image, uint8_t *d_out, size_t count, void *stream)
{
    if (!d_image || !d_out)
        return fail(PTG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (count == 0)
        return PTG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    size_t blocks = (count + 255) / 256;
    tonemap_kernel<<<(unsigned)blocks, 256, 0, s>>>(d_image, d_out, count);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

int ptg_render(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
               int device, double *image_rgb)
{
    if (!image_rgb)
        return fail(PTG_ERR_INVALID_ARGUMENT, "image is NULL");
    int rc = check_params(params);
    if (rc)
        return rc;
    ptg_context *ctx = nullptr;
    rc = ptg_context_create(spheres, n_spheres, cam, device, &ctx);
    if (rc)
        return rc;
    KArgs A;  // the frame's plan: the slab's geometry (and the reference-arithmetic mode's launch)
    int grid = 0;
    if ((rc = check_lights(ctx, params)) || (rc = fill_launch(ctx->base, ctx->wave_slots, params, A, grid))) {
        ptg_context_destroy(ctx);
        return rc;
    }
    const int slab_rows = A.slab_rows;
    size_t slab_elems = (size_t)slab_rows * params->width * 3;
    // the reference-arithmetic mode keeps its doubles to the host image
    const bool f64 = (params->flags & PTG_FLAG_REFERENCE_F64) != 0;
    const size_t esz = f64 ? sizeof(double) : sizeof(float);
    void *d_slab = nullptr;
    std::vector<unsigned char> host(slab_elems * esz);
    rc = PTG_OK;
    if (hipMalloc(&d_slab, slab_elems * esz) != hipSuccess) {
        ptg_context_destroy(ctx);
        return fail(PTG_ERR_OUT_OF_MEMORY, "hipMalloc of the image slab failed");
    }
    if (f64)
        rc = launch_ref64(ctx, A, static_cast<double *>(d_slab), nullptr, nullptr, nullptr);
    else
        rc = ptg_render_device(ctx, params, static_cast<float *>(d_slab), nullptr, nullptr);
    if (rc == PTG_OK) {
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess)
            e = hipMemcpy(host.data(), d_slab, slab_elems * esz, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            rc = fail(PTG_ERR_HIP, std::string("render: ") + hipGetErrorString(e));
    }
    (void)hipFree(d_slab);
    ptg_context_destroy(ctx);
    if (rc)
        return rc;
    const int W = params->width, H = params->height;
    for (int j = 0; j < slab_rows; ++j) {
        const int r = out_row_of(A, j);
        if (r >= H)
            continue;
        double *dst = image_rgb + (size_t)r * W * 3;
        const size_t off = (size_t)j * W * 3;
        if (f64)
            ptg_frames::add_image(dst, reinterpret_cast<const double *>(host.data()) + off, (size_t)W * 3);
        else
            ptg_frames::add_image(dst, reinterpret_cast<const float *>(host.data()) + off, (size_t)W * 3);
    }
    return PTG_OK;
}

}  // extern "C"
