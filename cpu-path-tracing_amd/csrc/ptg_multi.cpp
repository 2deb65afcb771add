// ptg_multi.cpp -- single-process multi-GPU frames: the
// drop-in ptg_render over several devices of one node, one RCCL gather.
//
// Replaces the taskflow row loop (src/main.cpp:214-236) for a C++ caller that
// owns several GPUs in one process (host/main.cpp --devices): device k renders
// the interleaved row bands b with b % n == k into a contiguous slab
// (ptg_render_device / ptg_resolve_device, shard_rank = k), ONE ncclGather
// (rccl.h:745, over xGMI between MI355X devices) collects the slabs on the
// first device, and ptg_unshard_device restores the row order there.  The RNG
// is keyed by the global pixel, so the image equals the one-device frame bit
// for bit.
//
// A ptg_multi holds, per device, the scene in HBM (a ptg_context), a
// non-blocking stream and the slab, the RCCL communicator of the device set
// (ncclCommInitAll once), and on the root the gathered slabs and the image:
// repeated frames and progressive passes reuse all of it.  ptg_render_multi is
// create + render + destroy.  The multi-process path (one rank per GPU,
// torch.distributed on RCCL) is ptgpu.render_sharded; all three use the same
// slab layout and un-shard kernel.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ptgpu.h"
#include "frame_passes.hpp"  // the drivers' checks, pass loops and report fillers; fail() (ptg_last_error's channel)

// csrc/ptg_denoise.hip: the filter parameters a driver runs with (NULL: the
// defaults; the camera's pixel_spread where none is given), checked
extern "C" int ptg_denoise_params_for_(const ptg_camera *cam, int32_t width, int32_t height,
                                       const ptg_denoise_params *denoise, ptg_denoise_params *out);
extern "C" int ptg_features_for_(ptg_context *ctx, const ptg_params *params, const ptg_denoise_params *k,
                                 float *d_feat, void *stream);

namespace {

using namespace ptg_frames;

struct Shard {
    int id = -1;  // HIP device
    ptg_context *ctx = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;  // local transport: the slab is complete
    hipEvent_t t_begin = nullptr, t_rendered = nullptr;  // timing of the last device frame
    float *slab = nullptr;
    size_t slab_cap = 0;  // floats
    float *var = nullptr;  // denoised frames: the variance slab, laid out like the slab
    size_t var_cap = 0;
    unsigned long long *counters = nullptr;  // PTG_FLAG_COUNT_TESTS: 4 per shard
    ncclComm_t comm = nullptr;
    bool stuck = false;  // destroy(): a broken group's stream did not drain
    // noise-target and adaptive frames (reserve_adaptive): this shard's over
    // bytes (also the staging of a host mask), every shard's after the
    // all-gather (rank-major), the 6 statistics + 4 kernel counters, the
    // sample counts read back
    uint8_t *over = nullptr, *over_all = nullptr;
    unsigned long long *stats = nullptr;
    int32_t *cnt = nullptr;
    size_t ad_pixels = 0;  // slab pixels the four are sized for
    long long max_units = 0;  // the active units of the last select (0: the host-side bound)
};

constexpr int kStats = 10;  // per shard: 6 statistics, then 4 kernel counters

// Restores the calling thread's current HIP device on every return path.
struct DeviceGuard {
    int dev = -1;
    DeviceGuard()
    {
        if (hipGetDevice(&dev) != hipSuccess)
            dev = -1;
    }
    ~DeviceGuard()
    {
        if (dev >= 0)
            (void)hipSetDevice(dev);
    }
};

int hip_fail(const char *what, hipError_t e) { return fail(PTG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
int nccl_fail(const char *what, ncclResult_t r)
{
    return fail(PTG_ERR_HIP, std::string(what) + ": " + ncclGetErrorString(r));
}

#define MULTI_HIP(call)                                                                                 \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return hip_fail(#call, e_);                                                                 \
    } while (0)

}  // namespace

struct ptg_multi {
    std::vector<Shard> shards;
    bool rccl = false;  // false: n shards on one device, gathered by device copies (tests)
    float *gathered = nullptr;  // root: n slabs, rank-major
    size_t gathered_cap = 0;
    float *image = nullptr;  // root: the un-sharded frame
    size_t image_cap = 0;
    std::vector<float> host;
    hipEvent_t t_unsharded = nullptr;  // root: the frame is un-sharded
    // the events and the image hold a completed ptg_multi_frame_device of this
    // size; cleared by every other frame call (render, passes, resolve), which
    // write the image or start frames the events do not describe
    bool timed = false;
    int32_t frame_w = 0, frame_h = 0, frame_band_rows = 0;
    // a failure inside the RCCL group: the communicators were aborted and the
    // context refuses further frames (PTG_ERR_HIP) until destroyed
    bool broken = false;
    int inject_gather_fault = -1;  // tests: fail ncclGather at this shard
    // noise-target and adaptive frames: every shard's statistics land here
    // (pinned, kStats per shard) with one synchronisation per pass
    unsigned long long *host_stats = nullptr;
    std::vector<uint8_t> host_mask;
    std::vector<int32_t> host_cnt;
    // denoised frames (reserve_denoise): the camera (the filter's pixel_spread)
    // and ONE allocation on the root, sized on first use: the gathered
    // variance slabs, the un-sharded variance, the filtered frame, the whole
    // frame's features and the filter's scratch
    ptg_camera cam{};
    float *dn_buf = nullptr;
    size_t dn_cap = 0;  // floats
    float *var_gathered = nullptr, *var_image = nullptr, *filtered = nullptr, *feat = nullptr, *dn_scratch = nullptr;
    size_t dn_scratch_bytes = 0;
};

namespace {

int destroy(ptg_multi *m)
{
    if (!m)
        return PTG_OK;
    DeviceGuard g;
    // Every stream is drained before its buffers are freed -- a broken
    // group's too, since a failed frame's render kernels may still be running
    // on the slabs.  A broken group's communicators were aborted when the
    // group failed, which should release every queued gather; its streams are
    // still drained with a bounded wait, so a peer that never returns cannot
    // hang close(): after ~10 s that shard's buffers are leaked, not freed
    // under a running kernel, and the call reports PTG_ERR_HIP.
    int rc = PTG_OK;
    for (Shard &s : m->shards) {
        if (s.id < 0)
            continue;
        (void)hipSetDevice(s.id);
        if (!s.stream)
            continue;
        if (!m->broken) {
            (void)hipStreamSynchronize(s.stream);
            continue;
        }
        const auto t0 = std::chrono::steady_clock::now();
        while (hipStreamQuery(s.stream) == hipErrorNotReady) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
                s.stuck = true;
                rc = PTG_ERR_HIP;
                break;
            }
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
    }
    bool any_stuck = false;
    for (Shard &s : m->shards) {
        if (s.id < 0)
            continue;
        (void)hipSetDevice(s.id);
        if (s.comm)
            (void)(m->broken ? ncclCommAbort(s.comm) : ncclCommDestroy(s.comm));
        if (s.stuck) {  // still running after the abort: leak its buffers
            any_stuck = true;
            continue;
        }
        if (s.slab)
            (void)hipFree(s.slab);
        if (s.var)
            (void)hipFree(s.var);
        if (s.counters)
            (void)hipFree(s.counters);
        for (void *q : {(void *)s.over, (void *)s.over_all, (void *)s.stats, (void *)s.cnt})
            if (q)
                (void)hipFree(q);
        if (s.done)
            (void)hipEventDestroy(s.done);
        if (s.t_begin)
            (void)hipEventDestroy(s.t_begin);
        if (s.t_rendered)
            (void)hipEventDestroy(s.t_rendered);
        if (s.stream)
            (void)hipStreamDestroy(s.stream);
        if (s.ctx)
            (void)ptg_context_destroy(s.ctx);
    }
    if (!any_stuck && !m->shards.empty() && m->shards[0].id >= 0) {
        (void)hipSetDevice(m->shards[0].id);
        if (m->gathered)
            (void)hipFree(m->gathered);
        if (m->image)
            (void)hipFree(m->image);
        if (m->dn_buf)
            (void)hipFree(m->dn_buf);
        if (m->t_unsharded)
            (void)hipEventDestroy(m->t_unsharded);
    }
    if (!any_stuck && m->host_stats)
        (void)hipHostFree(m->host_stats);
    delete m;
    return rc == PTG_OK ? PTG_OK : fail(rc, "multi: a broken group's stream did not drain within 10 s; its buffers were leaked");
}

int create(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const int *devices, int n, bool rccl,
           ptg_multi **out)
{
    if (!out)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi: out is NULL");
    *out = nullptr;
    if (!devices || n < 1)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi: no device");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PTG_ERR_NO_DEVICE, "no HIP device visible");
    for (int k = 0; k < n; ++k) {
        if (devices[k] < 0 || devices[k] >= count)
            return fail(PTG_ERR_INVALID_ARGUMENT, "multi: device ordinal out of range");
        for (int j = 0; j < k && rccl; ++j)
            if (devices[j] == devices[k])
                return fail(PTG_ERR_UNSUPPORTED, "render_multi: RCCL needs distinct devices (one rank per GPU)");
    }
    DeviceGuard g;
    ptg_multi *m = new ptg_multi();
    m->rccl = rccl;
    if (cam)
        m->cam = *cam;
    m->shards.resize(n);
    int rc = PTG_OK;
    for (int k = 0; k < n && rc == PTG_OK; ++k) {
        Shard &s = m->shards[k];
        s.id = devices[k];
        if ((rc = ptg_context_create(spheres, n_spheres, cam, s.id, &s.ctx)))
            break;
        hipError_t e = hipSetDevice(s.id);
        if (e == hipSuccess)
            e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        if (e == hipSuccess)
            e = hipEventCreate(&s.t_begin);
        if (e == hipSuccess)
            e = hipEventCreate(&s.t_rendered);
        if (e == hipSuccess && k == 0)
            e = hipEventCreate(&m->t_unsharded);
        if (e != hipSuccess)
            rc = hip_fail("multi: stream/event", e);
    }
    if (rc == PTG_OK && rccl) {
        std::vector<ncclComm_t> cm(n);
        const ncclResult_t r = ncclCommInitAll(cm.data(), n, devices);
        if (r != ncclSuccess)
            rc = nccl_fail("ncclCommInitAll", r);
        else
            for (int k = 0; k < n; ++k)
                m->shards[k].comm = cm[k];
    }
    if (rc != PTG_OK) {
        destroy(m);
        return rc;
    }
    *out = m;
    return PTG_OK;
}

// the part of check_frame that needs no context (the one-shot wrappers check
// their arguments before they create one)
int check_frame_params(const ptg_params *p)
{
    if (p->width <= 0 || p->height <= 0 || p->band_rows < 1)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi: width, height and band_rows must be positive");
    if (p->shard_count != 1 || p->shard_rank != 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "render_multi shards the whole frame itself: shard_count must be 1");
    if (p->flags & PTG_FLAG_REFERENCE_F64)
        return fail(PTG_ERR_UNSUPPORTED, "render_multi renders the fp32 kernel only (the reference-arithmetic "
                                         "mode keeps doubles: use ptg_render)");
    return PTG_OK;
}

int check_frame(const ptg_multi *m, const ptg_params *p)
{
    if (!m || !p)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi: NULL context or params");
    if (m->broken)
        return fail(PTG_ERR_HIP, "multi: the context's RCCL group failed earlier and its communicators were "
                                 "aborted; destroy it");
    return check_frame_params(p);
}

// params of shard k
ptg_params shard_params(const ptg_params *p, int k, int n)
{
    ptg_params q = *p;
    q.shard_rank = k;
    q.shard_count = n;
    return q;
}

// buffers for a frame of this size (grown, never shrunk)
int reserve(ptg_multi *m, const ptg_params *p, size_t &slab_elems)
{
    const int n = (int)m->shards.size();
    int32_t rows = 0;
    int rc = ptg_shard_rows(p->height, p->band_rows, n, &rows);
    if (rc)
        return rc;
    slab_elems = (size_t)rows * p->width * 3;
    const size_t image_elems = (size_t)p->width * p->height * 3;
    for (Shard &s : m->shards) {
        if (s.slab_cap >= slab_elems)
            continue;
        MULTI_HIP(hipSetDevice(s.id));
        if (s.slab) {
            MULTI_HIP(hipStreamSynchronize(s.stream));
            MULTI_HIP(hipFree(s.slab));
            s.slab = nullptr;
            s.slab_cap = 0;
        }
        if (hipMalloc(&s.slab, slab_elems * sizeof(float)) != hipSuccess)
            return fail(PTG_ERR_OUT_OF_MEMORY, "multi: hipMalloc of a slab failed");
        s.slab_cap = slab_elems;
    }
    Shard &r = m->shards[0];
    MULTI_HIP(hipSetDevice(r.id));
    if (m->gathered_cap < (size_t)n * slab_elems) {
        MULTI_HIP(hipStreamSynchronize(r.stream));
        if (m->gathered)
            MULTI_HIP(hipFree(m->gathered));
        m->gathered = nullptr;
        m->gathered_cap = 0;
        if (hipMalloc(&m->gathered, (size_t)n * slab_elems * sizeof(float)) != hipSuccess)
            return fail(PTG_ERR_OUT_OF_MEMORY, "multi: hipMalloc of the gather buffer failed");
        m->gathered_cap = (size_t)n * slab_elems;
    }
    if (m->image_cap < image_elems) {
        MULTI_HIP(hipStreamSynchronize(r.stream));
        if (m->image)
            MULTI_HIP(hipFree(m->image));
        m->image = nullptr;
        m->image_cap = 0;
        if (hipMalloc(&m->image, image_elems * sizeof(float)) != hipSuccess)
            return fail(PTG_ERR_OUT_OF_MEMORY, "multi: hipMalloc of the image failed");
        m->image_cap = image_elems;
    }
    m->host.resize(image_elems);
    return PTG_OK;
}

// One RCCL group over the shards: call(k, shard) queues shard k's collective
// (`what` names it in the error).  Every device is made current once BEFORE
// the group opens, so that inside it only the collective calls can fail; the
// group is closed on every path, and after a failure the communicators are
// aborted and the context refuses further frames.
template <class Call>
int rccl_group(ptg_multi *m, const char *what, Call &&call)
{
    const int n = (int)m->shards.size();
    for (int k = n - 1; k >= 0; --k)
        MULTI_HIP(hipSetDevice(m->shards[k].id));
    ncclResult_t r = ncclGroupStart();
    if (r != ncclSuccess)
        return nccl_fail("ncclGroupStart", r);
    int rc = PTG_OK;
    for (int k = 0; k < n && rc == PTG_OK; ++k) {
        Shard &s = m->shards[k];
        (void)hipSetDevice(s.id);
        r = call(k, s);
        if (r != ncclSuccess)
            rc = nccl_fail(what, r);
    }
    // the group is closed on every path (an error inside it must not leave
    // this thread's RCCL group open) ...
    const ncclResult_t re = ncclGroupEnd();
    if (rc != PTG_OK || re != ncclSuccess) {
        // ... but a partial group must not run without its peers: the
        // queued collectives are aborted with the communicators, and the
        // context refuses further frames
        m->broken = true;
        for (Shard &s : m->shards)
            if (s.comm) {
                (void)hipSetDevice(s.id);
                (void)ncclCommAbort(s.comm);
                s.comm = nullptr;
            }
        return rc != PTG_OK ? rc : nccl_fail("ncclGroupEnd", re);
    }
    return PTG_OK;
}

// ONE gather of the equal-size slabs to the root (RCCL: one ncclGather per
// rank inside a group, rank-major on the root -- rccl.h:745; local shards: the
// same layout by device copies after each shard's slab is complete) and the
// un-shard there, queued on the root's stream (asynchronous).  variance: the
// shards' variance slabs into the root's variance frame instead (denoised
// frames: the same layout, the same path).
int gather_unshard_device(ptg_multi *m, const ptg_params *p, size_t slab_elems, bool variance = false)
{
    const int n = (int)m->shards.size();
    Shard &root = m->shards[0];
    float *const gathered = variance ? m->var_gathered : m->gathered;
    float *const image = variance ? m->var_image : m->image;
    if (m->rccl) {
        const int rc = rccl_group(m, "ncclGather", [&](int k, Shard &s) {
            return k == m->inject_gather_fault
                       ? ncclInvalidArgument
                       : ncclGather(variance ? s.var : s.slab, k == 0 ? gathered : nullptr, slab_elems, ncclFloat, 0,
                                    s.comm, s.stream);
        });
        if (rc)
            return rc;
        MULTI_HIP(hipSetDevice(root.id));
    } else {
        MULTI_HIP(hipSetDevice(root.id));
        for (int k = 0; k < n; ++k) {
            Shard &s = m->shards[k];
            MULTI_HIP(hipEventRecord(s.done, s.stream));
            MULTI_HIP(hipStreamWaitEvent(root.stream, s.done, 0));
            MULTI_HIP(hipMemcpyAsync(gathered + (size_t)k * slab_elems, variance ? s.var : s.slab,
                                     slab_elems * sizeof(float), hipMemcpyDeviceToDevice, root.stream));
        }
    }
    return ptg_unshard_device(gathered, image, p->width, p->height, p->band_rows, n, root.stream);
}

// waits for every shard's stream (root last: its part ends with the un-shard)
int sync_all(ptg_multi *m)
{
    for (int k = (int)m->shards.size() - 1; k >= 0; --k) {
        MULTI_HIP(hipSetDevice(m->shards[k].id));
        MULTI_HIP(hipStreamSynchronize(m->shards[k].stream));
    }
    return PTG_OK;
}

// gather + un-shard, then the image to the host (m->host).  Synchronous.
int gather_unshard(ptg_multi *m, const ptg_params *p, size_t slab_elems)
{
    int rc = gather_unshard_device(m, p, slab_elems);
    if (rc)
        return rc;
    Shard &root = m->shards[0];
    const size_t image_elems = (size_t)p->width * p->height * 3;
    MULTI_HIP(hipSetDevice(root.id));
    MULTI_HIP(hipMemcpyAsync(m->host.data(), m->image, image_elems * sizeof(float), hipMemcpyDeviceToHost,
                             root.stream));
    return sync_all(m);
}

// ---- noise-target and adaptive frames (include/ptgpu.h "several GPUs") ----
// The contexts' statistics are integers that add across shards ([2]: max), the
// sums are exact and the RNG is keyed by the global pixel: what is left to the
// host is to hand every shard the whole frame's over bytes and to decide for
// the frame.

// the per-shard byte slabs, statistics and count slab for a frame of this
// size (grown, never shrunk), the pinned statistics of all shards
int reserve_adaptive(ptg_multi *m, const ptg_params *p, size_t &slab_pixels)
{
    const int n = (int)m->shards.size();
    int32_t rows = 0;
    int rc = ptg_shard_rows(p->height, p->band_rows, n, &rows);
    if (rc)
        return rc;
    slab_pixels = (size_t)rows * p->width;
    for (Shard &s : m->shards) {
        if (s.ad_pixels >= slab_pixels)
            continue;
        MULTI_HIP(hipSetDevice(s.id));
        MULTI_HIP(hipStreamSynchronize(s.stream));
        for (void **q : {(void **)&s.over, (void **)&s.over_all, (void **)&s.stats, (void **)&s.cnt}) {
            if (*q)
                MULTI_HIP(hipFree(*q));
            *q = nullptr;
        }
        s.ad_pixels = 0;
        if (hipMalloc(&s.over, slab_pixels) != hipSuccess || hipMalloc(&s.over_all, (size_t)n * slab_pixels) != hipSuccess ||
            hipMalloc(&s.stats, kStats * sizeof(unsigned long long)) != hipSuccess ||
            hipMalloc(&s.cnt, slab_pixels * sizeof(int32_t)) != hipSuccess)
            return fail(PTG_ERR_OUT_OF_MEMORY, "multi: hipMalloc of the adaptive-sampling slabs failed");
        MULTI_HIP(hipMemsetAsync(s.stats, 0, kStats * sizeof(unsigned long long), s.stream));
        s.ad_pixels = slab_pixels;
    }
    if (!m->host_stats &&
        hipHostMalloc(reinterpret_cast<void **>(&m->host_stats), (size_t)n * kStats * sizeof(unsigned long long)) != hipSuccess)
        return fail(PTG_ERR_OUT_OF_MEMORY, "multi: hipHostMalloc of the statistics failed");
    return PTG_OK;
}

// the first `count` statistics of every shard to the host: n asynchronous
// copies, then the pass's one synchronisation; the shards' values combined
// into out ([2]: max, the others add)
int read_stats(ptg_multi *m, int count, unsigned long long *out)
{
    const int n = (int)m->shards.size();
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        MULTI_HIP(hipSetDevice(s.id));
        MULTI_HIP(hipMemcpyAsync(m->host_stats + (size_t)k * kStats, s.stats, count * sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost, s.stream));
    }
    int rc = sync_all(m);
    if (rc)
        return rc;
    for (int i = 0; i < count; ++i)
        out[i] = 0;
    for (int k = 0; k < n; ++k)
        for (int i = 0; i < count; ++i) {
            const unsigned long long v = m->host_stats[(size_t)k * kStats + i];
            out[i] = i == 2 ? (out[i] > v ? out[i] : v) : out[i] + v;
        }
    return PTG_OK;
}

int multi_noise(ptg_multi *m, const ptg_params *p, int32_t samples_done, double rel_error, double floor,
                unsigned long long *stats)
{
    size_t slab_pixels = 0;
    int rc = reserve_adaptive(m, p, slab_pixels);
    if (rc)
        return rc;
    const int n = (int)m->shards.size();
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        MULTI_HIP(hipSetDevice(s.id));
        MULTI_HIP(hipMemsetAsync(s.stats, 0, 4 * sizeof(unsigned long long), s.stream));
        const ptg_params q = shard_params(p, k, n);
        if ((rc = ptg_noise_device(s.ctx, &q, samples_done, rel_error, floor, nullptr, nullptr, s.stats, s.stream)))
            return rc;
    }
    return read_stats(m, 4, stats);
}

// ONE all-gather of the shards' over bytes onto every device, rank-major
// (RCCL: one ncclAllGather per rank inside a group; local shards: the same
// layout by device copies after each shard's slab is complete)
int all_gather_over(ptg_multi *m, size_t slab_pixels)
{
    const int n = (int)m->shards.size();
    if (m->rccl)
        return rccl_group(m, "ncclAllGather", [&](int, Shard &s) {
            return ncclAllGather(s.over, s.over_all, slab_pixels, ncclUint8, s.comm, s.stream);
        });
    for (Shard &s : m->shards) {
        MULTI_HIP(hipSetDevice(s.id));
        MULTI_HIP(hipEventRecord(s.done, s.stream));
    }
    for (int j = 0; j < n; ++j) {
        Shard &d = m->shards[j];
        MULTI_HIP(hipSetDevice(d.id));
        for (int k = 0; k < n; ++k) {
            Shard &s = m->shards[k];
            if (k != j)
                MULTI_HIP(hipStreamWaitEvent(d.stream, s.done, 0));
            MULTI_HIP(hipMemcpyAsync(d.over_all + (size_t)k * slab_pixels, s.over, slab_pixels, hipMemcpyDeviceToDevice,
                                     d.stream));
        }
    }
    return PTG_OK;
}

int multi_select(ptg_multi *m, const ptg_params *p, double rel_error, double floor, int32_t dilate,
                 unsigned long long *stats)
{
    size_t slab_pixels = 0;
    int rc = reserve_adaptive(m, p, slab_pixels);
    if (rc)
        return rc;
    const int n = (int)m->shards.size();
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        MULTI_HIP(hipSetDevice(s.id));
        MULTI_HIP(hipMemsetAsync(s.stats, 0, 6 * sizeof(unsigned long long), s.stream));
        const ptg_params q = shard_params(p, k, n);
        if ((rc = ptg_select_over_device(s.ctx, &q, rel_error, floor, s.over, nullptr, s.stats, s.stream)))
            return rc;
    }
    if ((rc = all_gather_over(m, slab_pixels)))
        return rc;
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        const ptg_params q = shard_params(p, k, n);
        if ((rc = ptg_set_active_gathered_device(s.ctx, &q, s.over_all, dilate, s.stats, s.stream)))
            return rc;
    }
    unsigned long long st[6];
    if ((rc = read_stats(m, 6, st)))
        return rc;
    for (int k = 0; k < n; ++k) {
        // the shard's own unit count sizes its next pass (a shard without an
        // active unit: the smallest launch, not the host-side bound)
        const long long u = (long long)m->host_stats[(size_t)k * kStats + 5];
        m->shards[k].max_units = u > 0 ? u : 1;
    }
    if (stats)
        std::copy(st, st + 6, stats);
    return PTG_OK;
}

int multi_set_mask(ptg_multi *m, const ptg_params *p, const uint8_t *mask)
{
    size_t slab_pixels = 0;
    int rc = reserve_adaptive(m, p, slab_pixels);
    if (rc)
        return rc;
    const int n = (int)m->shards.size();
    const int W = p->width, H = p->height, br = p->band_rows;
    if (mask) {
        m->host_mask.assign((size_t)n * slab_pixels, 0);
        for (int r = 0; r < H; ++r) {
            const int band = r / br;
            const size_t slab_row = (size_t)(band / n) * br + (size_t)(r - band * br);
            std::memcpy(m->host_mask.data() + (size_t)(band % n) * slab_pixels + slab_row * W, mask + (size_t)r * W, W);
        }
    }
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        const ptg_params q = shard_params(p, k, n);
        if (mask) {
            MULTI_HIP(hipSetDevice(s.id));
            MULTI_HIP(hipMemcpyAsync(s.over, m->host_mask.data() + (size_t)k * slab_pixels, slab_pixels,
                                     hipMemcpyHostToDevice, s.stream));
        }
        if ((rc = ptg_set_active_mask_device(s.ctx, &q, mask ? s.over : nullptr, nullptr, s.stream)))
            return rc;
        s.max_units = 0;  // the host-side bound
    }
    return mask ? sync_all(m) : PTG_OK;  // (the staging buffers may be reused)
}

int multi_accumulate_active(ptg_multi *m, const ptg_params *p, int32_t add_samples, bool count)
{
    const int n = (int)m->shards.size();
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        const ptg_params q = shard_params(p, k, n);
        const int rc = ptg_accumulate_active_device(s.ctx, &q, add_samples, s.max_units, count ? s.stats + 6 : nullptr,
                                                    s.stream);
        if (rc)
            return rc;
    }
    return PTG_OK;
}

// the sums resolved into m->host: at samples_done, or (active) each pixel at its own count
int multi_resolve(ptg_multi *m, const ptg_params *p, int32_t samples_done, bool active = false)
{
    size_t slab_elems = 0;
    int rc = reserve(m, p, slab_elems);
    if (rc)
        return rc;
    const int n = (int)m->shards.size();
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        const ptg_params q = shard_params(p, k, n);
        if ((rc = active ? ptg_resolve_active_device(s.ctx, &q, s.slab, s.stream)
                         : ptg_resolve_device(s.ctx, &q, samples_done, s.slab, s.stream)))
            return rc;
    }
    return gather_unshard(m, p, slab_elems);
}

int multi_read_counts(ptg_multi *m, const ptg_params *p, int32_t *counts)
{
    size_t slab_pixels = 0;
    int rc = reserve_adaptive(m, p, slab_pixels);
    if (rc)
        return rc;
    const int n = (int)m->shards.size();
    m->host_cnt.resize((size_t)n * slab_pixels);
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        const ptg_params q = shard_params(p, k, n);
        if ((rc = ptg_read_sample_counts_device(s.ctx, &q, s.cnt, s.stream)))
            return rc;
        MULTI_HIP(hipSetDevice(s.id));
        MULTI_HIP(hipMemcpyAsync(m->host_cnt.data() + (size_t)k * slab_pixels, s.cnt, slab_pixels * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, s.stream));
    }
    if ((rc = sync_all(m)))
        return rc;
    const int W = p->width, br = p->band_rows;
    for (int r = 0; r < p->height; ++r) {  // the un-shard, on the host
        const int band = r / br;
        const size_t slab_row = (size_t)(band / n) * br + (size_t)(r - band * br);
        std::memcpy(counts + (size_t)r * W, m->host_cnt.data() + (size_t)(band % n) * slab_pixels + slab_row * W,
                    (size_t)W * sizeof(int32_t));
    }
    return PTG_OK;
}

// ---- denoised frames (include/ptgpu.h "denoising on several GPUs") ----
// Every input of the filter is bit-identical across shardings -- the colour
// and the variance come from exact sums, the features depend on the scene, the
// camera and the global pixel only -- and the filter is a fixed fp32 sequence
// run once, on the root, over the un-sharded frames: the filtered image equals
// the one-device driver's bit for bit.

// every shard's variance slab and the root's frames for a frame of this size
// (after reserve(); grown, never shrunk; freed in destroy())
int reserve_denoise(ptg_multi *m, const ptg_params *p, size_t slab_elems)
{
    const int n = (int)m->shards.size();
    for (Shard &s : m->shards) {
        if (s.var_cap >= slab_elems)
            continue;
        MULTI_HIP(hipSetDevice(s.id));
        if (s.var) {
            MULTI_HIP(hipStreamSynchronize(s.stream));
            MULTI_HIP(hipFree(s.var));
            s.var = nullptr;
            s.var_cap = 0;
        }
        if (hipMalloc(&s.var, slab_elems * sizeof(float)) != hipSuccess)
            return fail(PTG_ERR_OUT_OF_MEMORY, "multi: hipMalloc of a variance slab failed");
        s.var_cap = slab_elems;
    }
    int32_t frame_rows = 0;  // of the whole frame as ONE shard: what the root's ptg_features_device call addresses
    size_t scratch_bytes = 0;
    int rc;
    if ((rc = ptg_shard_rows(p->height, p->band_rows, 1, &frame_rows)) ||
        (rc = ptg_denoise_scratch_bytes(p->width, p->height, &scratch_bytes)))
        return rc;
    // every part starts at a multiple of 64 floats (256 B: ptg_features_device stores float4)
    const auto part = [](size_t floats) { return (floats + 63) / 64 * 64; };
    const size_t gath = part((size_t)n * slab_elems), img = part((size_t)p->width * p->height * 3);
    const size_t feat = part((size_t)frame_rows * p->width * 12), scratch = part(scratch_bytes / sizeof(float));
    const size_t total = gath + 2 * img + feat + scratch;
    Shard &r = m->shards[0];
    MULTI_HIP(hipSetDevice(r.id));
    if (m->dn_cap < total) {
        MULTI_HIP(hipStreamSynchronize(r.stream));
        if (m->dn_buf)
            MULTI_HIP(hipFree(m->dn_buf));
        m->dn_buf = nullptr;
        m->dn_cap = 0;
        if (hipMalloc(&m->dn_buf, total * sizeof(float)) != hipSuccess)
            return fail(PTG_ERR_OUT_OF_MEMORY, "multi: hipMalloc of the denoiser's frames failed");
        m->dn_cap = total;
    }
    m->var_gathered = m->dn_buf;
    m->var_image = m->var_gathered + gath;
    m->filtered = m->var_image + img;
    m->feat = m->filtered + img;
    m->dn_scratch = m->feat + feat;
    m->dn_scratch_bytes = scratch * sizeof(float);
    return PTG_OK;
}

// The sums the shards hold, resolved, filtered and copied to m->host: every
// shard resolves its slab and writes its variance slab (samples_done > 0:
// ptg_resolve_device / ptg_noise_device at that count; 0: the *_active pair,
// each pixel's own count), two gathers through the one helper, two un-shards,
// the whole frame's features from the root's own context (shard_count 1: they
// depend on the scene, the camera and the global pixel only, so nothing moves;
// ptg_features_device plans with_acc = false and touches neither the sums, the
// counts nor the active list of the root's shard), ONE filter on the root's
// stream.  Synchronous.
int multi_resolve_filtered(ptg_multi *m, const ptg_params *p, int32_t samples_done, const ptg_denoise_params &k)
{
    size_t slab_elems = 0;
    int rc;
    if ((rc = reserve(m, p, slab_elems)) || (rc = reserve_denoise(m, p, slab_elems)))
        return rc;
    const int n = (int)m->shards.size();
    for (int i = 0; i < n; ++i) {
        Shard &s = m->shards[i];
        const ptg_params q = shard_params(p, i, n);
        if (samples_done > 0)
            rc = ptg_resolve_device(s.ctx, &q, samples_done, s.slab, s.stream);
        else
            rc = ptg_resolve_active_device(s.ctx, &q, s.slab, s.stream);
        if (rc)
            return rc;
        if (samples_done > 0)
            rc = ptg_noise_device(s.ctx, &q, samples_done, 0.0, 1.0, s.var, nullptr, nullptr, s.stream);
        else
            rc = ptg_noise_active_device(s.ctx, &q, 1.0, s.var, nullptr, s.stream);
        if (rc)
            return rc;
    }
    if ((rc = gather_unshard_device(m, p, slab_elems)) || (rc = gather_unshard_device(m, p, slab_elems, /*variance=*/true)))
        return rc;
    Shard &root = m->shards[0];
    if ((rc = ptg_features_for_(root.ctx, p, &k, m->feat, root.stream)))  // p: shard_count 1 (check_frame_params)
        return rc;
    MULTI_HIP(hipSetDevice(root.id));
    if ((rc = ptg_denoise_device(m->image, m->var_image, m->feat, p->width, p->height, &k, m->filtered, nullptr,
                                 m->dn_scratch, m->dn_scratch_bytes, root.stream)))
        return rc;
    const size_t image_elems = (size_t)p->width * p->height * 3;
    MULTI_HIP(hipMemcpyAsync(m->host.data(), m->filtered, image_elems * sizeof(float), hipMemcpyDeviceToHost,
                             root.stream));
    return sync_all(m);
}

// The loops' steps (frame_passes.hpp) from a ptg_multi: each check's statistics are every shard's, combined,
// with one synchronisation; a pass is bounded by each shard's own unit count (multi_select), not the frame's.
struct MultiSteps {
    ptg_multi *m;
    const ptg_params &p;
    bool count;  // adaptive passes add to the shards' kernel counters

    int reset() { return ptg_multi_reset_accumulation(m, &p); }
    int accumulate(int32_t b, int32_t e) { return ptg_multi_accumulate(m, &p, b, e); }
    int noise(int32_t done, double rel_error, double floor, unsigned long long *st)
    {
        return multi_noise(m, &p, done, rel_error, floor, st);
    }
    int all_active() { return multi_set_mask(m, &p, nullptr); }
    int accumulate_active(int32_t add, long long) { return multi_accumulate_active(m, &p, add, count); }
    int select(double rel_error, double floor, int32_t dilate, unsigned long long *st)
    {
        return multi_select(m, &p, rel_error, floor, dilate, st);
    }
};

}  // namespace

extern "C" {

int ptg_multi_create(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const int *devices,
                     int n_devices, ptg_multi **out)
{
    return create(spheres, n_spheres, cam, devices, n_devices, true, out);
}

// internal (tests): n_shards shards on ONE device, gathered by device copies
// into the same rank-major layout an n-rank ncclGather produces -- the
// n > 1 slab layout, un-shard and host add of the multi path on a 1-GPU box
int ptg_multi_create_local_(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, int device,
                            int n_shards, ptg_multi **out)
{
    if (n_shards < 1 || n_shards > 64)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi (local): 1 <= n_shards <= 64");
    std::vector<int> d(n_shards, device);
    return create(spheres, n_spheres, cam, d.data(), n_shards, false, out);
}

int ptg_multi_destroy(ptg_multi *m) { return destroy(m); }

int ptg_multi_render(ptg_multi *m, const ptg_params *params, double *image_rgb)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    m->timed = false;  // the image / events no longer describe a frame_device frame
    if (!image_rgb)
        return fail(PTG_ERR_INVALID_ARGUMENT, "render_multi: image is NULL");
    DeviceGuard g;
    size_t slab_elems = 0;
    if ((rc = reserve(m, params, slab_elems)))
        return rc;
    const int n = (int)m->shards.size();
    // the shards render concurrently (asynchronous launches on each device)
    for (int k = 0; k < n; ++k) {
        const ptg_params q = shard_params(params, k, n);
        if ((rc = ptg_render_device(m->shards[k].ctx, &q, m->shards[k].slab, nullptr, m->shards[k].stream)))
            return rc;
    }
    if ((rc = gather_unshard(m, params, slab_elems)))
        return rc;
    add_image(image_rgb, m->host.data(), (size_t)params->width * params->height * 3);
    return PTG_OK;
}

int ptg_multi_reset_accumulation(ptg_multi *m, const ptg_params *params)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    m->timed = false;  // the image / events no longer describe a frame_device frame
    DeviceGuard g;
    const int n = (int)m->shards.size();
    for (int k = 0; k < n; ++k) {
        const ptg_params q = shard_params(params, k, n);
        if ((rc = ptg_reset_accumulation_device(m->shards[k].ctx, &q, m->shards[k].stream)))
            return rc;
    }
    return PTG_OK;
}

int ptg_multi_accumulate(ptg_multi *m, const ptg_params *params, int32_t sample_begin, int32_t sample_end)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    m->timed = false;  // the image / events no longer describe a frame_device frame
    DeviceGuard g;
    const int n = (int)m->shards.size();
    for (int k = 0; k < n; ++k) {
        const ptg_params q = shard_params(params, k, n);
        if ((rc = ptg_accumulate_device(m->shards[k].ctx, &q, sample_begin, sample_end, nullptr,
                                        m->shards[k].stream)))
            return rc;
    }
    return PTG_OK;
}

int ptg_multi_resolve(ptg_multi *m, const ptg_params *params, int32_t samples_done, float *image_rgb)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    m->timed = false;  // the image / events no longer describe a frame_device frame
    if (!image_rgb)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_resolve: image is NULL");
    DeviceGuard g;
    if ((rc = multi_resolve(m, params, samples_done)))
        return rc;
    const size_t image_elems = (size_t)params->width * params->height * 3;
    std::copy(m->host.begin(), m->host.begin() + image_elems, image_rgb);
    return PTG_OK;
}

int ptg_multi_noise(ptg_multi *m, const ptg_params *params, int32_t samples_done, double rel_error, double floor,
                    unsigned long long *stats)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    if (!stats)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_noise: stats is NULL");
    if (samples_done < 2 || samples_done > params->samples)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_noise: samples_done must be in [2, samples]");
    if ((rc = check_noise_args("multi_noise", rel_error, floor)))
        return rc;
    m->timed = false;  // the image / events no longer describe a frame_device frame
    DeviceGuard g;
    return multi_noise(m, params, samples_done, rel_error, floor, stats);
}

int ptg_multi_set_active_mask(ptg_multi *m, const ptg_params *params, const uint8_t *mask)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    m->timed = false;
    DeviceGuard g;
    return multi_set_mask(m, params, mask);
}

int ptg_multi_select_active(ptg_multi *m, const ptg_params *params, double rel_error, double floor, int32_t dilate,
                            unsigned long long *stats)
{
    int rc = check_frame(m, params);
    if (rc || (rc = check_noise_args("multi_select_active", rel_error, floor)))
        return rc;
    if (dilate < 0 || dilate > 8)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_select_active: dilate must be in [0, 8]");
    m->timed = false;
    DeviceGuard g;
    return multi_select(m, params, rel_error, floor, dilate, stats);
}

int ptg_multi_accumulate_active(ptg_multi *m, const ptg_params *params, int32_t add_samples)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    if (add_samples < 0)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_accumulate_active: add_samples must be >= 0");
    m->timed = false;
    DeviceGuard g;
    return multi_accumulate_active(m, params, add_samples, /*count=*/false);
}

int ptg_multi_resolve_active(ptg_multi *m, const ptg_params *params, float *image_rgb)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    if (!image_rgb)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_resolve_active: image is NULL");
    m->timed = false;
    DeviceGuard g;
    if ((rc = multi_resolve(m, params, 0, /*active=*/true)))
        return rc;
    const size_t image_elems = (size_t)params->width * params->height * 3;
    std::copy(m->host.begin(), m->host.begin() + image_elems, image_rgb);
    return PTG_OK;
}

int ptg_multi_read_sample_counts(ptg_multi *m, const ptg_params *params, int32_t *counts)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    if (!counts)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_read_sample_counts: counts is NULL");
    m->timed = false;
    DeviceGuard g;
    return multi_read_counts(m, params, counts);
}

// The noise-target frames, their arguments checked: the passes, checks and report of frame_passes.hpp (no
// target: the one pass [0, samples) of ptg_multi_render_denoised), the frame they stopped at resolved -- through
// the filter `dk` where there is one -- and ADDED into image_rgb
static int noise_frame_on(ptg_multi *m, const ptg_params *params, const Passes &ps, const ptg_noise_target *target,
                          const ptg_denoise_params *dk, double *image_rgb, ptg_noise_report *report)
{
    m->timed = false;
    DeviceGuard g;
    ptg_noise_report rep{};
    ptg_params p = *params;
    p.flags |= PTG_FLAG_MOMENTS;
    int32_t done = 0;
    int rc = noise_passes(MultiSteps{m, p, false}, ps, target, rep, done);
    if (rc || (rc = dk ? multi_resolve_filtered(m, &p, done, *dk) : multi_resolve(m, &p, done)))
        return rc;
    add_image(image_rgb, m->host.data(), (size_t)p.width * p.height * 3);
    if (report)
        *report = rep;
    return PTG_OK;
}

// ptg_multi_render_to_noise, and with `filter` ptg_multi_render_to_noise_denoised
static int render_to_noise_on(ptg_multi *m, const ptg_params *params, const ptg_noise_target *target,
                              const ptg_denoise_params *denoise, bool filter, double *image_rgb,
                              ptg_noise_report *report)
{
    if (!image_rgb || !target)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_render_to_noise: NULL image or target");
    Passes ps;
    ptg_denoise_params dk{};
    int rc = check_frame(m, params);
    if (rc || (rc = check_target("multi_render_to_noise", target_of(*target), params->samples, ps)) ||
        (filter && (rc = ptg_denoise_params_for_(&m->cam, params->width, params->height, denoise, &dk))))
        return rc;
    return noise_frame_on(m, params, ps, target, filter ? &dk : nullptr, image_rgb, report);
}

int ptg_multi_render_to_noise(ptg_multi *m, const ptg_params *params, const ptg_noise_target *target,
                              double *image_rgb, ptg_noise_report *report)
{
    return render_to_noise_on(m, params, target, nullptr, /*filter=*/false, image_rgb, report);
}

int ptg_multi_render_to_noise_denoised(ptg_multi *m, const ptg_params *params, const ptg_noise_target *target,
                                       const ptg_denoise_params *denoise, double *image_rgb, ptg_noise_report *report)
{
    return render_to_noise_on(m, params, target, denoise, /*filter=*/true, image_rgb, report);
}

// ptg_multi_render_adaptive, and with `filter` ptg_multi_render_adaptive_denoised
static int render_adaptive_on(ptg_multi *m, const ptg_params *params, const ptg_adaptive_target *target,
                              const ptg_denoise_params *denoise, bool filter, double *image_rgb,
                              int32_t *sample_counts, ptg_adaptive_report *report)
{
    if (!image_rgb || !target)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_render_adaptive: NULL image or target");
    Passes ps;
    ptg_denoise_params dk{};
    int rc = check_frame(m, params);
    if (rc || (rc = check_target("multi_render_adaptive", target_of(*target), params->samples, ps)) ||
        (filter && (rc = ptg_denoise_params_for_(&m->cam, params->width, params->height, denoise, &dk))))
        return rc;
    m->timed = false;
    DeviceGuard g;
    ptg_adaptive_report rep{};
    const ptg_params &p = *params;
    const bool count = (p.flags & (PTG_FLAG_COUNT_TESTS | PTG_FLAG_COUNT_NONFINITE)) != 0;
    size_t slab_pixels = 0;
    if ((rc = reserve_adaptive(m, &p, slab_pixels)))
        return rc;
    for (Shard &s : m->shards) {  // the kernel counters of the frame
        MULTI_HIP(hipSetDevice(s.id));
        MULTI_HIP(hipMemsetAsync(s.stats + 6, 0, 4 * sizeof(unsigned long long), s.stream));
    }
    if ((rc = adaptive_passes(MultiSteps{m, p, count}, p, ps, *target, rep)))
        return rc;
    if ((rc = filter ? multi_resolve_filtered(m, &p, 0, dk) : multi_resolve(m, &p, 0, /*active=*/true)) ||
        (sample_counts && (rc = multi_read_counts(m, &p, sample_counts))))
        return rc;
    if (count) {
        const int n = (int)m->shards.size();
        for (int k = 0; k < n; ++k) {  // into the pinned statistics, one wait for all
            Shard &s = m->shards[k];
            MULTI_HIP(hipSetDevice(s.id));
            MULTI_HIP(hipMemcpyAsync(m->host_stats + (size_t)k * kStats + 6, s.stats + 6, 4 * sizeof(unsigned long long),
                                     hipMemcpyDeviceToHost, s.stream));
        }
        if ((rc = sync_all(m)))
            return rc;
        for (int k = 0; k < n; ++k)
            for (int i = 0; i < 4; ++i)
                rep.counters[i] += m->host_stats[(size_t)k * kStats + 6 + i];
    }
    add_image(image_rgb, m->host.data(), (size_t)p.width * p.height * 3);
    if (report)
        *report = rep;
    return PTG_OK;
}

int ptg_multi_render_adaptive(ptg_multi *m, const ptg_params *params, const ptg_adaptive_target *target,
                              double *image_rgb, int32_t *sample_counts, ptg_adaptive_report *report)
{
    return render_adaptive_on(m, params, target, nullptr, /*filter=*/false, image_rgb, sample_counts, report);
}

int ptg_multi_render_adaptive_denoised(ptg_multi *m, const ptg_params *params, const ptg_adaptive_target *target,
                                       const ptg_denoise_params *denoise, double *image_rgb, int32_t *sample_counts,
                                       ptg_adaptive_report *report)
{
    return render_adaptive_on(m, params, target, denoise, /*filter=*/true, image_rgb, sample_counts, report);
}

// the filter's arguments of the pieces and of ptg_multi_render_denoised, after the frame's
static int check_filtered(const ptg_multi *m, const ptg_params *params, int32_t samples_done, const void *image,
                          const ptg_denoise_params *denoise, const char *who, ptg_denoise_params *k)
{
    if (!image)
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": image is NULL");
    if (samples_done < 2 || samples_done > params->samples)
        return fail(PTG_ERR_INVALID_ARGUMENT, std::string(who) + ": samples must be in [2, params->samples] (the "
                                                                 "variance needs two)");
    return ptg_denoise_params_for_(&m->cam, params->width, params->height, denoise, k);
}

int ptg_multi_resolve_denoised(ptg_multi *m, const ptg_params *params, int32_t samples_done,
                               const ptg_denoise_params *denoise, float *image_rgb)
{
    ptg_denoise_params k;
    int rc = check_frame(m, params);
    if (rc || (rc = check_filtered(m, params, samples_done, image_rgb, denoise, "multi_resolve_denoised", &k)))
        return rc;
    m->timed = false;  // the image / events no longer describe a frame_device frame
    DeviceGuard g;
    if ((rc = multi_resolve_filtered(m, params, samples_done, k)))
        return rc;
    std::copy(m->host.begin(), m->host.begin() + (size_t)params->width * params->height * 3, image_rgb);
    return PTG_OK;
}

int ptg_multi_resolve_active_denoised(ptg_multi *m, const ptg_params *params, const ptg_denoise_params *denoise,
                                      float *image_rgb)
{
    ptg_denoise_params k;
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    if (!image_rgb)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_resolve_active_denoised: image is NULL");
    if ((rc = ptg_denoise_params_for_(&m->cam, params->width, params->height, denoise, &k)))
        return rc;
    m->timed = false;
    DeviceGuard g;
    if ((rc = multi_resolve_filtered(m, params, 0, k)))
        return rc;
    std::copy(m->host.begin(), m->host.begin() + (size_t)params->width * params->height * 3, image_rgb);
    return PTG_OK;
}

int ptg_multi_render_denoised(ptg_multi *m, const ptg_params *params, const ptg_denoise_params *denoise,
                              double *image_rgb)
{
    ptg_denoise_params k;
    int rc = check_frame(m, params);
    if (rc || (rc = check_filtered(m, params, params->samples, image_rgb, denoise, "multi_render_denoised", &k)))
        return rc;
    Passes ps;
    ps.ends[0] = params->samples;
    ps.n = 1;
    return noise_frame_on(m, params, ps, nullptr, &k, image_rgb, nullptr);
}

int ptg_multi_frame_device(ptg_multi *m, const ptg_params *params, unsigned long long *counters)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    DeviceGuard g;
    // before reserve(): a failed re-allocation must not leave the previous
    // frame's flag on a freed image
    m->timed = false;
    size_t slab_elems = 0;
    if ((rc = reserve(m, params, slab_elems)))
        return rc;
    const int n = (int)m->shards.size();
    const bool count = (params->flags & (PTG_FLAG_COUNT_TESTS | PTG_FLAG_COUNT_NONFINITE)) != 0;
    for (int k = 0; k < n; ++k) {
        Shard &s = m->shards[k];
        MULTI_HIP(hipSetDevice(s.id));
        if (count && !s.counters && hipMalloc(&s.counters, 4 * sizeof(unsigned long long)) != hipSuccess)
            return fail(PTG_ERR_OUT_OF_MEMORY, "multi: hipMalloc of the counters failed");
        if (count)
            MULTI_HIP(hipMemsetAsync(s.counters, 0, 4 * sizeof(unsigned long long), s.stream));
        MULTI_HIP(hipEventRecord(s.t_begin, s.stream));
        const ptg_params q = shard_params(params, k, n);
        if ((rc = ptg_render_device(s.ctx, &q, s.slab, count ? s.counters : nullptr, s.stream)))
            return rc;
        MULTI_HIP(hipSetDevice(s.id));
        MULTI_HIP(hipEventRecord(s.t_rendered, s.stream));
    }
    if ((rc = gather_unshard_device(m, params, slab_elems)))
        return rc;
    MULTI_HIP(hipSetDevice(m->shards[0].id));
    MULTI_HIP(hipEventRecord(m->t_unsharded, m->shards[0].stream));
    if ((rc = sync_all(m)))
        return rc;
    m->timed = true;
    m->frame_w = params->width;
    m->frame_h = params->height;
    m->frame_band_rows = params->band_rows;
    if (count && counters) {
        for (int i = 0; i < 4; ++i)
            counters[i] = 0;
        for (Shard &s : m->shards) {
            unsigned long long c[4];
            MULTI_HIP(hipSetDevice(s.id));
            MULTI_HIP(hipMemcpy(c, s.counters, sizeof(c), hipMemcpyDeviceToHost));
            for (int i = 0; i < 4; ++i)
                counters[i] += c[i];
        }
    }
    return PTG_OK;
}

int ptg_multi_frame_timing(const ptg_multi *m, float *render_ms, int n, float *frame_ms)
{
    if (!m || !m->timed)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_frame_timing: no completed ptg_multi_frame_device");
    if (n != (int)m->shards.size() || !render_ms || !frame_ms)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_frame_timing: render_ms needs one entry per device");
    DeviceGuard g;
    for (int k = 0; k < n; ++k) {
        MULTI_HIP(hipSetDevice(m->shards[k].id));
        MULTI_HIP(hipEventElapsedTime(&render_ms[k], m->shards[k].t_begin, m->shards[k].t_rendered));
    }
    MULTI_HIP(hipSetDevice(m->shards[0].id));
    MULTI_HIP(hipEventElapsedTime(frame_ms, m->shards[0].t_begin, m->t_unsharded));
    return PTG_OK;
}

int ptg_multi_image(ptg_multi *m, const ptg_params *params, float *image_rgb)
{
    int rc = check_frame(m, params);
    if (rc)
        return rc;
    if (!image_rgb || !m->timed)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_image: NULL image or no completed ptg_multi_frame_device "
                                              "(since the last render / pass / resolve)");
    if (params->width != m->frame_w || params->height != m->frame_h || params->band_rows != m->frame_band_rows)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_image: params differ from the last frame's width, height or "
                                              "band_rows");
    const size_t image_elems = (size_t)params->width * params->height * 3;
    DeviceGuard g;
    MULTI_HIP(hipSetDevice(m->shards[0].id));
    MULTI_HIP(hipMemcpy(image_rgb, m->image, image_elems * sizeof(float), hipMemcpyDeviceToHost));
    return PTG_OK;
}

int ptg_multi_comm_info(const ptg_multi *m, int32_t *ranks, int32_t *comm_devices, int32_t *user_ranks, int n)
{
    if (!m || !ranks || !comm_devices || !user_ranks)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_comm_info: NULL argument");
    if (n != (int)m->shards.size())
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi_comm_info: one entry per shard");
    for (int k = 0; k < n; ++k) {
        const Shard &s = m->shards[k];
        ranks[k] = 0;
        comm_devices[k] = s.id;
        user_ranks[k] = -1;
        if (!s.comm)
            continue;
        int c = 0, dev = -1, ur = -1;
        ncclResult_t r = ncclCommCount(s.comm, &c);
        if (r == ncclSuccess)
            r = ncclCommCuDevice(s.comm, &dev);
        if (r == ncclSuccess)
            r = ncclCommUserRank(s.comm, &ur);
        if (r != ncclSuccess)
            return nccl_fail("ncclCommCount/CuDevice/UserRank", r);
        ranks[k] = c;
        comm_devices[k] = dev;
        user_ranks[k] = ur;
    }
    return PTG_OK;
}

int ptg_device_pci_bus_id(int device, char *buf, int len)
{
    if (!buf || len < 1)
        return fail(PTG_ERR_INVALID_ARGUMENT, "pci_bus_id: NULL or empty buffer");
    buf[0] = '\0';
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PTG_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count)
        return fail(PTG_ERR_INVALID_ARGUMENT, "pci_bus_id: device ordinal out of range");
    MULTI_HIP(hipDeviceGetPCIBusId(buf, len, device));
    return PTG_OK;
}

// internal (tests): make the next RCCL gather fail at shard k (-1: off)
int ptg_multi_inject_gather_fault_(ptg_multi *m, int k)
{
    if (!m)
        return fail(PTG_ERR_INVALID_ARGUMENT, "multi: NULL context");
    m->inject_gather_fault = k;
    return PTG_OK;
}

}  // extern "C"

// The one-shot forms: every argument checked before any device work (`args`: the form's own pointers are there;
// `target` NULL: a form without one), then create, call(m), destroy.
template <class Call>
static int one_shot(const std::string &who, bool args, const ptg_sphere *spheres, size_t n_spheres,
                    const ptg_camera *cam, const ptg_params *params, const int *devices, int n_devices,
                    const Target *target, bool filtered, const ptg_denoise_params *denoise, Call &&call)
{
    if (!args || !params || !devices || n_devices < 1 || (filtered && !cam))
        return fail(PTG_ERR_INVALID_ARGUMENT, who + ": NULL argument or no device");
    Passes ps;
    ptg_denoise_params k;
    int rc = check_frame_params(params);
    if (rc)
        return rc;
    if (filtered && !target && params->samples < 2)
        return fail(PTG_ERR_INVALID_ARGUMENT, who + ": samples must be >= 2 (the variance needs two)");
    if ((target && (rc = check_target(who, *target, params->samples, ps))) ||
        (filtered && (rc = ptg_denoise_params_for_(cam, params->width, params->height, denoise, &k))))
        return rc;
    ptg_multi *m = nullptr;
    if ((rc = ptg_multi_create(spheres, n_spheres, cam, devices, n_devices, &m)))
        return rc;
    rc = call(m);
    ptg_multi_destroy(m);
    return rc;
}

template <class T>
static Target target_or_none(const T *target)  // (a NULL target fails one_shot's `args`)
{
    return target ? target_of(*target) : Target{};
}

extern "C" {

int ptg_render_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam, const ptg_params *params,
                     const int *devices, int n_devices, double *image_rgb)
{
    return one_shot("render_multi", image_rgb, spheres, n_spheres, cam, params, devices, n_devices, nullptr, false,
                    nullptr, [&](ptg_multi *m) { return ptg_multi_render(m, params, image_rgb); });
}

int ptg_render_to_noise_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                              const ptg_params *params, const int *devices, int n_devices,
                              const ptg_noise_target *target, double *image_rgb, ptg_noise_report *report)
{
    const Target t = target_or_none(target);
    return one_shot("render_to_noise_multi", image_rgb && target, spheres, n_spheres, cam, params, devices, n_devices,
                    &t, false, nullptr,
                    [&](ptg_multi *m) { return ptg_multi_render_to_noise(m, params, target, image_rgb, report); });
}

int ptg_render_adaptive_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                              const ptg_params *params, const int *devices, int n_devices,
                              const ptg_adaptive_target *target, double *image_rgb, int32_t *sample_counts,
                              ptg_adaptive_report *report)
{
    const Target t = target_or_none(target);
    return one_shot("render_adaptive_multi", image_rgb && target, spheres, n_spheres, cam, params, devices, n_devices,
                    &t, false, nullptr, [&](ptg_multi *m) {
                        return ptg_multi_render_adaptive(m, params, target, image_rgb, sample_counts, report);
                    });
}

int ptg_render_denoised_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                              const ptg_params *params, const int *devices, int n_devices,
                              const ptg_denoise_params *denoise, double *image_rgb)
{
    return one_shot("render_denoised_multi", image_rgb, spheres, n_spheres, cam, params, devices, n_devices, nullptr,
                    true, denoise,
                    [&](ptg_multi *m) { return ptg_multi_render_denoised(m, params, denoise, image_rgb); });
}

int ptg_render_to_noise_denoised_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                                       const ptg_params *params, const int *devices, int n_devices,
                                       const ptg_noise_target *target, const ptg_denoise_params *denoise,
                                       double *image_rgb, ptg_noise_report *report)
{
    const Target t = target_or_none(target);
    return one_shot("render_to_noise_denoised_multi", image_rgb && target, spheres, n_spheres, cam, params, devices,
                    n_devices, &t, true, denoise, [&](ptg_multi *m) {
                        return ptg_multi_render_to_noise_denoised(m, params, target, denoise, image_rgb, report);
                    });
}

int ptg_render_adaptive_denoised_multi(const ptg_sphere *spheres, size_t n_spheres, const ptg_camera *cam,
                                       const ptg_params *params, const int *devices, int n_devices,
                                       const ptg_adaptive_target *target, const ptg_denoise_params *denoise,
                                       double *image_rgb, int32_t *sample_counts, ptg_adaptive_report *report)
{
    const Target t = target_or_none(target);
    return one_shot("render_adaptive_denoised_multi", image_rgb && target, spheres, n_spheres, cam, params, devices,
                    n_devices, &t, true, denoise, [&](ptg_multi *m) {
                        return ptg_multi_render_adaptive_denoised(m, params, target, denoise, image_rgb, sample_counts,
                                                                  report);
                    });
}

}  // extern "C"
