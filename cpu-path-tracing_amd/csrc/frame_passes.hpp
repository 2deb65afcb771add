// frame_passes.hpp -- what the whole-frame drivers share (host only): the target checks, the two pass loops,
// their report fillers and the ADD into the caller's image.  The loops are written against the few steps they
// need; csrc/ptg_frames.cpp supplies them from a ptg_context on the null stream, csrc/ptg_multi.cpp from a
// ptg_multi:
//   reset()  accumulate(b, e)  noise(done, rel_error, floor, st[4])
//   all_active()  accumulate_active(add, units)  select(rel_error, floor, dilate, st[6])
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/ptgpu.h"

extern "C" int ptg_set_error_(int code, const char *msg);  // ptg_render.hip: ptg_last_error's thread-local text

// (every function static: a host-only header, no symbol of it leaves its translation unit)
namespace ptg_frames {

static inline int fail(int code, const std::string &msg) { return ptg_set_error_(code, msg.c_str()); }

// either target (the two structs differ in their last field only), and the pass ends of its schedule
struct Target {
    double rel_error, floor, max_fraction;
    int32_t min_samples, dilate;
};
static inline Target target_of(const ptg_noise_target &t)
{
    return {t.rel_error, t.floor, t.max_fraction, t.min_samples, 0};
}
static inline Target target_of(const ptg_adaptive_target &t)
{
    return {t.rel_error, t.floor, t.max_fraction, t.min_samples, t.dilate};
}
struct Passes {
    int32_t ends[PTG_NOISE_MAX_PASSES];
    int32_t n = 0;
};

// The target checks, before any device work; `who` names the caller in the message.
static inline int check_noise_args(const std::string &who, double rel_error, double floor)
{
    if (!(floor > 0.0) || !(rel_error >= 0.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, who + ": floor must be > 0 and rel_error >= 0");
    return PTG_OK;
}

static inline int check_target(const std::string &who, const Target &t, int32_t samples, Passes &ps)
{
    if (int rc = check_noise_args(who, t.rel_error, t.floor))
        return rc;
    if (!(t.max_fraction >= 0.0 && t.max_fraction < 1.0))
        return fail(PTG_ERR_INVALID_ARGUMENT, who + ": max_fraction must be in [0, 1)");
    if (t.dilate < 0 || t.dilate > 8)
        return fail(PTG_ERR_INVALID_ARGUMENT, who + ": dilate must be in [0, 8]");
    return ptg_noise_schedule(t.min_samples, samples, ps.ends, PTG_NOISE_MAX_PASSES, &ps.n);
}

static inline double rho_of_bits(unsigned long long bits)
{
    const uint32_t b = (uint32_t)bits;
    float rho;
    std::memcpy(&rho, &b, sizeof(rho));
    return (double)rho;
}

// what both reports say of the last check: st = over, sum of min(rho, 4096) in 2^-20 steps, max rho's bits, pixels
template <class Report>
static void fill_check(Report &rep, int k, const unsigned long long *st, double max_fraction)
{
    rep.passes = k + 1;
    rep.pixels = st[3];
    rep.pixels_over = st[0];
    rep.pass_over[k] = st[0];
    rep.max_rho = rho_of_bits(st[2]);
    rep.mean_rho = st[3] ? (double)st[1] * 0x1p-20 / (double)st[3] : 0.0;
    rep.converged = (double)st[0] <= max_fraction * (double)st[3];
}

// Render until converged: the passes [done, ends[k]), after each one noise check and the stop rule.  Without a
// target: the passes (one, [0, samples)) unchecked.  done: the samples in the sums.
template <class Steps>
static int noise_passes(Steps &&s, const Passes &ps, const ptg_noise_target *t, ptg_noise_report &rep, int32_t &done)
{
    int rc = s.reset();
    done = 0;
    for (int k = 0; !rc && k < ps.n; ++k) {
        if ((rc = s.accumulate(done, ps.ends[k])))
            return rc;
        done = ps.ends[k];
        if (!t)
            continue;
        unsigned long long st[4];
        if ((rc = s.noise(done, t->rel_error, t->floor, st)))
            return rc;
        rep.samples_done = rep.pass_samples[k] = done;
        fill_check(rep, k, st, t->max_fraction);
        if (rep.converged)
            break;
    }
    return rc;
}

// Adaptive: every pixel active, then per pass ends[k] - done more samples for the active pixels, one selection
// (st[4]: pixels active after it, st[5]: their work units, the next pass's bound) and the stop rule.
template <class Steps>
static int adaptive_passes(Steps &&s, const ptg_params &p, const Passes &ps, const ptg_adaptive_target &t,
                           ptg_adaptive_report &rep)
{
    int rc;
    if ((rc = s.reset()) || (rc = s.all_active()))  // pass 0: every pixel
        return rc;
    unsigned long long active = (unsigned long long)p.width * p.height;
    long long units = 0;  // pass 0: the host-side bound
    int32_t done = 0;
    for (int k = 0; k < ps.n; ++k) {
        unsigned long long st[6];
        const int32_t add = ps.ends[k] - done;
        if ((rc = s.accumulate_active(add, units)))
            return rc;
        done = ps.ends[k];
        rep.total_samples += active * (unsigned long long)add;
        if ((rc = s.select(t.rel_error, t.floor, t.dilate, st)))
            return rc;
        rep.max_samples = done;
        rep.pass_added[k] = add;
        rep.pass_active[k] = st[4];
        fill_check(rep, k, st, t.max_fraction);
        if (rep.converged)
            break;
        active = st[4];
        units = (long long)st[5];  // (> 0: a pixel over the target is active)
    }
    return PTG_OK;
}

template <class T>
static void add_image(double *image, const T *frame, size_t n)
{
    for (size_t i = 0; i < n; ++i)  // main.cpp:196: image[row] += ...
        image[i] = image[i] + (double)frame[i];
}

}  // namespace ptg_frames
