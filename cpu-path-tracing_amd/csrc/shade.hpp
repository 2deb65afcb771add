// shade.hpp -- one bounce segment of a path: segment() runs a whole scan and
// shade(), everything after the scan (sky, emission, Russian roulette, the
// next direction, light sampling's shadow segment with LsLane / LsIo).
// Included by ptg_render.hip inside its unnamed namespace, after the two
// scans; needs scene_scan, scene_scan_bvh and ScanCount from them, KArgs,
// ShadeRec and LightRec (kernel_args.hpp), draw and Math (pt_device.hpp).
// Owns no switch; reads PTG_BLOCK_STATS (render_config.hpp).
#pragma once

// Per-lane state machine: one call = one bounce segment of radiance()
// (main.cpp:111-155).  Returns true when the path has ended; E then holds
// its radiance.
// shade(): everything after the scene scan -- sky on a miss, else hit
// record, emission, Russian roulette, BRDF sampling of the next ray.
//
// Light sampling (kLS; PTG_FLAG_LIGHT_SAMPLING, include/ptgpu.h): a diffuse
// hit may be followed by a shadow segment -- one more state of the lane.  The
// lane keeps the contribution the segment would add, the BRDF direction it
// resumes with and the light's id in LsLane; the segment's origin is the hit
// point, which o already holds.  What the lane is doing travels in LsIo: in,
// this segment is a shadow segment / this hit skips the listed emitters; out,
// the same two for the lane's next segment (the callers keep them as wave
// masks).  Without kLS both structs are unused and the code is as before.
struct LsLane {
    f3 pend, nd;
    int light;
};
struct LsIo {
    const LightRec *lights;
    int n_lights;
    int hid;                     // what the scan reported (LightRec id)
    bool shadow, skip;           // in
    bool to_shadow, skip_next;   // out
};
// kStrat (PTG_FLAG_STRATIFIED): fh holds the path's pairs 2 and 3, {phi, r,
// u1, u2} of its first hit -- read only at depth 0, on a diffuse lane
template <bool kExact, bool kLS = false, bool kStrat = false>
__device__ __forceinline__ bool shade(const ShadeRec *hit, float t, const float2 *trig, f3 &o, f3 &d, f3 &T, f3 &E,
                                      int &depth, uint32_t &st, LsLane &ls, LsIo &io, const uint4 fh = uint4{});
template <bool kExact>
__device__ __forceinline__ bool shade(const ShadeRec *hit, float t, const float2 *trig, f3 &o, f3 &d, f3 &T, f3 &E,
                                      int &depth, uint32_t &st)
{
    LsLane ls;
    LsIo io;
    return shade<kExact, false>(hit, t, trig, o, d, T, E, depth, st, ls, io);
}

template <bool kBvh, bool kExact, bool kCount = false, bool kLS = false, bool kStrat = false>
__device__ __forceinline__ bool segment(const KArgs &A, const LinRec *recs, const float2 *trig, f3 &o, f3 &d, f3 &T,
                                        f3 &E, int &depth, uint32_t &st, ScanCount &cnt, LsLane &ls, LsIo &io,
                                        [[maybe_unused]] const uint4 fh = uint4{})
{
    float t;
    const ShadeRec *hit;
    if constexpr (kBvh) {
        const int id = scene_scan_bvh<kCount, kExact>(A, o, d, t, cnt);
        hit = id >= 0 ? A.shade + id : nullptr;
        if constexpr (kLS)
            io.hid = id;
    } else {
        const LinRec *w = scene_scan<kExact, kCount>(A, recs, o, d, t, cnt);
        hit = w != recs + A.n ? &w->s : nullptr;
        if constexpr (kLS)
            io.hid = (int)(w - recs);
    }
    if constexpr (kStrat)
        return shade<kExact, kLS, true>(hit, t, trig, o, d, T, E, depth, st, ls, io, fh);
    else
    return shade<kExact, kLS>(hit, t, trig, o, d, T, E, depth, st, ls, io);
}
template <bool kBvh, bool kExact, bool kCount = false>
__device__ __forceinline__ bool segment(const KArgs &A, const LinRec *recs, const float2 *trig, f3 &o, f3 &d, f3 &T,
                                        f3 &E, int &depth, uint32_t &st, ScanCount &cnt)
{
    LsLane ls;
    LsIo io;
    return segment<kBvh, kExact, kCount, false>(A, recs, trig, o, d, T, E, depth, st, cnt, ls, io);
}

template <bool kExact, bool kLS, bool kStrat>
__device__ __forceinline__ bool shade(const ShadeRec *hit, float t, const float2 *trig, f3 &o, f3 &d, f3 &T, f3 &E,
                                      int &depth, uint32_t &st, [[maybe_unused]] LsLane &ls, [[maybe_unused]] LsIo &io,
                                      [[maybe_unused]] const uint4 fh)
{
    if constexpr (kLS) {
        // a shadow segment's "shade": the pending value when the light is
        // the nearest hit, then on with the bounce; depth is not counted
        if (io.shadow) {
            const bool lit = io.hid == ls.light;
            E = mk3(lit ? E.x + ls.pend.x : E.x, lit ? E.y + ls.pend.y : E.y, lit ? E.z + ls.pend.z : E.z);
            d = ls.nd;
            io.skip_next = true;
            return false;
        }
    }
    // the segment count first, for every lane: a sky lane's path ends here
    // (its depth is reset by the refill), so the value is only read below --
    // no per-branch copy of the loop-carried register
    depth += 1;
    // kStrat: the camera ray's own hit takes its BRDF and light-sample draws
    // from the path's pairs (io.fh) and leaves the xorshift state where it is
    [[maybe_unused]] const bool first = kStrat && depth == 1;
    if (!hit) {  // main.cpp:115-120: sky
        f3 ud = norm3m<kExact>(d);
        float tt = 0.5f * (ud.y + 1.0f);
        float it = 1.0f - tt;
        E = mk3(__builtin_fmaf(T.x, __builtin_fmaf(tt, 0.5f, it), E.x),
                __builtin_fmaf(T.y, __builtin_fmaf(tt, 0.7f, it), E.y),
                __builtin_fmaf(T.z, __builtin_fmaf(tt, 1.0f, it), E.z));
        return true;
    }
    const ShadeRec &S = *hit;
    float4 s0 = S.s0;
    const float4 s1 = S.s1;
    // hit_record.cpp:3-12
    f3 p = mk3(__builtin_fmaf(d.x, t, o.x), __builtin_fmaf(d.y, t, o.y), __builtin_fmaf(d.z, t, o.z));
    // hit_record.cpp:6 (p - C).norm() as (p - C) * (1/R): p lies on the sphere
    const bool rr = depth > kRRThreshold + 1;  // (the depth before this segment's count)
    const float4 cc = *(rr ? &S.s3 : &S.s2);  // (prepare_scene: 1/R in s2.w and s3.w)
    const float invR = cc.w;
    bool front;
    f3 on, nn;
    [[maybe_unused]] float kn = 0.0f;  // fast mode: nn.d
    if (!kExact) {
        const f3 pc = mk3(p.x - s0.x, p.y - s0.y, p.z - s0.z);
        const float sd = dot3(pc, d);
        front = sd < 0.0f;
        const float ks = front ? invR : -invR;
        nn = mk3(pc.x * ks, pc.y * ks, pc.z * ks);
        kn = sd * ks;
        on = nn;  // (unused: the mirror reflects on nn)
    } else {
        on = mk3((p.x - s0.x) * invR, (p.y - s0.y) * invR, (p.z - s0.z) * invR);
        front = dot3(on, d) < 0.0f;
        nn = front ? on : mk3(-on.x, -on.y, -on.z);
    }
    // main.cpp:126
    if constexpr (kLS) {
        // the hit after a light-sampling step: the listed emitters were
        // sampled there (their ids by wave-uniform loads) -- those met on
        // their front face.  A back face means the previous hit point lay
        // inside that light, where the step adds nothing: it counts here
        bool listed = false;
        if (io.skip & front)
            for (int k = 0; k < io.n_lights; ++k)
                listed |= io.hid == __float_as_int(io.lights[k].e.w);
        if (!listed)
            E = mk3(__builtin_fmaf(T.x, s1.x, E.x), __builtin_fmaf(T.y, s1.y, E.y), __builtin_fmaf(T.z, s1.z, E.z));
    } else
    E = mk3(__builtin_fmaf(T.x, s1.x, E.x), __builtin_fmaf(T.y, s1.y, E.y), __builtin_fmaf(T.z, s1.z, E.z));
    // main.cpp:128-139: Russian roulette after depth 4 (the colour row read
    // above by address)
    // Russian roulette without an early return: the roulette's draw advances the state of the
    // rr lanes only (a select), and a killed lane runs on with its materials
    // masked -- its next ray and state are discarded (the early return's
    // merge had cost state copies and exec-mask blocks)
    uint32_t st_rr = st;
    const uint32_t m_rr = draw_bits(st_rr);  // u = m_rr 2^-24; s0.w holds ceil(p 2^24) (prepare_scene)
    st = rr ? st_rr : st;
    const bool killed = rr & !(m_rr < __float_as_uint(s0.w));
    T = mk3(T.x * cc.x, T.y * cc.y, T.z * cc.z);
    // BRDF samplers (main.cpp:44-97).  Diffuse and dielectric lanes share the
    // three expensive ops (one rsqrt, two sqrt) through selects, so a wave
    // holding both materials issues them once; every lane's arithmetic is the
    // same as the per-material code (oracle sample_B).
    const int mat = __float_as_int(s1.w);
    const bool isD = !killed & (mat == PTG_DIFFUSE);
    const bool isG = !killed & (mat == PTG_DIELECTRIC);
    bool spec = !killed & (mat == PTG_SPECULAR);
    // every lane's first BRDF draw taken once, here: the diffuse phi, the
    // dielectric's Fresnel draw -- or, where it cannot refract, its
    // reflection's draw -- and the mirror's draw (main.cpp:46, :89, :62).
    // A dielectric lane reflected by its Fresnel draw takes the reflection's
    // draw as well: the block's shared second step below (fres_refl).
    // Each lane's draws keep their order and count; killed lanes advance a
    // state their ended path no longer reads.
    // light sampling: a diffuse lane whose path goes on takes the step's
    // draws first -- the light (only with several), then u1, u2 -- whatever
    // the geometry (include/ptgpu.h)
    [[maybe_unused]] bool ls_run = false;
    [[maybe_unused]] uint32_t ls_k = 0, ls_m1 = 0, ls_m2 = 0;
    if constexpr (kLS) {
        ls_run = isD & (depth < kDepthLimit);
        uint32_t st_l = st;
        if (io.n_lights > 1)  // floor(u L) of u = m 2^-24, exactly
            ls_k = min((uint32_t)(io.n_lights - 1), (draw_bits(st_l) * (uint32_t)io.n_lights) >> 24);
        [[maybe_unused]] const uint32_t st_k = st_l;  // (after the light choice, which stays xorshift)
        ls_m1 = draw_bits(st_l);
        ls_m2 = draw_bits(st_l);
        if constexpr (kStrat) {
            ls_m1 = first ? fh.z : ls_m1;
            ls_m2 = first ? fh.w : ls_m2;
            st_l = first ? st_k : st_l;
        }
        st = ls_run ? st_l : st;
    }
    [[maybe_unused]] const bool sd = first & isD;  // (no roulette at depth 0: isD is the material)
    uint32_t m1;
    if constexpr (kStrat) {
        uint32_t st_a = st;
        const uint32_t mx = draw_bits(st_a);
        m1 = sd ? fh.x : mx;
        st = sd ? st : st_a;
    } else
    m1 = draw_bits(st);
    bool fres_refl = false;  // dielectric lane reflected by its Fresnel draw (isG & fres & reflect)
    // its value u = m1 2^-24, converted once for the diffuse phi (fast
    // mode: v_sin / v_cos take revolutions) and the Fresnel compare
    const float u1 = (float)m1 * 0x1p-24f;
    // every lane sets it below (exact mode: reflecting lanes in the spec
    // block; fast mode: the diffuse/dielectric block forms every material's
    // direction, the spec block serves the waves that skip it)
    f3 nd = d;
    // a wave with only mirror lanes skips the diffuse/dielectric work
    // (wave-uniform, exact: those lanes' values are all overwritten)
    // (the active lanes less the mirror lanes' mask, which the spec compare
    // above already formed: a ballot of isD | isG was materialised as
    // v_cndmask + v_cmp, one of mat != PTG_SPECULAR as another compare;
    // killed lanes of those materials run the block for nothing, their
    // values unused)
    const bool dg_wave = (__ballot(1) & ~__ballot(mat == PTG_SPECULAR)) != 0ull;
    if (dg_wave)
    {
        PTG_STAT(4);
#if PTG_BLOCK_STATS == 3  // debug: wave cycles of the diffuse/dielectric block in [14]
        const unsigned long long dg_t0 = clock64();
#endif
        {
        // the second xorshift step, once for every lane of the block: the
        // diffuse r and the draw of a reflection chosen by the Fresnel draw
        // are the same step of the same state (st right after m1).  The
        // lanes that take it -- diffuse, Fresnel-reflected -- adopt st2 in
        // the one select after the Fresnel block; killed, mirror, totally
        // reflected and refracting lanes keep st.
        uint32_t st2 = st;
        uint32_t m2 = draw_bits(st2);
        if constexpr (kStrat)
            m2 = sd ? fh.y : m2;
        // read only where isD (the ?: operands and the isD branch below):
        // no initial values to set for the other lanes
        float cp, sp, ra;
        if (isD) {  // main.cpp:46-47: phi = 2 pi u, r = u
            const uint32_t m_phi = m1;
            ra = (float)m2 * 0x1p-24f;  // draw()'s value of the shared step
            if constexpr (!kExact) {
                cp = __builtin_amdgcn_cosf(u1);  // Math<false>::sincos2pi of m1
                sp = __builtin_amdgcn_sinf(u1);
            } else
            Math<kExact>::sincos2pi(m_phi, trig, cp, sp);
        }
        // op1: diffuse -> u = norm((|w.x| > 0.1 ? y : x) x w) (main.cpp:52); dielectric -> norm(d) (main.cpp:75)
        f3 uu = __builtin_fabsf(nn.x) > 0.1f ? mk3(nn.z, 0.0f, -nn.x) : mk3(0.0f, -nn.z, nn.y);
        const f3 v1raw = isD ? uu : d;
        const float r1 = Math<kExact>::rsqrt(dot3(v1raw, v1raw));
        // (fast mode: the normalising multiply waits for the Fresnel block --
        // a reflecting lane keeps its d as it is; nothing before reads v1)
        [[maybe_unused]] f3 v1 = v1raw;
        if constexpr (kExact)
            v1 = mk3(v1raw.x * r1, v1raw.y * r1, v1raw.z * r1);
        // (fast mode: only dielectric lanes read x0, and there v1 = d r1, so
        // v1.nn = (nn.d) r1 = kn r1 -- the dot the mirror already uses)
        const float x0 = kExact ? -dot3(v1, nn) : -(kn * r1);
        // fast mode: one v_min_f32 (differs from the select only for NaN)
        const float cthG = kExact ? (1.0f < x0 ? 1.0f : x0) : __builtin_fminf(1.0f, x0);  // main.cpp:77
        // op2: diffuse -> sin theta = sqrt(r); dielectric -> sin theta = sqrt(1 - cos^2)
        // (fast mode: the argument is >= 0 on every lane that reads s2 --
        // ra >= 0, and 0 < x0 <= 1 + rounding on a dielectric lane (nn faces
        // the ray), so cthG <= 1 and 1 - cthG^2 >= 0 -- so sqrt0's clamp of
        // negative inputs is left out)
        const float s2 = kExact ? Math<kExact>::sqrt0(isD ? ra : __builtin_fmaf(-cthG, cthG, 1.0f))
                                : Math<kExact>::sqrt(isD ? ra : __builtin_fmaf(-cthG, cthG, 1.0f));
        const float ratio = front ? 0.5f : 2.0f;  // main.cpp:72
        // fast mode: ratio sin theta once, for the refraction test and |r_out_perp| below
        [[maybe_unused]] const float rs2 = kExact ? 0.0f : ratio * s2;
        if (isG) {
            bool reflect = (kExact ? ratio * s2 : rs2) > 1.0f;  // cannot refract: no Fresnel draw (main.cpp:89)
            if (!reflect) {
                const float r0 = 0x1.c71c74p-4f;  // ((1-ratio)/(1+ratio))^2, equal for ratio 0.5 and 2
                float xm = 1.0f - cthG;
                float x2 = xm * xm;
                float x5 = (x2 * x2) * xm;
                float R = __builtin_fmaf(1.0f - r0, x5, r0);
                reflect = R > u1;
                fres_refl = reflect;  // (the reflection's draw after this one: st2, selected below)
            }
            spec = reflect;
        }
        // one select for the shared second step (lane masks combined by the scalar unit)
        if constexpr (kStrat)
            st = ((isD & !sd) || fres_refl) ? st2 : st;
        else
        st = (isD || fres_refl) ? st2 : st;
        // op3: diffuse -> cos theta = sqrt(1 - r); dielectric -> |r_out_parallel| (main.cpp:94)
        if constexpr (!kExact) {
            // One direction for every material of the block, as a linear
            // combination of nn, vv = nn x v1 and v1:
            //   diffuse     nn s3 + vv ss + v1 cs                (main.cpp:53-55)
            //   reflection  d - 2 kn nn                          (main.cpp:60-67; v1 = d, not normalised)
            //   refraction  r_out_perp - nn s3 with r_out_perp = (nn cthG + v1) ratio (main.cpp:93-96),
            //               = nn (ratio cthG - s3) + v1 ratio
            // in the operation order of the diffuse line.  A diffuse lane
            // runs its earlier operations on its earlier values; so does a
            // reflecting lane (vv 0 + d 1 is d, then fma(nn, -2 kn, d)), the
            // mirror spheres' lanes included; a refracting lane rounds the
            // same vector differently (three roundings either way).  ratio
            // cthG - s3 does not cancel: entering (ratio 0.5) ratio cthG <=
            // 0.5 and s3 = sqrt(1 - sin^2 theta / 4) >= 0.866; leaving
            // (ratio 2) a lane refracts only where 2 sin theta <= 1, so
            // ratio cthG >= 1.732 and s3 <= 1.
            const float rsel = spec ? 1.0f : r1;  // spec is final here
            v1 = mk3(v1raw.x * rsel, v1raw.y * rsel, v1raw.z * rsel);
            // (nn and v1 are unit and v1.nn = -cos theta, so |r_out_perp|^2 =
            // ratio^2 (1 - cos^2 theta) = rs2^2 -- one fma for the dot and
            // its subtraction, r_out_perp itself never formed.  The one
            // assumption added: cthG is the un-clamped x0 wherever the clamp
            // does not bind, which is where s2^2 is 1 - x0^2; then rs2^2 and
            // |r_out_perp|^2 differ by roundings only.  Where it binds,
            // cthG = 1 and s2 = 0: the argument is 1, r_out_perp is within
            // rounding of 0.)
            const float gq = __builtin_fmaf(-rs2, rs2, 1.0f);
            const float s3 = Math<kExact>::sqrt(isD ? 1.0f - ra : __builtin_fabsf(gq));  // both arguments >= 0
            const f3 vv = cross3(nn, v1);
            const float k3r = -(kn + kn), k3t = __builtin_fmaf(ratio, cthG, -s3);
            const float K3 = isD ? s3 : (spec ? k3r : k3t);
            const float K2 = isD ? sp * s2 : 0.0f;
            const float K1 = isD ? cp * s2 : (spec ? 1.0f : ratio);
            // (written to d itself, whose last reader was v1: formed in
            // registers of its own, the result took three copies per
            // iteration to reach the loop-carried d)
            d = mk3(__builtin_fmaf(nn.x, K3, __builtin_fmaf(vv.x, K2, v1.x * K1)),
                    __builtin_fmaf(nn.y, K3, __builtin_fmaf(vv.y, K2, v1.y * K1)),
                    __builtin_fmaf(nn.z, K3, __builtin_fmaf(vv.z, K2, v1.z * K1)));
            nd = d;
        } else {
            const f3 perp = mk3(__builtin_fmaf(nn.x, cthG, v1.x) * ratio, __builtin_fmaf(nn.y, cthG, v1.y) * ratio,
                                __builtin_fmaf(nn.z, cthG, v1.z) * ratio);
            const float s3 = Math<kExact>::sqrt(isD ? 1.0f - ra : __builtin_fabsf(1.0f - dot3(perp, perp)));
            if (isD) {  // main.cpp:53-55 (unit by construction, not re-normalised)
                f3 vv = cross3(nn, v1);
                float cs = cp * s2, ss = sp * s2;
                nd = mk3(__builtin_fmaf(nn.x, s3, __builtin_fmaf(vv.x, ss, v1.x * cs)),
                         __builtin_fmaf(nn.y, s3, __builtin_fmaf(vv.y, ss, v1.y * cs)),
                         __builtin_fmaf(nn.z, s3, __builtin_fmaf(vv.z, ss, v1.z * cs)));
            } else {  // refraction, main.cpp:93-96
                nd = mk3(__builtin_fmaf(nn.x, -s3, perp.x), __builtin_fmaf(nn.y, -s3, perp.y),
                         __builtin_fmaf(nn.z, -s3, perp.z));
            }
        }
        }
#if PTG_BLOCK_STATS == 3
        {
            const unsigned long long dg_t1 = clock64();
            if (__lane_id() == __ffsll((long long)__ballot(1)) - 1)
                atomicAdd(&ptg_dbg_stats[(blockIdx.x & 255) * 16 + 14], dg_t1 - dg_t0);
        }
#endif
    }
    // fast mode: the block above formed the reflecting lanes' direction as
    // well, so the mirror's own code is that block's wave-uniform else -- a
    // wave of mirror lanes only (frequent in box_mirror's tube of mirror
    // walls); box waves never execute it
    if (kExact || !dg_wave)
    if (spec) {  // main.cpp:60-67 (fuzz draw consumed, multiplied by 0)
        PTG_STAT(5);
        // (fast mode: an empty statement that the compiler may not execute
        // speculatively -- without it the two tests above are folded into
        // one select and every wave runs this block's arithmetic again)
        if constexpr (!kExact)
            asm volatile("");
        // (fast mode: on the facing normal nn = +-on, its dot kn)
        float k = !kExact ? kn : dot3(on, d);
        k = k + k;
        // (the reflection's draw after a Fresnel draw: the block's shared second step)
        const f3 rn = !kExact ? nn : on;
        nd = mk3(__builtin_fmaf(-k, rn.x, d.x), __builtin_fmaf(-k, rn.y, d.y), __builtin_fmaf(-k, rn.z, d.z));
    }
    if constexpr (kLS) {
        io.skip_next = ls_run;
        io.to_shadow = false;
        if (ls_run) {
            const LightRec *lr = io.lights + ls_k;
            const float4 lc = lr->c, le = lr->e;
            const f3 w = mk3(lc.x - p.x, lc.y - p.y, lc.z - p.z);
            const float d2 = dot3(w, w);
            // (a point inside the light, d2 <= R^2 -- a dome light, a lamp of
            // emissive glass: nothing here; the next hit can only meet that
            // light from the back, where its emission is not skipped)
            if (d2 > lc.w && io.hid != __float_as_int(le.w)) {
                const float q = Math<kExact>::div(lc.w, d2);
                const float omc = Math<kExact>::div(q, 1.0f + Math<kExact>::sqrt0(1.0f - q));  // 1 - cos theta_max
                const float a = ((float)ls_m1 * 0x1p-24f) * omc;
                const float ct = 1.0f - a;
                const float sth = Math<kExact>::sqrt0(a * (2.0f - a));
                float cph, sph;
                Math<kExact>::sincos2pi(ls_m2, trig, cph, sph);
                const float iw = Math<kExact>::rsqrt(d2);
                const f3 sw = mk3(w.x * iw, w.y * iw, w.z * iw);
                // the diffuse sampler's basis rule (main.cpp:52) around sw
                const f3 su = norm3m<kExact>(__builtin_fabsf(sw.x) > 0.1f ? mk3(sw.z, 0.0f, -sw.x)
                                                                          : mk3(0.0f, -sw.z, sw.y));
                const f3 sv = cross3(sw, su);
                const float kc = cph * sth, ks = sph * sth;
                const f3 l = mk3(__builtin_fmaf(sw.x, ct, __builtin_fmaf(sv.x, ks, su.x * kc)),
                                 __builtin_fmaf(sw.y, ct, __builtin_fmaf(sv.y, ks, su.y * kc)),
                                 __builtin_fmaf(sw.z, ct, __builtin_fmaf(sv.z, ks, su.z * kc)));
                const float cs = dot3(nn, l);
                if (cs > 0.0f) {
                    const float wgt = ((cs + cs) * omc) * (float)io.n_lights;
                    ls.pend = mk3((T.x * le.x) * wgt, (T.y * le.y) * wgt, (T.z * le.z) * wgt);
                    ls.nd = nd;
                    ls.light = __float_as_int(le.w);
                    nd = l;
                    io.to_shadow = true;
                }
            }
        }
    }
    o = p;
    d = nd;
    return killed | (depth >= kDepthLimit);
}
