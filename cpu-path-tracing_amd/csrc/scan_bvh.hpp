// scan_bvh.hpp -- the nearest-hit scan of BVH scenes (more than kLinearMax
// spheres): root_lex / update_lex (the reference's nearest-hit rule), the
// resumable per-lane walk (BvhTrav, SlabRay, bvh_start, bvh_node_step), the
// leaf phase (bvh_leaf, bvh_leaf_split) and the whole-ray scene_scan_bvh.
// Included by ptg_render.hip inside its unnamed namespace, after
// scan_linear.hpp; needs ScanCount and kCullMargin from it, KArgs
// (kernel_args.hpp), the node layout (bvh_build.hpp) and Math (pt_device.hpp).
// Owns no switch; reads PTG_BVH_STACK, PTG_LEAF_SPLIT, PTG_LONG_LEAF and
// PTG_WAVE_STATS (render_config.hpp).
#pragma once

// Scenes with more than kLinearMax spheres: the huge
// spheres linearly, then a stackless walk of the BVH.  The nearest-hit rule
// here is the reference's own -- every candidate root is divided,
// t = fl(num/den), and the winner is the smallest t, lowest scene index on
// ties (main.cpp:35 strict <, in index order) -- which does not depend on the
// visiting order, so the oracle reproduces it with a linear scan.  Box tests
// only cull: boxes are padded (bvh_build.hpp) and use fast reciprocals.

// Root of one sphere under the reference's rule (the root >= eps nearest to
// the origin, t = fl(num/den)); NaN when rejected or provably not below tb
// (the two exact culls of DESIGN.md "scene scan").  kBig: anchored form with
// g0 = {P0, R}, g1 = {n0, 2R} (huge spheres); else g0 = {C, -R^2}.
constexpr float kReject = __builtin_nanf("");  // every comparison with it is false

// the cull's scaled culling distance: tb * -2 (1 + 2^-20), exact constant
constexpr float kCullScale = -2.0f * kCullMargin;

template <bool kBig, bool kExact>
__device__ __forceinline__ float root_lex(const float4 g0, const float4 g1, const f3 o, const f3 d, const float a,
                                          const float tb, const float tbm)
{
    f3 e = mk3(o.x - g0.x, o.y - g0.y, o.z - g0.z);
    float ed = dot3(e, d);
    float ee = dot3(e, e);
    float hb, c;
    if constexpr (kBig) {
        hb = __builtin_fmaf(g0.w, dot3(mk3(g1.x, g1.y, g1.z), d), ed);
        c = __builtin_fmaf(g1.w, dot3(e, mk3(g1.x, g1.y, g1.z)), ee);
    } else {
        hb = ed;
        c = ee + g0.w;  // g0.w = -R^2
    }
    // the two culls and the discriminant test as one early-out (bitwise: the
    // && chains had been evaluated as nested exec-masked blocks; C5 -1.1 %)
    // The two culls as one compare: behind (hb >= 0, c >= 0) and beyond (hb
    // < 0, near root > tb: c >= 2 |hb| tb (1 + 2^-20); the margin covers the q
    // bound's 3u and the two roundings) are c >= max(hb tbm, 0) with tbm = tb
    // * kCullScale < 0 from the caller (once per change of tb): hb tbm <= 0
    // for hb >= 0 (NaN for hb = 0, tb = inf: fmax gives 0), > 0 for hb < 0.
    // (As two sign-selected compares the choice was materialised: 5 VALU.)
    const bool culled = c >= __builtin_fmaxf(hb * tbm, 0.0f);
    float disc;
    if constexpr (kBig) {
        disc = __builtin_fmaf(hb, hb, -(a * c));
    } else {
        // Lagrange form (scene_scan), limited to hb^2 for an origin outside
        // (c >= 0: exactly disc <= hb^2), which keeps q <= 2|hb|(1 + 3u)
        // and so the cull above exact
        const f3 x = cross3(e, d);
        disc = __builtin_fmaf(a, -g0.w, -dot3(x, x));
        disc = c >= 0.0f ? __builtin_fminf(disc, hb * hb) : disc;
    }
    if (culled | (disc < 0.0f))
        return kReject;
    const float sq = Math<kExact>::sqrt(disc);  // disc >= 0 here
    // the near root c/q (hb < 0, q = sq - hb), else the far root q/a, or -c/qn
    // (hb >= 0, qn = hb + sq) -- as selects (scene_scan's form: sq - hb and
    // hb + sq are the IEEE add sq + |hb|; one eps test covers the three cases),
    // not two divergent branches that a wave with both signs ran one after
    // the other
    const bool neg = hb < 0.0f;
    const float qq = sq + __builtin_fabsf(hb);
    const bool near_lt = c < kEps * qq;
    const float num = neg ? (near_lt ? qq : c) : -c;
    const float den = (neg & near_lt) ? a : qq;
    if (num < kEps * den)
        return kReject;
    if constexpr (kExact)
        return num / den;  // IEEE: the oracle's intersect_B_lex
    else
        return Math<false>::div(num, den);
}

// The BVH scan's winner is its scene index (-1: none).  Ties of t go to the
// lowest scene index (main.cpp:35: strict < in index order), which makes the
// result independent of the visiting order: the oracle's linear scan
// (intersect_B_lex) gives the same bits.
__device__ __forceinline__ void update_lex(const float t, const int sid, float &tb, int &best)
{
    // a NaN t (rejected) fails both compares; (unsigned) -1 orders after every
    // index.  Selects, not a short-circuit && / || (exec-masked blocks)
    const bool win = (t < tb) | ((t == tb) & ((unsigned)sid < (unsigned)best));
    tb = win ? t : tb;
    best = win ? sid : best;
}

// Per-lane BVH scan state.  The render kernel keeps it across iterations of
// its main loop (resumable scan): lanes whose scan ends early shade and start
// their next segment while the wave keeps walking for the long rays -- a
// wave otherwise waits for its slowest ray (measured 93 wave-level node
// steps for 33 per ray on the 10,000-sphere scene).
// global (address space 1) pointers: kernel-argument pointers pinned in
// SGPRs lose their address space, and generic (flat) loads also wait on LDS
template <class T>
using gptr = const T __attribute__((address_space(1))) *;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // a compact node record, loadable from gptr

struct BvhTrav {
    int ni;    // binary: next node in depth-first order; wide: see below
    int pend;  // parked leaf (first | count << 24) or -1
    float tb;  // nearest root so far
    int best;  // winner's scene index or -1
    // wide walk: ni = the next position (a wide node's first record + the
    // slot to resume from, >= 0), -1 (walk finished), or -- only while a leaf
    // is parked -- kPopLater (-2: pop the stack after the leaf phase) or a
    // leaf word (parked after the leaf phase).  A two-entry stack (top first, -1 empty)
    // of positions / leaf words still to visit; when it overflows it is
    // cleared and the walk continues, once it runs dry, from the resume
    // position `res` and its continuation chain (bvh_build.hpp wide_conts:
    // everything after it in depth-first order, culled by tb), so any tree
    // depth is walked correctly with three registers.
    int s0, s1;
#if PTG_BVH_STACK >= 3
    int s2;
#endif
    int res;
};

__device__ __forceinline__ bool bvh_done(const KArgs &, const BvhTrav &tr) { return (tr.ni == -1) & (tr.pend < 0); }
__device__ __forceinline__ int bvh_pop(gptr<int> cont, BvhTrav &tr)
{
    const int v = tr.s0;
    tr.s0 = tr.s1;
#if PTG_BVH_STACK >= 3
    tr.s1 = tr.s2;
    tr.s2 = -1;
#else
    tr.s1 = -1;
#endif
    if (v != -1)
        return v;
    const int r = tr.res;  // stack dry: the resume position, then its continuation
    if (r != -1)
        tr.res = cont[r >> 2];
    return r;
}

// Start a scan: the huge spheres (tested linearly, first), then the BVH in
// the layout of the ray's direction octant.
template <bool kCount, bool kExact>
__device__ __forceinline__ void bvh_start(const KArgs &A, f3 o, f3 d, BvhTrav &tr, ScanCount &cnt)
{
    const float a = dot3(d, d);
    tr.tb = kInf;
    tr.best = -1;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(4))) f32x4 *cvec_t;
    typedef const __attribute__((address_space(4))) int *cint_t;
    const cvec_t bgeo = (cvec_t)A.big_geo;  // GeoRec k: words 2 k, 2 k + 1
    const cint_t bid = (cint_t)A.big_id;
    for (int k = 0; k < A.n_big; ++k) {
        const f32x4 v0 = bgeo[2 * k], v1 = bgeo[2 * k + 1];
        const float4 g0 = make_float4(v0.x, v0.y, v0.z, v0.w), g1 = make_float4(v1.x, v1.y, v1.z, v1.w);
        update_lex(root_lex<true, kExact>(g0, g1, o, d, a, tr.tb, tr.tb * kCullScale), bid[k], tr.tb, tr.best);
    }
    if constexpr (kCount)
        cnt.spheres += A.n_big;
    // the wide layouts store each box near-plane first for their octant:
    // all 8 layouts exist
    const unsigned oct = (__float_as_uint(d.x) >> 31) | ((__float_as_uint(d.y) >> 30) & 2u) |
                         ((__float_as_uint(d.z) >> 29) & 4u);
    tr.ni = A.n_nodes > 0 ? (int)(oct << 2) : -1;  // layout k's root: interleaved node k
    tr.s0 = -1;
    tr.s1 = -1;
#if PTG_BVH_STACK >= 3
    tr.s2 = -1;
#endif
    tr.res = -1;
    tr.pend = -1;
}

// Slab-test constants of a ray in the compact nodes' grid units (culling
// only: fast reciprocals, boxes padded and rounded outward):
// t = q * (scale / d) + (lo - o) / d.
struct SlabRay {
    float sx, sy, sz, bx, by, bz;
};
__device__ __forceinline__ SlabRay slab_ray(const KArgs &A, f3 o, f3 d)
{
    const float ix = d.x != 0.0f ? __builtin_amdgcn_rcpf(d.x) : __builtin_copysignf(1e30f, d.x);
    const float iy = d.y != 0.0f ? __builtin_amdgcn_rcpf(d.y) : __builtin_copysignf(1e30f, d.y);
    const float iz = d.z != 0.0f ? __builtin_amdgcn_rcpf(d.z) : __builtin_copysignf(1e30f, d.z);
    SlabRay r;
    r.sx = A.q_scale[0] * ix;
    r.sy = A.q_scale[1] * iy;
    r.sz = A.q_scale[2] * iz;
    r.bx = (A.q_lo[0] - o.x) * ix;
    r.by = (A.q_lo[1] - o.y) * iy;
    r.bz = (A.q_lo[2] - o.z) * iz;
    return r;
}


// Box test of a wide-layout record: binary16 planes on the wide grid, stored
// near-plane first for the ray's octant (bvh_build.hpp WideGrid), each read
// by one v_fma_mix_f32.  No slab margin: the boxes are padded far beyond the
// rounding of the slab times (bvh_build.hpp); tcap keeps the 1e-4 margin
// over the nearest root.
// binary16 halves of a word as float: folded into v_fma_mix_f32 operands.
// (A __builtin_bit_cast of the word to a 2 x _Float16 vector miscompiles
// here: every plane was read from the record's first word.)
__device__ __forceinline__ float lo_half(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu)); }
__device__ __forceinline__ float hi_half(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
__device__ __forceinline__ bool box_hit_sorted(const u32x4 q, const SlabRay &r, const float tcap)
{
    const float tnx = __builtin_fmaf(lo_half(q.x), r.sx, r.bx);
    const float tny = __builtin_fmaf(hi_half(q.x), r.sy, r.by);
    const float tnz = __builtin_fmaf(lo_half(q.y), r.sz, r.bz);
    const float tfx = __builtin_fmaf(hi_half(q.y), r.sx, r.bx);
    const float tfy = __builtin_fmaf(lo_half(q.z), r.sy, r.by);
    const float tfz = __builtin_fmaf(hi_half(q.z), r.sz, r.bz);
    const float t_in = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), __builtin_fmaxf(tnz, 0.0f));
    // tcap by its own compare: as a min operand it came from outside the
    // node step's block, so the compiler re-canonicalised it (v_max x, x) in
    // every step; the slab times are fresh v_fma_mix results
    const float t_out = __builtin_fminf(__builtin_fminf(tfx, tfy), tfz);
    return !(t_in > t_out) & !(t_in > tcap);
}

// One wide node step at position ni (node + first slot): the node's 4
// records (one 64-B line) in one go.  Slots are in near-first order for the
// layout's octant.  The nearest hit child is visited next -- or, when it is a
// leaf, parked in tr.pend and the second hit visited next; of the hits after
// that one goes on the stack as itself, several as the position of the first
// (the node is re-tested from there, with the culling distance of then).
// With no successor the stack is popped -- at most once per step, and not
// when a leaf was parked: ni = kPopLater then, and the leaf phase pops.
// Selections are branch-free (v_cndmask).
constexpr int kPopLater = -2;
__device__ __forceinline__ int bvh_pop_sel(gptr<int> cont, BvhTrav &tr, const bool need, const int keep);
template <bool kCount>
__device__ __forceinline__ void bvh_node_step(gptr<int> cont, gptr<u32x4> qnodes, const SlabRay &r_in, BvhTrav &tr,
                                              ScanCount &cnt)
{
    const int base = tr.ni & ~3;
    u32x4 q0, q1, q2, q3;
    const SlabRay &r = r_in;
    {
        // a 32-bit byte offset on the uniform base: the load's saddr form
        // (no 64-bit address arithmetic per lane)
        gptr<u32x4> q = (gptr<u32x4>)((const __attribute__((address_space(1))) char *)qnodes + ((unsigned)base << 4));
        q0 = q[0];
        q1 = q[1];
        q2 = q[2];
        q3 = q[3];
    }
    if constexpr (kCount)
        cnt.boxes += 4 - (tr.ni & 3);
    const float tcap = tr.tb * 1.0001f;
    // slots before the walk's position (ni & 3) are not tested again
    const int s = tr.ni & 3;
    const bool h0 = box_hit_sorted(q0, r, tcap) & (s == 0), h1 = box_hit_sorted(q1, r, tcap) & (s <= 1),
               h2 = box_hit_sorted(q2, r, tcap) & (s <= 2), h3 = box_hit_sorted(q3, r, tcap);
    // the words of the first three hits in slot order (-1: none) and the
    // slots of the second and third, shifted in from the last slot: every
    // step is a v_cndmask on its box test's lane mask (the hit mask with
    // lowest-set-bit lookups took 10-16 VALU more per node step: C5 +4.8 %)
    int w1 = h3 ? (int)q3.w : -1, w2 = -1, w3 = -1;
    w2 = h2 ? w1 : w2;
    w1 = h2 ? (int)q2.w : w1;
    w3 = h1 ? w2 : w3;
    w2 = h1 ? w1 : w2;
    w1 = h1 ? (int)q1.w : w1;
    w3 = h0 ? w2 : w3;
    w2 = h0 ? w1 : w2;
    w1 = h0 ? (int)q0.w : w1;
    int i2 = 3, i3 = 3;  // (meaningful only where the hit exists)
    i3 = h1 ? i2 : i3;
    i2 = h1 ? (h2 ? 2 : 3) : i2;
    i3 = h0 ? i2 : i3;
    i2 = h0 ? (h1 ? 1 : h2 ? 2 : 3) : i2;
    const bool leaf = w1 < kPopLater;  // the first hit is a leaf: parked (no hit: w1 = -1)
    int next = leaf ? (w2 != -1 ? w2 : kPopLater) : w1;
    tr.pend = leaf ? (w1 & 0x7FFFFFFF) : tr.pend;
    // the hits left after next: from the second (an inner first hit) or the
    // third (a parked leaf); one goes on the stack as its word, several as
    // the position of the first of them
    // (each select on one lane mask: a select between two conditions was
    // materialised as 5 VALU)
    const bool push = leaf ? w3 != -1 : w2 != -1;
    const int pos = base + (leaf ? i3 : i2);
    const int e = leaf ? ((h0 & h1 & h2 & h3) ? pos : w3) : (w3 != -1 ? pos : w2);
#if PTG_BVH_STACK >= 3
    const bool full = tr.s2 != -1;
    tr.res = (push & full) ? pos : tr.res;
    const int s0 = tr.s0, s1 = tr.s1;
    tr.s0 = push ? (full ? -1 : e) : s0;
    tr.s1 = push ? (full ? -1 : s0) : s1;
    tr.s2 = push ? (full ? -1 : s1) : tr.s2;
#else
    const bool full = tr.s1 != -1;
    tr.res = (push & full) ? pos : tr.res;
    const int s0 = tr.s0;
    tr.s0 = push ? (full ? -1 : e) : s0;
    tr.s1 = push ? (full ? -1 : s0) : tr.s1;
#endif
    if (next == -1) {
        next = bvh_pop(cont, tr);
        if (next < kPopLater) {  // a leaf from the stack
            tr.pend = next & 0x7FFFFFFF;
            next = kPopLater;
        }
    }
    tr.ni = next;
}

// The render kernel's leaf completion (bvh_leaf_done) and its pop, executed
// by every lane of the wave: lanes without a tested leaf (act false) keep
// their state through selects.  As nested divergent branches the update
// merged the traversal state through exec-masked copies (39 v_mov per leaf
// phase in the ISA); same values, C5 -0.5 %.
//
// Pop where need (else return keep): the stack top, or once it runs dry the
// resume position and its continuation -- the one load stays behind a branch
// (rare: the two-entry stack overflowed earlier).
__device__ __forceinline__ int bvh_pop_sel(gptr<int> cont, BvhTrav &tr, const bool need, const int keep)
{
    const int v = tr.s0, r = tr.res;
    const bool dry = v == -1;
    int nres = r;
    if (need & dry & (r != -1))
        nres = cont[r >> 2];
    tr.s0 = need ? tr.s1 : v;
#if PTG_BVH_STACK >= 3
    tr.s1 = need ? tr.s2 : tr.s1;
    tr.s2 = need ? -1 : tr.s2;
#else
    tr.s1 = need ? -1 : tr.s1;
#endif
    tr.res = nres;
    return need ? (dry ? r : v) : keep;
}

// bvh_leaf_done for the lanes whose parked leaf was tested (act)
__device__ __forceinline__ void bvh_leaf_done_sel(gptr<int> cont, BvhTrav &tr, const bool act)
{
    tr.pend = act ? -1 : tr.pend;
    int next = bvh_pop_sel(cont, tr, act & (tr.ni == kPopLater), tr.ni);
    const bool lf = act & (next < kPopLater);  // a leaf word (popped, or waiting in ni)
    tr.pend = lf ? (next & 0x7FFFFFFF) : tr.pend;
    next = lf ? kPopLater : next;
    tr.ni = act ? next : tr.ni;
}

// Spheres [f, f + cnt) of the leaf order against one ray: compact records
// {C, -R^2}; (tb, best) updated by the lex rule.
template <bool kCount, bool kExact>
__device__ __forceinline__ void leaf_spheres(const KArgs &A, int f, int cnt, f3 o, f3 d, float &tb, int &best,
                                             ScanCount &sc)
{
    const float a = dot3(d, d);
    if constexpr (kCount)
        sc.spheres += cnt;
    // 32-bit byte offsets on the uniform bases (saddr loads)
    const char *sph = (const char *)A.bvh_sph;
    const char *ids = (const char *)A.bvh_id;
    float tbm = tb * kCullScale;
    for (int j = 0; j < cnt; ++j) {
        const unsigned off = (unsigned)(f + j) << 4;
        const float4 rec = *(const float4 *)(sph + off);
        const float t = root_lex<false, kExact>(rec, float4{}, o, d, a, tb, tbm);
        if (t <= tb) {  // the scene index is read only for a candidate that wins or ties
            update_lex(t, *(const int *)(ids + (off >> 2)), tb, best);
            tbm = tb * kCullScale;
        }
    }
}

// After the parked leaf's spheres: wide walk -- a leaf word waiting in tr.ni
// is parked next, or the pop deferred by the node step happens.
__device__ __forceinline__ void bvh_leaf_done(gptr<int> cont, BvhTrav &tr)
{
    tr.pend = -1;
    if (tr.ni < -1) {  // kPopLater, or the leaf the node step moved to after parking one
        int next = tr.ni == kPopLater ? bvh_pop(cont, tr) : tr.ni;
        if (next < kPopLater) {  // a leaf: parked for the next leaf phase
            tr.pend = next & 0x7FFFFFFF;
            next = kPopLater;
        }
        tr.ni = next;
    }
}

// The parked leaf's spheres, all by this lane.
template <bool kCount, bool kExact>
__device__ __forceinline__ void bvh_leaf(const KArgs &A, gptr<int> cont, f3 o, f3 d, BvhTrav &tr, ScanCount &cnt)
{
    const int first = tr.pend & 0xFFFFFF, nl = tr.pend >> 24;
    const int take = nl;
    leaf_spheres<kCount, kExact>(A, first, take, o, d, tr.tb, tr.best, cnt);
    if (take < nl) {
        tr.pend = (first + take) | ((nl - take) << 24);
        return;
    }
    bvh_leaf_done(cont, tr);
}

// Leaf phase with helpers (PTG_LEAF_SPLIT; called by the whole wave): lanes
// with no leaf to test are assigned, by rank, to lanes holding a leaf of >= 2
// spheres -- one helper per such leaf, longest leaves (>= PTG_LONG_LEAF spheres: they set
// the wave's loop length) first, then a second helper per long leaf while
// idle lanes remain.  A helper tests its part of the leaf with the owner's
// ray and culling distance (ds_bpermute) and the owner merges the helpers'
// nearest roots by the same lex rule -- order-independent, so the result is
// the one-lane result bit for bit.  pair: 2 x 64 bytes of LDS (owner lane by
// owner rank, helper lane by helper rank).
template <bool kCount, bool kExact>
__device__ __forceinline__ void bvh_leaf_split(const KArgs &A, gptr<int> cont, f3 o, f3 d, bool has,
                                               unsigned long long mhas, BvhTrav &tr, ScanCount &cnt,
                                               uint8_t (*pair)[64])
{
    const int lane = (int)__lane_id();
    const int nl = has ? (tr.pend >> 24) : 0;
    const bool own = nl >= 2, hlp = !has;
    auto rank = [](unsigned long long m) {
        return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    };
    const bool longl = nl >= PTG_LONG_LEAF;
    // (mhas = ballot(has), the whole wave active: ballots of single compares only)
    const unsigned long long ml = __ballot(longl), ms = __ballot(own) & ~ml, mh = ~mhas;
    const int nlong = (int)__popcll(ml), nown = nlong + (int)__popcll(ms), nhelp = (int)__popcll(mh);
    const int np1 = min(nown, nhelp);  // owners (by rank) with a first helper
#if PTG_LEAF_SPLIT >= 2
    const int np2 = max(0, min(nlong, nhelp - nown));  // long-leaf owners with a second helper
#else
    const int np2 = 0;
#endif
    const int ro = longl ? rank(ml) : nlong + rank(ms);
    const int rh = rank(mh);
    const bool po = own & (ro < np1), ph = hlp & (rh < np1 + np2);
    if (po)
        pair[0][ro] = (uint8_t)lane;
    if (ph)
        pair[1][rh] = (uint8_t)lane;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int orank = rh < np1 ? rh : rh - np1;  // a helper's owner, and which helper it is
    const int part = rh < np1 ? 1 : 2;
    const int partner = po ? (int)pair[1][ro] : ph ? (int)pair[0][orank] : lane;
    const int partner2 = (po & (ro < np2)) ? (int)pair[1][np1 + ro] : lane;
    auto bpf = [](int who, float v) {
        return __int_as_float(__builtin_amdgcn_ds_bpermute(who << 2, __float_as_int(v)));
    };
    auto bpi = [](int who, int v) { return __builtin_amdgcn_ds_bpermute(who << 2, v); };
    // helpers take the owner's ray, culling distance and leaf
    const f3 po3 = mk3(bpf(partner, o.x), bpf(partner, o.y), bpf(partner, o.z));
    const f3 pd3 = mk3(bpf(partner, d.x), bpf(partner, d.y), bpf(partner, d.z));
    const float ptb = bpf(partner, tr.tb);
    const int ppend = bpi(partner, tr.pend);
    const f3 ro3 = ph ? po3 : o, rd3 = ph ? pd3 : d;
    const int pendl = ph ? ppend : tr.pend;
    const int first = pendl & 0xFFFFFF, nll = pendl >> 24;
    // the leaf's parts: one helper -> [0, ceil(n/2)), [ceil(n/2), n); two
    // helpers -> [0, n/3), [n/3, 2n/3), [2n/3, n) (n <= 12: x/3 = x*11 >> 5)
    const int k = ph ? 1 + (orank < np2) : po ? 1 + (ro < np2) : 0;
    const int b1 = k == 2 ? (nll * 11) >> 5 : (nll + 1) >> 1;
    const int b2 = k == 2 ? (2 * nll * 11) >> 5 : nll;
    const int lo = !ph ? 0 : part == 1 ? b1 : b2;
    const int hi = !ph ? (po ? b1 : (has ? nll : 0)) : part == 1 ? b2 : nll;
    const int f = first + lo, c = hi - lo;
    float tb = ph ? ptb : tr.tb;
    int best = ph ? -1 : tr.best;
#if PTG_WAVE_STATS == 1  // debug: the wave's loop length
    {
        int mx = c;
        for (int off = 32; off > 0; off >>= 1)
            mx = max(mx, __shfl_xor(mx, off, 64));
        const bool first_lane = lane == __ffsll((long long)__ballot(1)) - 1;
        cnt.spheres += first_lane ? (uint32_t)mx : 0u;
    }
#endif
    leaf_spheres<kCount && !PTG_WAVE_STATS, kExact>(A, f, c, ro3, rd3, tb, best, cnt);
    // owners merge their helpers' nearest roots
    const float htb = bpf(partner, tb), htb2 = bpf(partner2, tb);
    const int hbest = bpi(partner, best), hbest2 = bpi(partner2, best);
    if (po) {
        update_lex(htb, hbest, tb, best);
        update_lex(htb2, hbest2, tb, best);  // partner2 = lane without a second helper: a no-op
    }
    tr.tb = has ? tb : tr.tb;
    tr.best = has ? best : tr.best;
    bvh_leaf_done_sel(cont, tr, has);
}

// Whole scan of one ray (parity probe kernel): walk, testing each parked leaf
// at once.
template <bool kCount, bool kExact>
__device__ __forceinline__ int scene_scan_bvh(const KArgs &A, f3 o, f3 d, float &tbest, ScanCount &cnt)
{
    BvhTrav tr;
    bvh_start<kCount, kExact>(A, o, d, tr, cnt);
    const SlabRay sr = slab_ray(A, o, d);
    while (!bvh_done(A, tr)) {
        if (tr.pend >= 0)
            bvh_leaf<kCount, kExact>(A, (gptr<int>)A.bvh_cont, o, d, tr, cnt);
        else
            bvh_node_step<kCount>((gptr<int>)A.bvh_cont, (gptr<u32x4>)A.bvh_qnodes, sr, tr, cnt);
    }
    tbest = tr.tb;
    return tr.best;
}
