// accum_kernels.hpp -- the kernels that read or index the exact accumulators:
// resolve (resolve_pixel, resolve_kernel, resolve_active_kernel), the noise
// estimates (noise_kernel, select_over_kernel, noise_active_kernel), the
// active list's list_* kernels and bump_counts_kernel.  Included by
// ptg_render.hip inside its unnamed namespace, after render_unit.hpp; needs
// KArgs (kernel_args.hpp), f3 (pt_device.hpp) and out_row_of.  No LDS beyond
// the kernels' own arrays, no switch.
#pragma once

// The pixel value from the exact sums g of its sub-pixels after samps samples
// (main.cpp:195-196): the clamped sub-pixel means added with weight 1/nsub^2
// in (sy, sx) order.  Shared by resolve_kernel (one samps for the slab) and
// resolve_active_kernel (each pixel's own count).
__device__ __forceinline__ f3 resolve_pixel(const KArgs &A, unsigned long long *g, const int &samps, const int &keep)
{
    f3 pix = mk3(0.0f, 0.0f, 0.0f);
    for (int j = 0; j < A.lanes_per_pixel; ++j) {
        float m[3];
        for (int c = 0; c < 3; ++c) {
            unsigned long long sum = g[3 * j + c];
            if (!keep)
                g[3 * j + c] = 0ull;
            float mean = samps > 0 ? (float)(((double)sum * 0x1p-32) / (double)samps) : 0.0f;
            m[c] = mean < 0.0f ? 0.0f : (1.0f < mean ? 1.0f : mean);
        }
        pix = mk3(__builtin_fmaf(m[0], A.inv_sub2, pix.x), __builtin_fmaf(m[1], A.inv_sub2, pix.y),
                  __builtin_fmaf(m[2], A.inv_sub2, pix.z));
    }
    return pix;
}

// main.cpp:195-196 per pixel (resolve_pixel); re-zeroes the accumulator for
// the next frame.
__global__ __launch_bounds__(256) void resolve_kernel(KArgs A)
{
    const long long i = (long long)A.resolve_row0 * A.W + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)A.slab_rows * A.W)
        return;
    const int slab_row = (int)(i / A.W);
    if (out_row_of(A, slab_row) >= A.H)
        return;
    unsigned long long *g = A.acc + (size_t)i * A.lanes_per_pixel * 3;
    const f3 pix = resolve_pixel(A, g, A.samps, A.keep_acc);
    float *out = A.out + (size_t)i * 3;
    out[0] = pix.x;
    out[1] = pix.y;
    out[2] = pix.z;
}

// ptg_resolve_active_device: resolve_kernel's arithmetic with each pixel's
// own sample count (0 samples: 0); the sums are kept.
__global__ __launch_bounds__(256) void resolve_active_kernel(KArgs A, const int *__restrict__ counts)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)A.slab_rows * A.W)
        return;
    if (out_row_of(A, (int)(i / A.W)) >= A.H)
        return;
    const int np = counts[i], keep = 1;
    const f3 pix = resolve_pixel(A, A.acc + (size_t)i * A.lanes_per_pixel * 3, np, keep);
    float *out = A.out + (size_t)i * 3;
    out[0] = pix.x;
    out[1] = pix.y;
    out[2] = pix.z;
}

// include/ptgpu.h "per-pixel noise estimates": from a pixel's exact sums g1
// (S1) and g2 (S2) after n >= 2 samples, the variance V[3] of its value and
// its relative standard error.  Shared by noise_kernel (one n for the slab)
// and select_over_kernel (each pixel's own count).
__device__ __forceinline__ float noise_pixel(const KArgs &A, const unsigned long long *g1,
                                             const unsigned long long *g2, const double n, const double floor,
                                             double V[3])
{
    f3 pix = mk3(0.0f, 0.0f, 0.0f);
    double vs[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < A.lanes_per_pixel; ++j) {
        float m[3];
        for (int c = 0; c < 3; ++c) {
            const double m1 = ((double)g1[3 * j + c] * 0x1p-32) / n;
            const double m2 = ((double)g2[3 * j + c] * 0x1p-32) / n;
            const float mean = (float)m1;
            m[c] = mean < 0.0f ? 0.0f : (1.0f < mean ? 1.0f : mean);
            double v = m2 - m1 * m1;
            v = (v > 0.0 ? v : 0.0) / (n - 1.0);
            vs[c] += v < 0.25 ? v : 0.25;
        }
        pix = mk3(__builtin_fmaf(m[0], A.inv_sub2, pix.x), __builtin_fmaf(m[1], A.inv_sub2, pix.y),
                  __builtin_fmaf(m[2], A.inv_sub2, pix.z));
    }
    const double w = (double)A.inv_sub2 * (double)A.inv_sub2;
    V[0] = w * vs[0];
    V[1] = w * vs[1];
    V[2] = w * vs[2];
    const double sigma = __builtin_sqrt((V[0] + V[1] + V[2]) / 3.0);
    const double mu = ((double)pix.x + (double)pix.y + (double)pix.z) / 3.0;
    return (float)(sigma / (mu > floor ? mu : floor));
}

// The four statistics of ptg_noise_device, reduced per wave and per workgroup
// (LDS), then one vector atomic per workgroup and value; every thread of the
// workgroup calls it.
__device__ __forceinline__ void reduce_noise_stats(unsigned over, unsigned cnt, unsigned long long fixed,
                                                   unsigned rho_bits, unsigned long long *stats)
{
    for (int off = 32; off > 0; off >>= 1) {  // every lane of the wave takes part
        over += __shfl_xor(over, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
        fixed += __shfl_xor(fixed, off, 64);
        const unsigned other = __shfl_xor(rho_bits, off, 64);
        rho_bits = rho_bits > other ? rho_bits : other;
    }
    __shared__ unsigned long long red[4][4];
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *r = red[threadIdx.x >> 6];
        r[0] = over;
        r[1] = fixed;
        r[2] = rho_bits;
        r[3] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[4] = {0ull, 0ull, 0ull, 0ull};
        for (int wv = 0; wv < 4; ++wv) {
            t[0] += red[wv][0];
            t[1] += red[wv][1];
            t[2] = t[2] > red[wv][2] ? t[2] : red[wv][2];
            t[3] += red[wv][3];
        }
        if (t[3]) {
            atomicAdd(stats + 0, t[0]);
            atomicAdd(stats + 1, t[1]);
            atomicMax(stats + 2, t[2]);
            atomicAdd(stats + 3, t[3]);
        }
    }
}

// ptg_noise_device (include/ptgpu.h "per-pixel noise estimates"): one thread
// per slab pixel (grid-stride), from the exact sums A.acc (S1) and acc2 (S2)
// after A.samps samples: the pixel value p as resolve_kernel computes it, per
// channel the variance V of that value (every sub-pixel's variance of the
// mean capped at 1/4: the image clamps the mean to [0, 1]) and the relative
// standard error rho = sqrt(mean V) / max(mean p, floor); var / rho / stats
// are optional.  stats: four integers, reduced per thread, per wave and per
// workgroup (LDS), then one vector atomic per workgroup and value -- the
// result does not depend on any order, and the grid is small enough
// (ptg_noise_device: at most kNoiseBlocks workgroups) that the atomics on the
// one cache line do not set the time (one per wave of a 1920x1080 frame:
// 1.58 ms, against 0.22 ms without the stats).
constexpr int kNoiseBlocks = 2048;  // 8 workgroups of 256 per CU on 256 CUs
__global__ __launch_bounds__(256) void noise_kernel(KArgs A, const unsigned long long *__restrict__ acc2,
                                                    double rel_error, double floor, float *__restrict__ var,
                                                    float *__restrict__ rho_out, unsigned long long *stats)
{
    const long long total = (long long)A.slab_rows * A.W;
    const long long stride = (long long)gridDim.x * 256;
    unsigned over = 0u, cnt = 0u, rho_bits = 0u;
    unsigned long long fixed = 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        if (out_row_of(A, (int)(i / A.W)) >= A.H)
            continue;  // a slab row past the image
        const unsigned long long *g1 = A.acc + (size_t)i * A.lanes_per_pixel * 3;
        const unsigned long long *g2 = acc2 + (size_t)i * A.lanes_per_pixel * 3;
        double V[3];
        const float rho = noise_pixel(A, g1, g2, (double)A.samps, floor, V);
        if (var) {
            var[(size_t)i * 3 + 0] = (float)V[0];
            var[(size_t)i * 3 + 1] = (float)V[1];
            var[(size_t)i * 3 + 2] = (float)V[2];
        }
        if (rho_out)
            rho_out[i] = rho;
        over += (double)rho > rel_error ? 1u : 0u;
        fixed += (unsigned long long)((rho < 4096.0f ? rho : 4096.0f) * 0x1p20f);
        const unsigned bits = __float_as_uint(rho);  // rho >= 0: the bit patterns order like the values
        rho_bits = rho_bits > bits ? rho_bits : bits;
        cnt += 1u;
    }
    if (!stats)
        return;  // the whole grid
    reduce_noise_stats(over, cnt, fixed, rho_bits, stats);
}

// ---- adaptive sampling: the active list (include/ptgpu.h "adaptive sampling") ----
// ptg_select_active_device, step 1: noise_kernel with each pixel's own sample
// count n_p (n_p < 2: rho = +inf) -- per slab pixel a byte "over the target"
// (0 in rows past the image, so step 2 may read any row), optionally rho, and
// the four statistics.
__global__ __launch_bounds__(256) void select_over_kernel(KArgs A, const unsigned long long *__restrict__ acc2,
                                                          const int *__restrict__ counts, double rel_error,
                                                          double floor, uint8_t *__restrict__ over_out,
                                                          float *__restrict__ rho_out, unsigned long long *stats)
{
    const long long total = (long long)A.slab_rows * A.W;
    const long long stride = (long long)gridDim.x * 256;
    unsigned over = 0u, cnt = 0u, rho_bits = 0u;
    unsigned long long fixed = 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        if (out_row_of(A, (int)(i / A.W)) >= A.H) {
            over_out[i] = 0;
            continue;  // a slab row past the image
        }
        const int np = counts[i];
        float rho = __builtin_inff();
        if (np >= 2) {
            double V[3];
            rho = noise_pixel(A, A.acc + (size_t)i * A.lanes_per_pixel * 3, acc2 + (size_t)i * A.lanes_per_pixel * 3,
                              (double)np, floor, V);
        }
        if (rho_out)
            rho_out[i] = rho;
        const unsigned is_over = (double)rho > rel_error ? 1u : 0u;
        over_out[i] = (uint8_t)is_over;
        over += is_over;
        fixed += (unsigned long long)((rho < 4096.0f ? rho : 4096.0f) * 0x1p20f);
        const unsigned bits = __float_as_uint(rho);
        rho_bits = rho_bits > bits ? rho_bits : bits;
        cnt += 1u;
    }
    if (!stats)
        return;  // the whole grid
    reduce_noise_stats(over, cnt, fixed, rho_bits, stats);
}

// ptg_noise_active_device: noise_kernel's variance slab and rho with each
// pixel's own sample count n_p, the filter's guide for an adaptive frame (one
// thread per slab pixel, grid-stride; var and rho_out each optional).
// n_p < 2 knows nothing beyond the clamp's bound: rho = +inf as in
// select_over_kernel, and per channel the V noise_pixel yields when every
// sub-pixel's variance sits at the 1/4 cap.  No statistics: the select step
// supplies them.
__global__ __launch_bounds__(256) void noise_active_kernel(KArgs A, const unsigned long long *__restrict__ acc2,
                                                           const int *__restrict__ counts, double floor,
                                                           float *__restrict__ var, float *__restrict__ rho_out)
{
    const long long total = (long long)A.slab_rows * A.W;
    const long long stride = (long long)gridDim.x * 256;
    const float v_cap = (float)(((double)A.inv_sub2 * (double)A.inv_sub2) * ((double)A.lanes_per_pixel * 0.25));
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        if (out_row_of(A, (int)(i / A.W)) >= A.H)
            continue;  // a slab row past the image
        const int np = counts[i];
        float rho = __builtin_inff();
        float v[3] = {v_cap, v_cap, v_cap};
        if (np >= 2) {
            double V[3];
            rho = noise_pixel(A, A.acc + (size_t)i * A.lanes_per_pixel * 3, acc2 + (size_t)i * A.lanes_per_pixel * 3,
                              (double)np, floor, V);
            v[0] = (float)V[0];
            v[1] = (float)V[1];
            v[2] = (float)V[2];
        }
        if (var) {
            var[(size_t)i * 3 + 0] = v[0];
            var[(size_t)i * 3 + 1] = v[1];
            var[(size_t)i * 3 + 2] = v[2];
        }
        if (rho_out)
            rho_out[i] = rho;
    }
}

// List building, step 1: one workgroup per slab row writes the row's active x
// in ascending order to list[row * W ...] and their number to row_count[row].
// Active: flags == NULL, or some flag byte of the pixel's (2 dilate + 1)^2
// window, clipped to the image, is set (dilate > 0 only with shard_count 1,
// where slab row j is image row j).  Ranks: ballot / mbcnt within a wave, the
// waves' counts through LDS -- the order does not depend on any timing.
__global__ __launch_bounds__(256) void list_rows_kernel(KArgs A, const uint8_t *__restrict__ flags, int dilate,
                                                        int *__restrict__ list, int *__restrict__ row_count)
{
    const int row = blockIdx.x;
    const bool valid_row = out_row_of(A, row) < A.H;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ int wave_cnt[4];
    int base = 0;  // the row's active pixels left of this tile (workgroup-uniform)
    for (int x0 = 0; x0 < A.W; x0 += 256) {
        const int x = x0 + (int)threadIdx.x;
        bool act = false;
        if (valid_row && x < A.W) {
            if (!flags) {
                act = true;
            } else if (dilate == 0) {
                act = flags[(size_t)row * A.W + x] != 0;
            } else {
                const int r0 = row - dilate > 0 ? row - dilate : 0;
                const int r1 = row + dilate < A.H - 1 ? row + dilate : A.H - 1;
                const int c0 = x - dilate > 0 ? x - dilate : 0;
                const int c1 = x + dilate < A.W - 1 ? x + dilate : A.W - 1;
                for (int rr = r0; rr <= r1; ++rr)
                    for (int cc = c0; cc <= c1; ++cc)
                        act |= flags[(size_t)rr * A.W + cc] != 0;
            }
        }
        const unsigned long long m = __ballot(act);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0)
            wave_cnt[wv] = (int)__popcll(m);
        __syncthreads();
        int before = 0, tile = 0;
        for (int w = 0; w < 4; ++w) {
            const int c = wave_cnt[w];
            before += w < wv ? c : 0;
            tile += c;
        }
        if (act)
            list[(size_t)row * A.W + base + before + rank] = x;  // base + before + rank < the row's count <= W
        base += tile;
        __syncthreads();  // wave_cnt is rewritten by the next tile
    }
    if (threadIdx.x == 0)
        row_count[row] = base;
}

// Step 1 for a shard of a multi-device frame (ptg_set_active_gathered_device):
// list_rows_kernel's output from the over bytes of the WHOLE frame, gathered
// rank-major (shard_count slabs of slab_rows * W bytes, ptg_unshard_device's
// layout) -- with interleaved bands the window rows of a pixel live in other
// shards' slabs.  Separable, per tile of 256 columns:
//   1. the row's <= 17 window rows (clipped to the image) are mapped to
//      gathered slab rows once, in LDS (workgroup-uniform);
//   2. each lane ORs its column over those rows (coalesced byte loads); the
//      wave's ballot is a 64-bit word in LDS -- 4 words a tile, and a fifth
//      from the first `dilate` columns right of it (the seam: x = 255 needs
//      columns up to 263); the word left of the tile is carried in a register;
//   3. every wave dilates the 4 words horizontally, each OR-ed with its two
//      neighbours shifted by -dilate..+dilate (dilate <= 8 < 64) -- scalar
//      work; its own word gives the lanes' flags, the popcounts of all four
//      the ranks (no second pass through LDS).
// Columns >= W and rows outside the image contribute no set bit, so the window
// is clipped; slab rows past the image are never read.
constexpr int kMaxDilate = 8;

__device__ __forceinline__ unsigned long long dilate_word(unsigned long long l, unsigned long long c,
                                                          unsigned long long r, int dilate)
{
    unsigned long long d = c;
    for (int k = 1; k <= dilate; ++k)  // column b -+ k set: pixel b is active
        d |= (c << k) | (l >> (64 - k)) | (c >> k) | (r << (64 - k));
    return d;
}

__global__ __launch_bounds__(256) void list_rows_gathered_kernel(KArgs A, const uint8_t *__restrict__ gathered,
                                                                 int dilate, int *__restrict__ list,
                                                                 int *__restrict__ row_count)
{
    const int row = blockIdx.x;
    const int r = out_row_of(A, row);
    if (r >= A.H) {  // a slab row past the image (the whole workgroup)
        if (threadIdx.x == 0)
            row_count[row] = 0;
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ long long win_row[2 * kMaxDilate + 1];  // gathered slab row (rank-major) of each window row
    __shared__ unsigned long long word[5];             // column-OR ballots: the tile's four, the right seam's
    const int r0 = r - dilate > 0 ? r - dilate : 0;
    const int r1 = r + dilate < A.H - 1 ? r + dilate : A.H - 1;
    const int n_win = r1 - r0 + 1;
    if ((int)threadIdx.x < n_win) {
        const int rr = r0 + (int)threadIdx.x;
        const int band = rr / A.band_rows;
        const int rank = band % A.shard_count;
        win_row[threadIdx.x] = (long long)rank * A.slab_rows + (long long)(band / A.shard_count) * A.band_rows +
                               (rr - band * A.band_rows);
    }
    __syncthreads();
    auto column_or = [&](int x, bool on) -> unsigned long long {
        unsigned v = 0u;
        if (on && x < A.W)
            for (int j = 0; j < n_win; ++j)
                v |= gathered[(size_t)win_row[j] * A.W + x];
        return __ballot(v != 0u);
    };
    unsigned long long left = 0ull;  // the word of the 64 columns left of the tile (workgroup-uniform)
    int base = 0;                    // the row's active pixels left of this tile (workgroup-uniform)
    for (int x0 = 0; x0 < A.W; x0 += 256) {
        const int x = x0 + (int)threadIdx.x;
        const unsigned long long own = column_or(x, true);
        if (lane == 0)
            word[wv] = own;
        if (wv == 0) {  // the seam: the first `dilate` columns of the next tile
            const unsigned long long seam = column_or(x + 256, lane < dilate);
            if (lane == 0)
                word[4] = seam;
        }
        __syncthreads();
        unsigned long long w[6];
        w[0] = left;
        for (int i = 0; i < 5; ++i)
            w[i + 1] = word[i];
        int before = 0, tile = 0;
        unsigned long long mine = 0ull;
        for (int i = 0; i < 4; ++i) {
            const int nv = A.W - (x0 + 64 * i);  // the word's columns inside the image
            const unsigned long long valid = nv >= 64 ? ~0ull : (nv > 0 ? (1ull << nv) - 1ull : 0ull);
            const unsigned long long d = dilate_word(w[i], w[i + 1], w[i + 2], dilate) & valid;
            const int c = (int)__popcll(d);
            before += i < wv ? c : 0;
            tile += c;
            mine = i == wv ? d : mine;
        }
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mine >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((unsigned)mine, 0u));
        if ((mine >> lane) & 1ull)
            list[(size_t)row * A.W + base + before + rank] = x;  // base + before + rank < the row's count <= W
        base += tile;
        left = w[4];
        __syncthreads();  // word is rewritten by the next tile
    }
    if (threadIdx.x == 0)
        row_count[row] = base;
}

// Step 2, one workgroup: a row's pixels are cut into units of pixels_per_wave
// (units never span rows); row_unit0[row] = the units of the rows before it
// (an exclusive scan: shuffles within a wave, LDS across the workgroup, a
// carry across tiles of 256 rows).  Writes the device record {active pixels,
// active units}, the same two values to info (optional), and adds them to
// stats[4], stats[5] (optional).
__global__ __launch_bounds__(256) void list_units_kernel(int slab_rows, int ppw, const int *__restrict__ row_count,
                                                         int *__restrict__ row_unit0, unsigned long long *rec,
                                                         unsigned long long *info, unsigned long long *stats)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ int wave_sum[4];
    __shared__ unsigned long long wave_pix[4];
    unsigned long long pixels = 0ull;
    int carry = 0;
    for (int r0 = 0; r0 < slab_rows; r0 += 256) {
        const int r = r0 + (int)threadIdx.x;
        const int cnt = r < slab_rows ? row_count[r] : 0;
        const int nu = (cnt + ppw - 1) / ppw;
        pixels += (unsigned long long)cnt;
        int incl = nu;
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            incl += lane >= off ? v : 0;
        }
        if (lane == 63)
            wave_sum[wv] = incl;
        __syncthreads();
        int before = 0, tile = 0;
        for (int w = 0; w < 4; ++w) {
            const int c = wave_sum[w];
            before += w < wv ? c : 0;
            tile += c;
        }
        if (r < slab_rows)
            row_unit0[r] = carry + before + incl - nu;
        carry += tile;
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1)
        pixels += __shfl_xor(pixels, off, 64);
    if (lane == 0)
        wave_pix[wv] = pixels;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long np = wave_pix[0] + wave_pix[1] + wave_pix[2] + wave_pix[3];
        rec[0] = np;
        rec[1] = (unsigned long long)carry;
        if (info) {
            info[0] = np;
            info[1] = (unsigned long long)carry;
        }
        if (stats) {
            atomicAdd(stats + 4, np);
            atomicAdd(stats + 5, (unsigned long long)carry);
        }
    }
}

// Step 3, one workgroup per slab row: the row's entries of the unit table,
// {slab row, first index in the row's list, pixels}.  The entries written are
// [0, rec[1]), at most n_groups (the table's size).
__global__ __launch_bounds__(256) void list_fill_kernel(int ppw, const int *__restrict__ row_count,
                                                        const int *__restrict__ row_unit0, int4 *__restrict__ units)
{
    const int row = blockIdx.x;
    const int cnt = row_count[row], u0 = row_unit0[row];
    for (int k = threadIdx.x; k * ppw < cnt; k += 256)
        units[u0 + k] = make_int4(row, k * ppw, cnt - k * ppw < ppw ? cnt - k * ppw : ppw, 0);
}

// After gather_kernel (not inside it: other chunks of the same pixel read
// n_p at unit setup): one wave per unit (grid-stride) adds add_samples to the
// counts of the unit's pixels, the same units [0, min(rec[1], max_units)).
__global__ __launch_bounds__(256) void bump_counts_kernel(int W, const int4 *__restrict__ units,
                                                          const int *__restrict__ list,
                                                          const unsigned long long *__restrict__ rec,
                                                          long long max_units, int add, int *__restrict__ counts)
{
    long long n = (long long)rec[1];
    n = n < max_units ? n : max_units;
    const int lane = threadIdx.x & 63;
    for (long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); u < n; u += (long long)gridDim.x * 4) {
        const int4 e = units[u];
        if (lane < e.z) {
            const size_t rowbase = (size_t)e.x * W;
            counts[rowbase + list[rowbase + e.y + lane]] += add;
        }
    }
}
