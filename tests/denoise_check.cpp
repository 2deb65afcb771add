// denoise_check -- the a-trous filter's host loop (csrc/denoise_filter.hpp) on
// seeded frames, built with AddressSanitizer + UBSan by
// tests/test_denoise_host.py.  For every size: the output is finite, sum w > 0
// at every pixel of every iteration, iterations = 0 copies the input, and an
// in-place tap can never read outside the frame (the sanitizers' part).
// Writes inputs and outputs as raw float32 files into argv[1] for the Python
// side, which restates the definition in numpy.
//
//   denoise_check OUT_DIR [ITERATIONS ...]      (default: 5 iterations)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../cpu-path-tracing_amd/csrc/denoise_filter.hpp"

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    float u() { return (float)(next() >> 40) * 0x1p-24f; }
};

struct Frame {
    int W, H;
    std::vector<float> color, var, feat;
};

// A frame of a few regions (vertical bands and a sky strip at the top), each
// with its own plane, albedo and base colour; noisy colour whose variance the
// variance frame states; silhouette columns with fractional hit.
Frame make_frame(int W, int H, uint64_t seed)
{
    Frame f{W, H, {}, {}, {}};
    const size_t px = (size_t)W * H;
    f.color.resize(px * 3);
    f.var.resize(px * 3);
    f.feat.assign(px * ptg_dn::kFeat, 0.0f);
    Rng r{seed};
    const int bands = 3;
    float nrm[bands][3], alb[bands][3], base[bands][3], depth[bands];
    for (int b = 0; b < bands; ++b) {
        float len = 0.0f;
        for (int c = 0; c < 3; ++c) {
            nrm[b][c] = r.u() - 0.5f;
            len += nrm[b][c] * nrm[b][c];
            alb[b][c] = 0.25f + 0.5f * (float)(r.next() & 1);
            base[b][c] = r.u();
        }
        len = std::sqrt(len) + 1e-3f;
        for (int c = 0; c < 3; ++c)
            nrm[b][c] /= len;
        depth[b] = 2.0f + 6.0f * r.u();
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const int b = (x * bands) / W;
            const bool sky = y * 6 < H;
            const bool edge = !sky && x > 0 && ((x - 1) * bands) / W != b;  // first column of a band
            const float sd = 0.02f + 0.1f * r.u();
            for (int c = 0; c < 3; ++c) {
                f.color[i * 3 + c] = (sky ? 0.6f : base[b][c]) + sd * (r.u() - 0.5f);
                f.var[i * 3 + c] = sd * sd * (1.0f / 12.0f) * (0.5f + r.u());
            }
            float *g = &f.feat[i * ptg_dn::kFeat];
            if (sky) {
                g[8] = g[9] = g[10] = 1.0f;
                continue;
            }
            const float hit = edge ? 0.25f * (float)(1 + (r.next() % 3)) : 1.0f;
            const float z = depth[b] + 0.01f * (float)x + 0.02f * (float)y;
            for (int c = 0; c < 3; ++c) {
                g[c] = nrm[b][c] * (edge ? 0.9f : 1.0f);
                g[8 + c] = alb[b][c];
            }
            g[3] = z;
            g[4] = 0.01f * (float)x * z;
            g[5] = 0.01f * (float)y * z;
            g[6] = -z;
            g[7] = hit;
        }
    return f;
}

int g_bad = 0;
void expect(bool ok, const std::string &what)
{
    if (!ok) {
        std::printf("FAIL %s\n", what.c_str());
        ++g_bad;
    }
}

void dump(const std::string &path, const std::vector<float> &v)
{
    FILE *fp = std::fopen(path.c_str(), "wb");
    if (!fp || std::fwrite(v.data(), sizeof(float), v.size(), fp) != v.size()) {
        std::printf("FAIL cannot write %s\n", path.c_str());
        ++g_bad;
    }
    if (fp)
        std::fclose(fp);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::printf("usage: denoise_check OUT_DIR [ITERATIONS ...]\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::vector<int> iters;
    for (int a = 2; a < argc; ++a)
        iters.push_back(std::atoi(argv[a]));
    if (iters.empty())
        iters.push_back(5);
    const int sizes[][2] = {{1, 1}, {8, 5}, {70, 37}, {150, 70}, {257, 66}};
    for (const auto &wh : sizes) {
        const int W = wh[0], H = wh[1];
        const Frame f = make_frame(W, H, 0x5EED0000ull + (uint64_t)W * 1000 + H);
        const std::string tag = dir + "/" + std::to_string(W) + "x" + std::to_string(H);
        dump(tag + "_color.f32", f.color);
        dump(tag + "_var.f32", f.var);
        dump(tag + "_feat.f32", f.feat);
        ptg_denoise_params k;
        ptg_dn::defaults(&k);
        k.pixel_spread = 0.01f;
        expect(ptg_dn::params_error(&k) == nullptr, tag + " defaults are valid");
        std::vector<float> work(ptg_dn::scratch_of(W, H).total);
        std::vector<float> out(f.color.size()), vout(f.color.size());
        // iterations = 0: a copy
        k.iterations = 0;
        ptg_dn::filter_host(f.color.data(), f.var.data(), f.feat.data(), W, H, k, out.data(), vout.data(),
                            work.data(), nullptr);
        expect(out == f.color && vout == f.var, tag + " iterations 0 copies the input");
        for (int n : iters) {
            k.iterations = n;
            float least = 0.0f;
            ptg_dn::filter_host(f.color.data(), f.var.data(), f.feat.data(), W, H, k, out.data(), vout.data(),
                                work.data(), &least);
            bool finite = true, nonneg = true;
            for (size_t i = 0; i < out.size(); ++i) {
                finite = finite && std::isfinite(out[i]) && std::isfinite(vout[i]);
                nonneg = nonneg && vout[i] >= 0.0f;
            }
            expect(finite, tag + " finite output at " + std::to_string(n) + " iterations");
            expect(nonneg, tag + " variance >= 0");
            // the centre tap alone weighs 9/64
            expect(least >= 0.140625f, tag + " sum w >= 9/64 everywhere (least " + std::to_string(least) + ")");
            // without the optional variance output: the same colour
            std::vector<float> out2(out.size());
            ptg_dn::filter_host(f.color.data(), f.var.data(), f.feat.data(), W, H, k, out2.data(), nullptr,
                                work.data(), nullptr);
            expect(out2 == out, tag + " colour does not depend on var_out");
            dump(tag + "_out" + std::to_string(n) + ".f32", out);
            dump(tag + "_vout" + std::to_string(n) + ".f32", vout);
            std::printf("%dx%d iterations %d: least sum w %.6f\n", W, H, n, least);
        }
    }
    std::printf(g_bad ? "%d checks FAILED\n" : "all checks passed\n", g_bad);
    return g_bad ? 1 : 0;
}
