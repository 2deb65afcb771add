// Host-side check of the launch plan (cpu-path-tracing_amd/csrc/launch_plan.hpp)
// and of the scene fields the kernels are given (csrc/scene_prep.hpp), built
// and run on the CPU by tests/test_launch_plan.py with AddressSanitizer/UBSan.
// For every row of a table of frames, shards and progressive passes it fills
// the plan and verifies what render_kernel relies on when it maps a unit to
// its level, pixel group and samples (render_unit.hpp: "unit -> level"):
//   * lvl_group and lvl_unit are non-decreasing, lvl_group[0] = 0,
//     lvl_group[n_levels] = n_groups, lvl_unit[n_levels] = n_units;
//   * every lvl_chunk is in [1, kMaxChunk] (divmod_nv's exact range);
//   * a cooperative level starts on a workgroup boundary and has exactly one
//     chunk per wave of the workgroup;
//   * lvl_psplit <= pixels_per_wave;
//   * needs_resolve holds exactly when some level is not resolved in the
//     wave, and then resolve_row0 is that level's first slab row;
//   * the grid is ceil(n_units / waves per workgroup);
//   * decoded as the kernel decodes them, the units cover the samples
//     [sample_begin, sample_end) of every pixel group (and pixel part)
//     exactly once;
//   * the pixels of every unit, formed as render_unit forms them (x0, npix,
//     left), fit the wave's 64 lanes, lie inside the row and inside their
//     group's span, and every pixel of every slab row receives exactly
//     sample_end - sample_begin samples.
// Then it prints the plan and, for the three built-in scenes, the scene
// fields of KArgs with a hash of the linear upload table; --dump prints both
// as JSON, which the test compares with tests/golden/launch_plans.json.
// Exits non-zero on the first violation.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../cpu-path-tracing_amd/csrc/kernel_args.hpp"
#include "../cpu-path-tracing_amd/csrc/launch_plan.hpp"
#include "../cpu-path-tracing_amd/csrc/scene_prep.hpp"
#include "../cpu-path-tracing_amd/host/pt/gpu_render.hpp"
#include "../cpu-path-tracing_amd/host/pt/scenes.hpp"

static int fails = 0;
#define CHECK(c, ...)                                                                              \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            std::fprintf(stderr, "%s: ", name);                                                    \
            std::fprintf(stderr, __VA_ARGS__);                                                     \
            std::fprintf(stderr, "\n");                                                            \
            ++fails;                                                                               \
            return;                                                                                \
        }                                                                                          \
    } while (0)

struct Row {
    const char *name;
    int n, wave_slots;
    int W, H, samples, nsub;
    int band_rows, shard_rank, shard_count, chunk_samples, flags;
    int s_begin, s_end;  // s_end < 0: every sample
    bool accumulate_only;
    int box_walls_out;
    int expect_rc;
};

// what the kernels index without checks
static void check_plan(const char *name, const KArgs &A, int grid, bool bvh)
{
    const int L = A.n_levels;
    CHECK(L >= 1 && L <= kMaxLevels, "n_levels %d", L);
    CHECK(A.lvl_group[0] == 0 && A.lvl_group[L] == A.n_groups, "lvl_group ends %d %d (n_groups %d)", A.lvl_group[0],
          A.lvl_group[L], A.n_groups);
    CHECK(A.n_groups == A.slab_rows * A.waves_per_row, "n_groups %d", A.n_groups);
    CHECK(A.lvl_unit[0] == 0 && A.lvl_unit[L] == A.n_units, "lvl_unit ends %lld %lld (n_units %lld)", A.lvl_unit[0],
          A.lvl_unit[L], A.n_units);
    const int waves = (bvh ? PTG_BVH_BLOCK : kBlock) / 64;
    const int nsamp = A.sample_end - A.sample_begin;
    bool accumulates = false;
    int first_acc_row = -1;
    for (int l = 0; l < L; ++l) {
        CHECK(A.lvl_group[l] <= A.lvl_group[l + 1], "lvl_group decreases at level %d", l);
        CHECK(A.lvl_unit[l] <= A.lvl_unit[l + 1], "lvl_unit decreases at level %d", l);
        CHECK(A.lvl_chunk[l] >= 1 && A.lvl_chunk[l] <= kMaxChunk, "level %d chunk %d", l, A.lvl_chunk[l]);
        CHECK(A.lvl_psplit[l] >= 1 && A.lvl_psplit[l] <= A.pixels_per_wave, "level %d psplit %d", l, A.lvl_psplit[l]);
        CHECK(A.lvl_group[l] % A.waves_per_row == 0, "level %d starts inside a row", l);
        if (A.lvl_coop[l]) {
            CHECK(!bvh && A.lvl_unit[l] % waves == 0, "cooperative level %d starts at unit %lld", l, A.lvl_unit[l]);
            CHECK((nsamp + A.lvl_chunk[l] - 1) / A.lvl_chunk[l] == waves, "cooperative level %d: chunk %d of %d samples",
                  l, A.lvl_chunk[l], nsamp);
            CHECK(A.lvl_psplit[l] == 1 && !A.lvl_inwave[l], "cooperative level %d flags", l);
        }
        if (A.lvl_inwave[l])  // one unit holds every sample of its pixels
            CHECK(A.lvl_chunk[l] >= nsamp && A.sample_begin == 0 && A.sample_end == A.samps, "in-wave level %d", l);
        // (a cooperative level resolves from LDS, an in-wave level in the wave)
        if (!A.lvl_inwave[l] && !A.lvl_coop[l] && A.lvl_group[l] < A.lvl_group[l + 1] && !accumulates) {
            accumulates = true;
            first_acc_row = A.lvl_group[l] / A.waves_per_row;
        }
    }
    bool all_inwave = true;
    for (int l = 0; l < L; ++l)
        all_inwave = all_inwave && (A.lvl_inwave[l] || A.lvl_coop[l] || A.lvl_group[l] == A.lvl_group[l + 1]);
    CHECK((A.needs_resolve != 0) == !all_inwave, "needs_resolve %d", A.needs_resolve);
    if (A.needs_resolve)
        CHECK(A.resolve_row0 == first_acc_row, "resolve_row0 %d, first accumulating row %d", A.resolve_row0,
              first_acc_row);
    else
        CHECK(A.resolve_row0 == 0, "resolve_row0 %d without a resolve", A.resolve_row0);
    CHECK((long long)grid == (A.n_units + waves - 1) / waves, "grid %d for %lld units", grid, A.n_units);
    // the kernel's decode of every unit: each (pixel group, part) must receive
    // the sample chunks s_begin, s_begin + len, ... in order, up to s_end
    std::vector<int> next((size_t)A.n_groups * A.pixels_per_wave, A.sample_begin);
    std::vector<char> parts((size_t)A.n_groups, 0);
    // ... and the pixels the unit covers, formed as render_unit forms them
    // (slab_row, xblk, x0, npix, left): samples received per slab pixel
    std::vector<int> got((size_t)A.slab_rows * A.W, 0);
    for (long long unit = 0; unit < (long long)grid * waves; ++unit) {
        if (unit >= A.n_units)
            continue;
        int lv = 0;
        while (lv + 1 < L && unit >= A.lvl_unit[lv + 1])
            ++lv;
        const long long t = unit - A.lvl_unit[lv];
        const int nlg = A.lvl_group[lv + 1] - A.lvl_group[lv];
        const bool coop = A.lvl_coop[lv] != 0;
        const int ps = A.lvl_psplit[lv];
        const long long nlu = (long long)nlg * ps;
        CHECK(nlu > 0, "unit %lld falls into the empty level %d", unit, lv);
        const long long tg = coop ? t / waves : t % nlu;
        const int group = A.lvl_group[lv] + (int)(coop ? tg : tg % nlg);
        const int part = coop ? 0 : (int)(tg / nlg);
        const int len = A.lvl_chunk[lv];
        const long long s0 = A.sample_begin + (coop ? t % waves : t / nlu) * len;
        if (s0 >= A.sample_end)
            continue;  // alignment padding before a cooperative level
        CHECK(group >= A.lvl_group[lv] && group < A.lvl_group[lv + 1], "unit %lld: group %d outside level %d", unit,
              group, lv);
        CHECK(part < ps, "unit %lld: part %d of %d", unit, part, ps);
        int &nx = next[(size_t)group * A.pixels_per_wave + part];
        CHECK(nx == s0, "unit %lld: group %d part %d gets samples from %lld, expected %d", unit, group, part, s0, nx);
        const int cnt = A.sample_end - (int)s0 < len ? A.sample_end - (int)s0 : len;
        nx += cnt;
        parts[group] = (char)ps;
        const int slab_row = group / A.waves_per_row;
        const int xblk = group - slab_row * A.waves_per_row;
        const int x0 = xblk * A.pixels_per_wave + part;
        int npix = (A.pixels_per_wave - part + ps - 1) / ps;
        const int left = A.W - x0 > 0 ? (A.W - x0 + ps - 1) / ps : 0;
        npix = npix < left ? npix : left;
        CHECK(slab_row >= 0 && slab_row < A.slab_rows, "unit %lld: slab row %d", unit, slab_row);
        CHECK(npix >= 0 && npix * A.lanes_per_pixel <= 64, "unit %lld: %d pixels of %d lanes", unit, npix,
              A.lanes_per_pixel);
        for (int k = 0; k < npix; ++k) {
            const int px = x0 + k * ps;
            CHECK(px < A.W, "unit %lld: pixel %d outside the row", unit, px);
            CHECK(px >= xblk * A.pixels_per_wave && px < (xblk + 1) * A.pixels_per_wave,
                  "unit %lld: pixel %d outside group %d's span", unit, px, group);
            got[(size_t)slab_row * A.W + px] += cnt;
        }
    }
    for (size_t i = 0; i < got.size(); ++i)
        CHECK(got[i] == nsamp, "slab row %zu pixel %zu received %d of %d samples", i / A.W, i % A.W, got[i], nsamp);
    for (int g = 0; g < A.n_groups && nsamp > 0; ++g) {
        CHECK(parts[g] >= 1, "group %d has no unit", g);
        for (int k = 0; k < parts[g]; ++k)
            CHECK(next[(size_t)g * A.pixels_per_wave + k] == A.sample_end, "group %d part %d: samples end at %d", g, k,
                  next[(size_t)g * A.pixels_per_wave + k]);
    }
}

template <typename T>
static std::string list(const T *v, int n)
{
    std::string s = "[";
    for (int i = 0; i < n; ++i)
        s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

static void run_row(const Row &r, bool dump, bool last)
{
    const char *name = r.name;
    KArgs base;
    std::memset(&base, 0, sizeof(base));
    base.n = r.n;
    base.box_mode = r.n <= kLinearMax ? 1 : 0;
    base.box_walls_out = r.box_walls_out;
    ptg_params p{};
    p.width = r.W;
    p.height = r.H;
    p.samples = r.samples;
    p.num_subpixels = r.nsub;
    p.seed = 1;
    p.band_rows = r.band_rows;
    p.shard_rank = r.shard_rank;
    p.shard_count = r.shard_count;
    p.chunk_samples = r.chunk_samples;
    p.flags = r.flags;
    KArgs A;
    int grid = -1;
    int rc = check_params(&p);
    if (rc == PTG_OK)
        rc = fill_launch(base, r.wave_slots, &p, A, grid, r.s_begin, r.s_end, r.accumulate_only);
    CHECK(rc == r.expect_rc, "status %d, expected %d (%s)", rc, r.expect_rc, g_last_error.c_str());
    if (rc != PTG_OK) {
        CHECK(grid == 0, "grid %d after a failure", grid);
        if (dump)
            std::printf("  {\"name\": \"%s\", \"rc\": %d, \"error\": \"%s\"}%s\n", name, rc, g_last_error.c_str(),
                        last ? "" : ",");
        else
            std::printf("%s: rc=%d %s\n", name, rc, g_last_error.c_str());
        return;
    }
    const bool bvh = r.n > kLinearMax;
    check_plan(name, A, grid, bvh);
    if (fails)
        return;
    const int L = A.n_levels;
    if (dump) {
        std::printf("  {\"name\": \"%s\", \"rc\": 0, \"grid\": %d, \"n_units\": %lld, \"n_levels\": %d, \"chunk\": %d, "
                    "\"n_groups\": %d, \"single_chunk\": %d, \"needs_resolve\": %d, \"resolve_row0\": %d, "
                    "\"box_mode\": %d, \"slab_rows\": %d, \"waves_per_row\": %d, \"pixels_per_wave\": %d, "
                    "\"sample_begin\": %d, \"sample_end\": %d, \"lvl_group\": %s, \"lvl_unit\": %s, \"lvl_chunk\": %s, "
                    "\"lvl_coop\": %s, \"lvl_psplit\": %s, \"lvl_inwave\": %s}%s\n",
                    name, grid, A.n_units, L, A.chunk, A.n_groups, A.single_chunk, A.needs_resolve, A.resolve_row0,
                    A.box_mode, A.slab_rows, A.waves_per_row, A.pixels_per_wave, A.sample_begin, A.sample_end,
                    list(A.lvl_group, L + 1).c_str(), list(A.lvl_unit, L + 1).c_str(), list(A.lvl_chunk, L).c_str(),
                    list(A.lvl_coop, L).c_str(), list(A.lvl_psplit, L).c_str(), list(A.lvl_inwave, L).c_str(),
                    last ? "" : ",");
        return;
    }
    std::printf("%s: grid=%d units=%lld levels=%d resolve_row0=%d box_mode=%d\n", name, grid, A.n_units, L,
                A.needs_resolve ? A.resolve_row0 : -1, A.box_mode);
    for (int l = 0; l < L; ++l)
        std::printf("    L%d groups [%d, %d) units from %lld chunk=%d%s psplit=%d%s\n", l, A.lvl_group[l],
                    A.lvl_group[l + 1], A.lvl_unit[l], A.lvl_chunk[l], A.lvl_coop[l] ? " coop" : "", A.lvl_psplit[l],
                    A.lvl_inwave[l] ? " in-wave" : "");
}

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static std::string hex3(const float *v)
{
    char buf[64];
    std::snprintf(buf, sizeof buf, "[\"%08x\", \"%08x\", \"%08x\"]", bits(v[0]), bits(v[1]), bits(v[2]));
    return buf;
}

// scene fields of KArgs as ptg_context_create fills them, floats as bit patterns
static void run_scene(const char *name, const pt::scene &scn, bool dump, bool last)
{
    const pt::camera cam = pt::camera::with_config(scn.camera_parameters);
    const ptg_sphere *s = reinterpret_cast<const ptg_sphere *>(scn.spheres.data());
    const ptg_camera *c = reinterpret_cast<const ptg_camera *>(&cam);
    const int n = (int)scn.spheres.size();
    for (int i = 0; i < n; ++i)
        CHECK(sphere_ok(s[i]), "sphere %d", i);
    KArgs A;
    std::memset(&A, 0, sizeof(A));
    A.n = n;
    const SceneRecs sc = prepare_scene(s, n, c);
    const std::vector<LinRec> lin = prepare_linear_upload(s, n, c, sc, A);
    A.room_nmr = room_neg_margin(A);
    CHECK((int)lin.size() == n + 4, "linear upload: %zu records", lin.size());
    CHECK(A.end_ax[0] <= A.end_ax[1] && A.end_ax[1] <= A.end_ax[2] && A.end_ax[2] <= A.end_big && A.end_big <= n,
          "scan groups");
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a-64 of the table's bytes
    const unsigned char *b = reinterpret_cast<const unsigned char *>(lin.data());
    for (size_t i = 0; i < lin.size() * sizeof(LinRec); ++i)
        h = (h ^ b[i]) * 0x100000001b3ull;
    if (dump) {
        std::printf("  {\"name\": \"%s\", \"n\": %d, \"end_ax\": %s, \"end_big\": %d, \"pairs\": %s, \"pair_lo\": %s, "
                    "\"pair_hi\": %s, \"box_mode\": %d, \"box_walls_out\": %d, \"rec_plus\": %s, \"rec_minus\": %s, "
                    "\"plane_plus\": %s, \"plane_minus\": %s, \"room_nmr\": \"%08x\", \"lin_fnv1a64\": \"%016" PRIx64
                    "\"}%s\n",
                    name, n, list(A.end_ax, 3).c_str(), A.end_big, list(A.pairs, 3).c_str(), hex3(A.pair_lo).c_str(),
                    hex3(A.pair_hi).c_str(), A.box_mode, A.box_walls_out, list(A.rec_plus, 3).c_str(),
                    list(A.rec_minus, 3).c_str(), hex3(A.plane_plus).c_str(), hex3(A.plane_minus).c_str(),
                    bits(A.room_nmr), h, last ? "" : ",");
        return;
    }
    std::printf("%s: n=%d end_ax=%s end_big=%d pairs=%s box_mode=%d box_walls_out=%d room_nmr=%g table=%016" PRIx64 "\n",
                name, n, list(A.end_ax, 3).c_str(), A.end_big, list(A.pairs, 3).c_str(), A.box_mode, A.box_walls_out,
                (double)A.room_nmr, h);
}

int main(int argc, char **argv)
{
    const bool dump = argc > 1 && std::strcmp(argv[1], "--dump") == 0;
    std::vector<Row> rows;
    std::vector<std::string> names;  // (rows point into it: reserved, never reallocated)
    names.reserve(64);
    auto add = [&](const std::string &nm, Row r) {
        names.push_back(nm);
        r.name = names.back().c_str();
        rows.push_back(r);
    };
    for (int n : {9, 10000}) {
        const std::string s = "n" + std::to_string(n) + " ";
        // name, n, slots, W, H, spp, nsub, band, rank, count, chunk, flags, s_begin, s_end, accumulate, walls_out, status
        add(s + "1920x1080x1024 slots2048", {nullptr, n, 2048, 1920, 1080, 1024, 2, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
        add(s + "1920x1080x1024", {nullptr, n, 8192, 1920, 1080, 1024, 2, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
        add(s + "1920x1080x1024 shard 1/8", {nullptr, n, 8192, 1920, 1080, 1024, 2, 1, 0, 8, 0, 0, 0, -1, false, 1, PTG_OK});
        add(s + "1024x768x256", {nullptr, n, 8192, 1024, 768, 256, 2, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
        add(s + "400x300x64", {nullptr, n, 8192, 400, 300, 64, 2, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
        add(s + "1920x1080x4096", {nullptr, n, 8192, 1920, 1080, 4096, 2, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
        add(s + "64x48x16 nsub2", {nullptr, n, 8192, 64, 48, 16, 2, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
        add(s + "64x48x16 nsub3", {nullptr, n, 8192, 64, 48, 16, 3, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
        add(s + "64x48x16 band4 shard 2/3 chunk5", {nullptr, n, 8192, 64, 48, 16, 2, 4, 1, 3, 5, 0, 0, -1, false, 1, PTG_OK});
        add(s + "64x48x16 accumulate [3,11)", {nullptr, n, 8192, 64, 48, 16, 2, 1, 0, 1, 0, 0, 3, 11, true, 1, PTG_OK});
        add(s + "64x48x0", {nullptr, n, 8192, 64, 48, 0, 2, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
    }
    // a wall some ray may start inside: the fast mode scans generically, the exact mode keeps box mode
    add("n9 400x300x64 fast, walls_out 0", {nullptr, 9, 8192, 400, 300, 64, 2, 1, 0, 1, 0, 0, 0, -1, false, 0, PTG_OK});
    add("n9 400x300x64 exact, walls_out 0",
        {nullptr, 9, 8192, 400, 300, 64, 2, 1, 0, 1, 0, PTG_FLAG_EXACT_MATH, 0, -1, false, 0, PTG_OK});
    add("n10000 16384x16384x16 nsub8 chunk1",
        {nullptr, 10000, 8192, 16384, 16384, 16, 8, 1, 0, 1, 1, 0, 0, -1, false, 1, PTG_ERR_UNSUPPORTED});
    // every unit-level kind away from nsub 2 (tests/test_gpu_frame_shapes.py runs these frames on the GPU)
    struct Shape {
        int n, nsub, W, H, samples;
    };
    for (const Shape &f : {Shape{9, 8, 128, 96, 8},      // split tail, accumulating: exactly 12,288 groups
                           Shape{9, 8, 128, 95, 8},      // one row below it: a single level, 2 chunks of 4
                           Shape{9, 8, 256, 160, 8},     // cooperative tail, 1 pixel per wave
                           Shape{9, 5, 513, 160, 8},     // cooperative tail, 50 and 25 valid slots
                           Shape{9, 5, 257, 96, 8},      // accumulating tail, 50 / 25 slots
                           Shape{9, 3, 701, 122, 8},     // accumulating tail, 63 / 9 slots
                           Shape{9, 6, 127, 97, 9},      // tail chunks 2, 2, 2, 2, 1; 36 slots
                           Shape{9, 7, 129, 96, 8},      // 49 slots
                           Shape{9, 1, 1000, 768, 8},    // the last group of a row has 40 of 64 pixels
                           Shape{300, 3, 700, 246, 8},   // BVH tail that cannot pixel-split (7 < 8)
                           Shape{300, 3, 700, 246, 9},   // BVH pixel split, 5 parts of 7 pixels
                           Shape{300, 3, 700, 246, 13},  // BVH pixel split, 7 of 7
                           Shape{300, 1, 1000, 1536, 8},  // BVH pixel split, 8 of 64, ragged last group
                           Shape{300, 8, 192, 128, 8},   // BVH accumulating tail, 1 pixel per wave
                           Shape{300, 8, 96, 64, 16}})   // BVH head/tail plan
        add("n" + std::to_string(f.n) + " " + std::to_string(f.W) + "x" + std::to_string(f.H) + "x" +
                std::to_string(f.samples) + " nsub" + std::to_string(f.nsub),
            {nullptr, f.n, 8192, f.W, f.H, f.samples, f.nsub, 1, 0, 1, 0, 0, 0, -1, false, 1, PTG_OK});
    // the last slab row of rank 1 lies outside the image
    add("n9 129x191x8 nsub7 shard 2/2", {nullptr, 9, 8192, 129, 191, 8, 7, 1, 1, 2, 0, 0, 0, -1, false, 1, PTG_OK});
    // 3-row bands over 2 shards, H no multiple of 6: slab rows past the image in the last band
    add("n9 13x20x4 nsub5 band3 shard 2/2", {nullptr, 9, 8192, 13, 20, 4, 5, 3, 1, 2, 0, 0, 0, -1, false, 1, PTG_OK});
    add("n300 9x20x4 nsub8 band3 shard 1/2", {nullptr, 300, 8192, 9, 20, 4, 8, 3, 0, 2, 0, 0, 0, -1, false, 1, PTG_OK});
    if (dump)
        std::printf("{\"plans\": [\n");
    for (size_t i = 0; i < rows.size() && !fails; ++i)
        run_row(rows[i], dump, i + 1 == rows.size());
    if (fails)
        return 1;
    if (dump)
        std::printf("], \"scenes\": [\n");
    const int cams[2][2] = {{1920, 1080}, {1024, 768}};
    for (int k = 0; k < 2 && !fails; ++k) {
        const int w = cams[k][0], h = cams[k][1];
        const std::string a = k == 0 ? " 16:9" : " 4:3";
        run_scene(("simple" + a).c_str(), pt::simple_scene(w, h), dump, false);
        run_scene(("box" + a).c_str(), pt::box_scene(w, h), dump, false);
        run_scene(("box_mirror" + a).c_str(), pt::box_mirror_scene(w, h), dump, k == 1);
    }
    if (dump)
        std::printf("]}\n");
    return fails ? 1 : 0;
}
