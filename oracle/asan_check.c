/* asan_check.c -- TEST INFRASTRUCTURE ONLY (tests/test_oracle_asan.py).
 *
 * Drives the oracle's Mode B through box mode's degenerate case under
 * AddressSanitizer: a scene whose only walls are a left/right pair, a camera
 * with aperture 0 looking along -z, and image column x = W/2 of a 2^19-wide
 * image with 8 sub-pixels, where the jittered camera ray has d.x == 0 exactly
 * for 1/8 of the samples (xin rounds to 2^18, s = 0.5, d.x = X.x/2 + base.x).
 * No axis the ray moves toward then has a reachable wall plane, and box mode
 * must not select a missing wall (it read the record before the
 * scene array).  Exit status 0 and "ok <count of d.x == 0 rays>" on success.
 *
 * Then Mode A/xs with a light list (po_render_xs_f64_ls) on the 16 lights of
 * tests/light_zoo.py's `sixteen`, built by the same rule: every index of the
 * full list is picked, scanned for and looked up under the sanitizers.  A
 * black frame or a count without shadow segments is an error. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "pt_oracle.h"

/* tests/light_zoo.py: sixteen_lights() over a floor of R = 100 and a grey ball */
static int sixteen(po_sphere *s, int32_t *lights)
{
    const double floor_r = 100.0;
    memset(s, 0, 18 * sizeof(po_sphere));
    s[0].radius = floor_r; s[0].position[1] = -floor_r;
    s[0].color[0] = s[0].color[1] = s[0].color[2] = 0.6;
    s[1].radius = 0.6; s[1].position[1] = 0.6;
    s[1].color[0] = s[1].color[1] = s[1].color[2] = 0.7;
    for (int i = 0; i < 16; ++i) {
        po_sphere *l = &s[2 + i];
        const double r = 0.02 * pow(100.0, i / 15.0), ang = 2.4 * i, dist = 1.5 + 0.35 * i;
        const double e = r < 0.25 ? 0.25 / r : 1.0;
        l->radius = r;
        l->position[0] = dist * cos(ang);
        l->position[1] = sqrt((floor_r + r) * (floor_r + r) - dist * dist) - floor_r + 0.3 * (i % 4);
        l->position[2] = dist * sin(ang);
        l->emission[0] = e * (1.0 + (i % 3));
        l->emission[1] = e * (1.0 + 0.5 * (i % 5));
        l->emission[2] = e * (3.0 - 0.6 * (i % 4));
        if (i == 0) {
            l->position[0] = 30.0; l->position[1] = 25.0; l->position[2] = -40.0;
            l->emission[0] = l->emission[1] = l->emission[2] = 5.0;
        }
        l->color[0] = l->color[1] = l->color[2] = i % 3 == 0 ? 0.0 : 0.9;
        l->material = i % 3;
        lights[i] = 2 + i;
    }
    return 18;
}

static int light_list_check(void)
{
    po_sphere s[18];
    int32_t lights[16];
    const int n = sixteen(s, lights), W = 32, H = 24;
    po_camera_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.position[1] = 3.0; cfg.position[2] = 9.0;
    cfg.direction[1] = 0.5;
    cfg.up[1] = 1.0;
    cfg.aspect_ratio = (double)W / (double)H;
    cfg.vertical_fov_radians = 0.8;
    cfg.focal_length = 1.0;
    cfg.focus_distance = sqrt(2.5 * 2.5 + 81.0);
    po_camera cam;
    po_camera_with_config(&cfg, &cam);
    static double img[32 * 24 * 3], plain[32 * 24 * 3];
    uint64_t segs = 0, psegs = 0;
    if (po_render_xs_f64_ls(s, n, &cam, W, H, 2, 2, 0x5EED0001ull, lights, 16, 0, H, 1, 1, img, &segs) ||
        po_render_xs_f64_ls(s, n, &cam, W, H, 2, 2, 0x5EED0001ull, NULL, 0, 0, H, 1, 1, plain, &psegs))
        return 3;
    double sum = 0.0;
    for (int i = 0; i < W * H * 3; ++i)
        sum += img[i];
    if (!(sum > 0.0) || segs <= psegs) {
        printf("light list: sum %.6f segments %llu (plain %llu)\n", sum, (unsigned long long)segs,
               (unsigned long long)psegs);
        return 4;
    }
    return 0;
}

int main(void)
{
    po_sphere s[3];
    memset(s, 0, sizeof(s));
    const double big = 1e6, off = 0.4;
    s[0].radius = big; s[0].position[0] = -big - off; s[0].position[2] = -1.0;
    s[0].color[0] = 0.9; s[0].color[1] = 0.1; s[0].color[2] = 0.2;
    s[1].radius = big; s[1].position[0] = big + off; s[1].position[2] = -1.0;
    s[1].color[0] = 0.3; s[1].color[1] = 0.1; s[1].color[2] = 0.9;
    s[2].radius = 0.2; s[2].position[1] = -0.2; s[2].position[2] = -1.0;
    s[2].color[0] = s[2].color[1] = s[2].color[2] = 1.0; s[2].material = 1;
    const int W = 1 << 19, H = 1, nsub = 8;
    po_camera_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.position[2] = 2.0;
    cfg.direction[2] = -1.0;
    cfg.up[1] = 1.0;
    cfg.aspect_ratio = (double)W / (double)H;
    cfg.vertical_fov_radians = 0.5;
    cfg.focal_length = 1.0;
    cfg.aperture = 0.0;
    cfg.focus_distance = 3.0;
    po_camera cam;
    po_camera_with_config(&cfg, &cam);
    int32_t axis[3], order[3];
    po_scan_layout(s, 3, &cam, axis, order);
    if (axis[0] != 3 || axis[1] != 3) {
        printf("not a wall pair: %d %d\n", axis[0], axis[1]);
        return 2;
    }
    float out[3];
    double sum = 0.0;
    for (int sy = 0; sy < nsub; ++sy)
        for (uint32_t k = 0; k < 256; ++k) {
            po_sample_f32(s, 3, &cam, W, H, nsub, 0x5EED0001ull, W / 2, 0, 0, sy, k, out);
            sum += out[0] + out[1] + out[2];
        }
    const int rc = light_list_check();
    if (rc)
        return rc;
    printf("ok %.6f\n", sum);
    return 0;
}
