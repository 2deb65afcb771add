"""The denoiser on the GPU (include/ptgpu.h "denoising"): the filter kernels
against the host loop bit for bit, the first-hit features against a numpy
float64 restatement, the render-and-denoise driver against its pieces called
by hand, errors, and the acceptance test: the filtered preview is nearer to
a converged frame than the preview is."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import ptgpu
import tie_scenes
from denoise_camera import OFF_AXIS
from ptgpu.scene import _sub, length

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
# (the box scenes are looked at from a little off the room's axis: tests/denoise_camera.py says why, and
# tests/test_denoise_host.py checks the restatement against itself with this camera)


def scene_and_camera(name, W, H):
    if name in tie_scenes.CASES:  # (tests/test_gpu_ties.py)
        return tie_scenes.make(name, W, H)
    scn = ptgpu.make_scene(name, W, H)
    if name.startswith("box"):
        c = scn.camera_parameters
        c.position = tuple(p + o for p, o in zip(c.position, OFF_AXIS))
        c.focus_distance = length(_sub(c.position, c.direction))
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def _params(iterations=5, spread=0.01):
    k = ptgpu.denoise_defaults()
    k.iterations = iterations
    k.pixel_spread = spread
    return k


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- (a) the filter against the host loop ---------------------------------
@pytest.fixture(scope="module")
def frames():
    return {(W, H): denoise_ref.seeded_frame(W, H, 1000 * W + H)
            for W, H in ((1, 1), (8, 5), (70, 37), (150, 70), (257, 66))}


@pytest.fixture(scope="module")
def program_frames(tmp_path_factory):
    """The host program's own frames and outputs (tests/denoise_check.cpp,
    built here without sanitizers: those belong to the CPU suite)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path_factory.mktemp("denoise_check")
    exe = d / "denoise_check"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1",
                           "-ffp-contract=off", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "denoise_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(d), "1", "3", "5", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return lambda W, H, name, ch: np.fromfile(os.path.join(str(d), f"{W}x{H}_{name}.f32"),
                                              dtype=np.float32).reshape(H, W, ch)


@pytest.mark.parametrize("kernel", [0, 1], ids=["tiled", "plain"])
@pytest.mark.parametrize("iterations", [1, 3, 5, 8])
@pytest.mark.parametrize("W,H", [(1, 1), (8, 5), (70, 37), (150, 70), (257, 66)])
def test_filter_equals_the_host_programs_output(program_frames, kernel, W, H, iterations):
    """ptg_denoise_device against what the stand-alone host program wrote, bit
    for bit, on the program's frames: both kernels (the tiled one up to step
    16, the plain one above: 8 iterations run both), colour and variance."""
    c, v, f = (program_frames(W, H, n, ch) for n, ch in (("color", 3), ("var", 3), ("feat", 12)))
    got, vgot = ptgpu.denoise(_dev(c), _dev(v), _dev(f), _params(iterations), var_out=True, kernel_=kernel)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), program_frames(W, H, f"out{iterations}", 3))
    assert np.array_equal(vgot.cpu().numpy(), program_frames(W, H, f"vout{iterations}", 3))


@pytest.mark.parametrize("kernel", [0, 1], ids=["tiled", "plain"])
@pytest.mark.parametrize("iterations", [1, 3, 5, 8])
@pytest.mark.parametrize("W,H", [(1, 1), (8, 5), (70, 37), (150, 70), (257, 66)])
def test_filter_equals_the_host_loop(frames, kernel, W, H, iterations):
    """ptg_denoise_device == ptg_denoise_host bit for bit: colour and
    variance, with and without the optional variance output.  257x66 is one
    column past four 64-wide tiles; 8x5 loses every far tap from step 4 on;
    70 rows are a ragged last group of lattice rows at every step."""
    c, v, f = frames[(W, H)]
    k = _params(iterations)
    want, vwant = ptgpu.denoise_host(c, v, f, k, var_out=True)
    got, vgot = ptgpu.denoise(_dev(c), _dev(v), _dev(f), k, var_out=True, kernel_=kernel)
    only = ptgpu.denoise(_dev(c), _dev(v), _dev(f), k, kernel_=kernel)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(vgot.cpu().numpy(), vwant)
    assert np.array_equal(only.cpu().numpy(), want)


def test_filter_iterations_0_copies(frames):
    c, v, f = frames[(70, 37)]
    got, vgot = ptgpu.denoise(_dev(c), _dev(v), _dev(f), _params(0), var_out=True)
    assert np.array_equal(got.cpu().numpy(), c) and np.array_equal(vgot.cpu().numpy(), v)


# ---- (b) the features against a numpy float64 first hit --------------------
FEATURE_CASES = [("box", 64, 48, 1), ("box", 64, 48, 2), ("simple", 64, 48, 1), ("simple", 64, 48, 2),
                 ("box_mirror", 64, 48, 1), ("box_mirror", 64, 48, 2), ("synthetic:300", 32, 18, 1),
                 ("synthetic:300", 32, 18, 2)]
# scenes with exact ties (tests/tie_scenes.py): the albedo is the tie's winner -- the sphere visited first,
# lowest scene index -- which the restatement's strict < in index order gives as well
FEATURE_CASES += [(name, 64, 48, nsub) for name in ("twins_lin_low", "twins_bvh_low", "stack9_b") for nsub in (1, 2)]


def _features(scn, cam, p):
    with ptgpu.Context(scn, cam, device=0) as ctx:
        out = ctx.features(p)
        torch.cuda.synchronize()
        return out.cpu().numpy()


@pytest.mark.parametrize("name,W,H,nsub", FEATURE_CASES)
def test_features_against_numpy_first_hit(name, W, H, nsub):
    """hit equals the float64 restatement's on >= 99.5 % of the pixels and,
    where it does, so does the albedo (with nsub 1: the sphere hit).  On those
    pixels normals (absolute), z and P (relative) are within 4 times the
    largest difference a float32 run of the restatement shows against
    float64 on the same scene.  Measured at nsub 1, float32 restatement /
    kernel (the bound is 4 times the first): box |dn| 1.2e-4 / 4.3e-6, dz
    1.0e-5 / 3.8e-7, dP 5.1e-5 / 1.9e-6; simple 1.1e-4 / 1.6e-6, 2.5e-5 /
    1.7e-6, 6.4e-5 / 1.8e-6; box_mirror 1.2e-4 / 8.3e-6, 1.0e-5 / 6.2e-7,
    6.1e-5 / 2.3e-6; synthetic:300 1.8e-3 / 2.3e-5, 2.0e-5 / 4.0e-7, 7.2e-5 /
    1.0e-6.  hit differed on no pixel.  The kernel is far inside: its scan
    keeps the roots as fractions and anchors the huge spheres, the restatement
    rounds sphere.cpp's form in fp32."""
    scn, cam = scene_and_camera(name, W, H)
    got = _features(scn, cam, ptgpu.make_params(W, H, 4, nsub))
    f64, _ = denoise_ref.first_hit(scn, cam, W, H, nsub, np.float64)
    f32, _ = denoise_ref.first_hit(scn, cam, W, H, nsub, np.float32)
    ref = denoise_ref.feature_differences(f32, f64)
    d = denoise_ref.feature_differences(got, f64)
    print(name, nsub, "float32 restatement:", {k: ref[k] for k in "nzP"}, "kernel:", {k: d[k] for k in "nzP"},
          "hit differs:", d["hit_differs"])
    assert ref["hit_differs"] <= 0.005  # the reference alone (also tests/test_denoise_host.py, on the CPU)
    assert d["hit_differs"] <= 0.005
    same_hit = got[..., 7] == f64[..., 7]
    assert np.abs(got[..., 8:11] - f64[..., 8:11])[same_hit].max() <= 1e-6
    assert d["agree"].sum() >= 0.995 * (f64[..., 7] > 0).sum()
    for key in "nzP":
        assert d[key] <= 4.0 * ref[key], (key, d[key], ref[key])
    assert (got[..., 11] == 0).all()
    sky = f64[..., 7] == 0
    assert (got[sky & same_hit][:, :8] == 0).all()


def test_features_rows_shards_and_independence():
    W, H, nsub = 64, 48, 2
    scn, cam = scene_and_camera("simple", W, H)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        base = ctx.features(ptgpu.make_params(W, H, 4, nsub)).cpu().numpy()
        # seed, samples and flags do not matter
        for p in (ptgpu.make_params(W, H, 4, nsub, seed=7), ptgpu.make_params(W, H, 1000, nsub),
                  ptgpu.make_params(W, H, 4, nsub, flags=ptgpu.FLAG_EXACT_MATH),
                  ptgpu.make_params(W, H, 4, nsub, flags=ptgpu.FLAG_LIGHT_SAMPLING | ptgpu.FLAG_MOMENTS)):
            assert np.array_equal(ctx.features(p).cpu().numpy(), base)
        # slab rows past the image stay untouched: 48 rows in bands of 5 make a slab of 50
        p5 = ptgpu.make_params(W, H, 4, nsub, band_rows=5)
        out = torch.full((50, W, 12), 7.0, dtype=torch.float32, device=DEV)
        ctx.features(p5, out)
        o = out.cpu().numpy()
        assert np.array_equal(o[:48], base) and (o[48:] == 7.0).all()
        # a 2-way shard of 3-row bands holds the un-sharded rows
        for rank in (0, 1):
            ps = ptgpu.make_params(W, H, 4, nsub, band_rows=3, shard_rank=rank, shard_count=2)
            slab = ctx.features(ps).cpu().numpy()
            rows = ptgpu.slab_to_image_rows(H, 3, rank, 2)
            assert (rows >= 0).all()
            assert np.array_equal(slab, base[rows])


# ---- (c) the driver against its pieces ----------------------------------------
def _by_hand(scn, cam, W, H, samples, nsub, flags, k):
    p = ptgpu.make_params(W, H, samples, nsub, flags=flags | ptgpu.FLAG_MOMENTS)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        color = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
        var = torch.zeros_like(color)
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, samples)
        ctx.resolve(color, p, samples)
        ctx.noise(p, samples, 0.0, 1.0, var=var)
        feat = ctx.features(p)
        out = ptgpu.denoise(color, var, feat, k)
        torch.cuda.synchronize()
        return out.cpu().numpy(), color.cpu().numpy(), var.cpu().numpy(), feat.cpu().numpy()


@pytest.mark.parametrize("flags", [0, ptgpu.FLAG_EXACT_MATH, ptgpu.FLAG_LIGHT_SAMPLING])
def test_driver_equals_its_pieces(flags):
    W, H, samples, nsub = 48, 32, 8, 2
    scn, cam = scene_and_camera("box", W, H)
    k = ptgpu.denoise_defaults()
    k.pixel_spread = ptgpu.pixel_spread(cam, W, H)
    want, _, _, _ = _by_hand(scn, cam, W, H, samples, nsub, flags, k)
    img = np.zeros((H, W, 3))
    ptgpu.render_denoised(scn, cam, img, W, H, samples, nsub, device=0, flags=flags)  # params None: the same k
    assert np.array_equal(img, want.astype(np.float64))
    img2 = np.ones((H, W, 3))
    ptgpu.render_denoised(scn, cam, img2, W, H, samples, nsub, device=0, flags=flags, params=k)
    assert np.array_equal(img2, 1.0 + want.astype(np.float64))  # it adds


@pytest.mark.parametrize("W,H,band_rows", [(70, 37, 1), (257, 66, 1), (71, 37, 4), (33, 21, 2)])
def test_drivers_at_frames_that_are_no_multiple_of_anything(W, H, band_rows):
    """Both drivers where rows * W is no multiple of 4 (70x37, 257x66), and
    with an odd width under bands of several rows (the slab then has more
    rows than the image: 71x37 in bands of 4 is 40 rows, 33x21 in bands of 2
    is 22): the parts of the drivers' one allocation must stay aligned for
    the feature kernel's float4 stores and the check's 64-bit counters.  The
    image does not depend on band_rows: it equals the pieces called by hand."""
    samples, nsub = 4, 2
    scn, cam = scene_and_camera("simple", W, H)
    k = ptgpu.denoise_defaults()
    k.pixel_spread = ptgpu.pixel_spread(cam, W, H)
    want, _, _, _ = _by_hand(scn, cam, W, H, samples, nsub, 0, k)
    sp, ca = scn.to_array(), cam.to_array()
    p = ptgpu.make_params(W, H, samples, nsub, band_rows=band_rows)
    L = ptgpu.lib()
    a, b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    ptgpu._abi.check(L.ptg_render_denoised(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                           C.byref(p), 0, None, a.ctypes.data_as(C.c_void_p)), "ptg_render_denoised")
    assert np.array_equal(a, want.astype(np.float64))
    target = ptgpu.NoiseTarget(0.0, 0.01, 0.01, 2, 0)  # never met: both passes (2, then 4 samples) and both checks run
    rep = ptgpu.NoiseReport()
    ptgpu._abi.check(L.ptg_render_to_noise_denoised(sp.ctypes.data_as(C.c_void_p), len(sp),
                                                    ca.ctypes.data_as(C.c_void_p), C.byref(p), 0, C.byref(target), None,
                                                    b.ctypes.data_as(C.c_void_p), C.byref(rep)),
                     "ptg_render_to_noise_denoised")
    assert (rep.samples_done, rep.passes, rep.pixels) == (samples, 2, W * H)
    assert np.array_equal(b, a)


def test_driver_iterations_0_is_the_plain_render():
    W, H, samples, nsub = 48, 32, 8, 2
    scn, cam = scene_and_camera("simple", W, H)
    a, b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    ptgpu.render(scn, cam, a, W, H, samples, nsub, device=0)
    ptgpu.render_denoised(scn, cam, b, W, H, samples, nsub, device=0, params=_params(0))
    assert np.array_equal(a, b)


# ---- (d) errors and state ---------------------------------------------------------
def test_errors_on_the_device():
    W, H = 16, 8
    scn, cam = scene_and_camera("box", W, H)
    img = np.zeros((H, W, 3))
    with pytest.raises(ptgpu.PtgError, match="samples"):
        ptgpu.render_denoised(scn, cam, img, W, H, 1, device=0)
    with pytest.raises(ptgpu.PtgError, match="fp32 only"):
        ptgpu.render_denoised(scn, cam, img, W, H, 4, device=0, flags=ptgpu.FLAG_REFERENCE_F64)
    sp, ca = scn.to_array(), cam.to_array()
    p = ptgpu.make_params(W, H, 4, shard_count=2)
    L = ptgpu.lib()
    assert L.ptg_render_denoised(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p), C.byref(p),
                                 0, None, img.ctypes.data_as(C.c_void_p)) == -1
    assert b"shard_count" in L.ptg_last_error()
    assert (img == 0).all()
    c = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
    f = torch.zeros((H, W, 12), dtype=torch.float32, device=DEV)
    small = torch.zeros(ptgpu.denoise_scratch_bytes(W, H) // 4 - 1, dtype=torch.float32, device=DEV)
    with pytest.raises(ptgpu.PtgError, match="scratch"):
        ptgpu.denoise(c, c.clone(), f, _params(), scratch=small)
    with pytest.raises(ptgpu.PtgError, match="iterations"):
        ptgpu.denoise(c, c.clone(), f, _params(9))


def test_features_leave_the_accumulation_state_alone():
    """ptg_features_device between the passes of a progressive frame changes
    neither the sums nor what the context knows of them: the frame resolves
    and its noise is read as without the call."""
    W, H, samples, nsub = 32, 16, 4, 2
    scn, cam = scene_and_camera("box", W, H)
    p = ptgpu.make_params(W, H, samples, nsub, flags=ptgpu.FLAG_MOMENTS)
    res = []
    for with_features in (False, True):
        with ptgpu.Context(scn, cam, device=0) as ctx:
            color = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
            var = torch.zeros_like(color)
            ctx.reset_accumulation(p)
            ctx.accumulate(p, 0, 2)
            if with_features:
                ctx.features(p)
            ctx.accumulate(p, 2, samples)
            ctx.resolve(color, p, samples)
            ctx.noise(p, samples, 0.0, 1.0, var=var)
            res.append((color.cpu().numpy(), var.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- (e) acceptance: the filter helps ------------------------------------------------
@pytest.mark.parametrize("name", ["box", "simple"])
def test_denoised_preview_is_nearer_the_converged_frame(name):
    """64x48, 2x2 sub-pixels, 16 samples each, default parameters, the
    scene's own camera: RMSE against ptg_render_device's frame at 4096 samples
    per sub-pixel (light sampling on, for a cleaner reference) falls.
    Measured denoised / noisy: see CHANGELOG.md."""
    W, H, nsub = 64, 48, 2
    scn = ptgpu.make_scene(name, W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        ref = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
        ctx.render_device(ref, ptgpu.make_params(W, H, 4096, nsub, flags=ptgpu.FLAG_LIGHT_SAMPLING))
        torch.cuda.synchronize()
        ref = ref.cpu().numpy().astype(np.float64)
    noisy, den = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    ptgpu.render(scn, cam, noisy, W, H, 16, nsub, device=0)
    ptgpu.render_denoised(scn, cam, den, W, H, 16, nsub, device=0)
    rmse = lambda a: float(np.sqrt(((a - ref) ** 2).mean()))  # noqa: E731
    print(f"{name}: RMSE noisy {rmse(noisy):.5f} denoised {rmse(den):.5f} ratio {rmse(den) / rmse(noisy):.3f}")
    assert rmse(den) < rmse(noisy)


# ---- (f) the command-line tool ----------------------------------------------------------
def test_cli_denoise_writes_the_drivers_image(tmp_path):
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(ptgpu.LIB_PATH), "pt_render_gpu")
    W, H, spp = 64, 48, 64

    def run(*extra):
        out = tmp_path / f"o{len(extra)}_{'_'.join(e.strip('-') for e in extra[:1])}.ppm"
        r = subprocess.run([cli, "--scene", "box", "--width", str(W), "--height", str(H), "--format", "p6",
                            "--spp", str(spp), "--out", str(out), *extra], capture_output=True, text=True, timeout=120)
        return r, (out.read_bytes() if out.exists() else b"")

    head = len(f"P6\n{W} {H}\n255\n")

    class tonemap:  # utils.cpp:11-16; equal up to one 8-bit step where the two pow() round a tie apart
        def __init__(self, img):
            self.v = np.round(np.clip(img, 0, 1) ** (1 / 2.2) * 255).astype(np.int16).reshape(-1)

        def __eq__(self, data):
            d = np.abs(np.frombuffer(data, dtype=np.uint8).astype(np.int16) - self.v)
            return len(data) == self.v.size and d.max() <= 1 and (d != 0).sum() <= 2

    r, plain = run()
    r0, it0 = run("--denoise", "--denoise-iterations", "0")
    assert r.returncode == 0 and r0.returncode == 0 and plain == it0 and len(plain) == head + W * H * 3

    scn = ptgpu.make_scene("box", W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    r, got = run("--denoise")
    assert r.returncode == 0, r.stderr
    want = np.zeros((H, W, 3))
    ptgpu.render_denoised(scn, cam, want, W, H, spp // 4, 2, device=0)
    assert got[head:] == tonemap(want)
    r, got3 = run("--denoise", "--denoise-iterations", "3")
    assert r.returncode == 0, r.stderr
    k = ptgpu.denoise_defaults()
    k.iterations, k.pixel_spread = 3, 0.0
    want3 = np.zeros((H, W, 3))
    ptgpu.render_denoised(scn, cam, want3, W, H, spp // 4, 2, device=0, params=k)
    assert got3[head:] == tonemap(want3) and got3 != got
    # with --noise-target: the frame at the spp the run stopped at, filtered
    r, gotn = run("--denoise", "--noise-target", "1000", "--min-spp", "16")
    assert r.returncode == 0 and "stopped at 16 spp" in r.stderr, r.stderr
    wantn = np.zeros((H, W, 3))
    ptgpu.render_denoised(scn, cam, wantn, W, H, 4, 2, device=0)
    assert gotn[head:] == tonemap(wantn)
    # --features-out: Context.features through the documented mapping
    r, _ = run("--features-out", str(tmp_path / "f"))
    assert r.returncode == 0, r.stderr
    with ptgpu.Context(scn, cam, device=0) as ctx:
        feat = ctx.features(ptgpu.make_params(W, H, 4, 2)).cpu().numpy().astype(np.float64)
    step = lambda x: np.floor(np.clip(x, 0, 1) * 255 + 0.5).astype(np.uint8).tobytes()  # noqa: E731
    assert (tmp_path / "f_normal.ppm").read_bytes() == f"P6\n{W} {H}\n255\n".encode() + step((feat[..., 0:3] + 1) / 2)
    assert (tmp_path / "f_albedo.ppm").read_bytes() == f"P6\n{W} {H}\n255\n".encode() + step(feat[..., 8:11])
    z16 = np.floor(65535.0 * feat[..., 3] / feat[..., 3].max() + 0.5).astype(">u2").tobytes()
    assert (tmp_path / "f_distance.pgm").read_bytes() == f"P5\n{W} {H}\n65535\n".encode() + z16

    # the refusals
    for extra, word in ((("--denoise", "--noise-target", "0.1", "--adaptive"), "--adaptive"),
                        (("--denoise", "--devices", "0,1"), "one device"),
                        (("--denoise-iterations", "3"), "--denoise"),
                        (("--denoise", "--denoise-iterations", "9"), "0..8")):
        r, _ = run(*extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
    r = subprocess.run([cli, "--denoise", "--spp", "4", "--width", "8", "--height", "8"], capture_output=True, text=True)
    assert r.returncode == 2 and "--spp >= 8" in r.stderr


def test_to_noise_denoised_is_the_filtered_frame_it_stopped_at():
    """ptg_render_to_noise_denoised: ptg_render_to_noise's report, and
    ptg_render_denoised's image at the samples it stopped at, bit for bit --
    stopping early, and running to the budget."""
    W, H, nsub = 48, 32, 2
    scn, cam = scene_and_camera("box", W, H)
    for rel_error, samples in ((1000.0, 16), (0.0, 8)):
        plain, a, b = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
        want_rep = ptgpu.render_to_noise(scn, cam, plain, W, H, samples, rel_error, min_samples=4, num_subpixels=nsub,
                                         device=0)
        rep = ptgpu.render_to_noise_denoised(scn, cam, a, W, H, samples, rel_error, min_samples=4,
                                             num_subpixels=nsub, device=0)
        assert rep == want_rep and rep["samples_done"] == (4 if rel_error else samples)
        ptgpu.render_denoised(scn, cam, b, W, H, rep["samples_done"], nsub, device=0)
        assert np.array_equal(a, b) and not np.array_equal(a, plain)
