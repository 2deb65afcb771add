"""Host-side render API over the C ABI.

* render(...)            -- the drop-in for the reference's row loop
                            (main.cpp:214-236): fills the caller's image
                            (H*W RGB doubles, reference row order) exactly as
                            the loop would, through ptg_render.
* render_to_noise(...),  -- render() that stops when a noise target is met;
  render_adaptive(...)      the adaptive one gives the later passes only to
                            the pixels still over it (a sample count per pixel).
* render_denoised(...),  -- render() followed by the variance-guided a-trous
  denoise(...)              filter (first-hit features from Context.features);
                            denoise() filters device tensors the caller holds.
                            render_adaptive_denoised() filters an adaptive
                            frame (variance from each pixel's own count), and
                            MultiContext.render_*_denoised() frames sharded
                            over several GPUs, bit for bit the same image.
* Context                -- device-resident scene for repeated renders into
                            torch CUDA tensors (bench, multi-GPU).
* render_sharded(...)    -- one process per GPU: each rank renders its
                            interleaved row bands into a slab, one gather
                            (RCCL over xGMI via torch.distributed) collects
                            the slabs on rank 0, ptg_unshard_device restores
                            the row order.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional

import numpy as np

from ._abi import NOISE_MAX_PASSES, AdaptiveReport, AdaptiveTarget, DenoiseParams, NoiseReport, NoiseTarget, Params, check, lib
from .scene import CAMERA_DT, SPHERE_DT, camera, scene

DEFAULT_SEED = 0x5EED0001
DEFAULT_BAND_ROWS = 1  # single-row bands: equal shards whenever N divides H (tools/shard_sim.py: 8-way 95.8 % vs 94.4 % with 8-row bands)


def _spheres_array(scn) -> np.ndarray:
    if isinstance(scn, scene):
        return scn.to_array()
    a = np.ascontiguousarray(scn)
    if a.dtype != SPHERE_DT:
        raise TypeError("spheres must be a ptgpu.scene or a SPHERE_DT array")
    return a


def _camera_array(cam) -> np.ndarray:
    if isinstance(cam, camera):
        return cam.to_array()
    a = np.ascontiguousarray(cam).reshape(1)
    if a.dtype != CAMERA_DT:
        raise TypeError("cam must be a ptgpu.camera or a CAMERA_DT array")
    return a


FLAG_COUNT_TESTS = 1  # include/ptgpu.h PTG_FLAG_COUNT_TESTS
FLAG_COUNT_NONFINITE = 2  # include/ptgpu.h PTG_FLAG_COUNT_NONFINITE (4 counters)
FLAG_REFERENCE_F64 = 4  # include/ptgpu.h PTG_FLAG_REFERENCE_F64: the reference's double arithmetic (parity mode)
FLAG_EXACT_MATH = 8  # include/ptgpu.h PTG_FLAG_EXACT_MATH: exact sequences, bit for bit the oracle's Mode B
FLAG_MOMENTS = 16  # include/ptgpu.h PTG_FLAG_MOMENTS: progressive passes also sum second moments (Context.noise)
# include/ptgpu.h PTG_FLAG_LIGHT_SAMPLING: next-event estimation for the small emissive spheres (light_list).
# Unbiased like the plain estimator: compare the two on raw sums (Context.read_moments), not on clamped images
FLAG_LIGHT_SAMPLING = 32
MAX_LIGHTS = 16  # include/ptgpu.h PTG_MAX_LIGHTS
# include/ptgpu.h PTG_FLAG_STRATIFIED: four pairs of draws per path (jitter, lens, the first hit's diffuse bounce
# and light sample) from a scrambled Sobol' (0,2)-sequence in the sample index (Context.sampler_pairs)
FLAG_STRATIFIED = 64


def _n_counters(flags: int) -> int:
    return 4 if flags & FLAG_COUNT_NONFINITE else (3 if flags & FLAG_COUNT_TESTS else 1)


def make_params(width, height, samples, num_subpixels=2, seed=DEFAULT_SEED, band_rows=DEFAULT_BAND_ROWS,
                shard_rank=0, shard_count=1, chunk_samples=0, flags=0) -> Params:
    return Params(int(width), int(height), int(samples), int(num_subpixels), int(seed) & (2**64 - 1),
                  int(band_rows), int(shard_rank), int(shard_count), int(chunk_samples), int(flags))


def shard_rows(height: int, band_rows: int, shard_count: int) -> int:
    out = C.c_int32(0)
    check(lib().ptg_shard_rows(height, band_rows, shard_count, C.byref(out)), "ptg_shard_rows")
    return out.value


def slab_to_image_rows(height: int, band_rows: int, shard_rank: int, shard_count: int) -> np.ndarray:
    """Output row of every slab row (-1 for padding), the mapping ptg_render_device uses."""
    rows = shard_rows(height, band_rows, shard_count)
    j = np.arange(rows)
    band = j // band_rows
    r = (band * shard_count + shard_rank) * band_rows + (j - band * band_rows)
    return np.where(r < height, r, -1)


def unshard_host(gathered: np.ndarray, width: int, height: int, band_rows: int, shard_count: int) -> np.ndarray:
    """Host statement of ptg_unshard_device (rank-major slabs -> image rows)."""
    rows = shard_rows(height, band_rows, shard_count)
    g = np.asarray(gathered).reshape(shard_count * rows, width * 3)
    out = np.zeros((height, width * 3), dtype=g.dtype)
    for k in range(shard_count):
        m = slab_to_image_rows(height, band_rows, k, shard_count)
        ok = m >= 0
        out[m[ok]] = g[k * rows:(k + 1) * rows][ok]
    return out.reshape(height, width, 3)


def render(scn, cam, image: np.ndarray, width: int, height: int, samples: int, num_subpixels: int = 2,
           seed: int = DEFAULT_SEED, device: int = -1, flags: int = 0) -> np.ndarray:
    """Drop-in for main.cpp:214-236: image (W*H RGB doubles, reference row
    order, zero-initialised by the caller like main.cpp:210-212) receives
    += sum_sub clamp(mean radiance) / num_subpixels^2 for every pixel."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    img = image if image.dtype == np.float64 and image.flags["C_CONTIGUOUS"] else None
    if img is None or img.size != width * height * 3:
        raise ValueError("image must be a C-contiguous float64 array of width*height*3 values")
    p = make_params(width, height, samples, num_subpixels, seed, flags=flags)
    check(lib().ptg_render(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p), C.byref(p),
                           int(device), img.ctypes.data_as(C.c_void_p)), "ptg_render")
    return image


def noise_schedule(min_samples: int, samples: int) -> list:
    """ptg_noise_schedule (host only): the pass ends min_samples, 2 min_samples,
    ... of a render-until-converged frame; the last one is `samples`."""
    ends = (C.c_int32 * NOISE_MAX_PASSES)()
    n = C.c_int32(0)
    check(lib().ptg_noise_schedule(int(min_samples), int(samples), ends, NOISE_MAX_PASSES, C.byref(n)),
          "ptg_noise_schedule")
    return list(ends[:n.value])


def render_to_noise(scn, cam, image: np.ndarray, width: int, height: int, samples: int, rel_error: float,
                    floor: float = 0.01, max_fraction: float = 0.01, min_samples: int = 16, num_subpixels: int = 2,
                    seed: int = DEFAULT_SEED, device: int = -1, flags: int = 0) -> dict:
    """ptg_render_to_noise: render() that stops at the first of the passes
    noise_schedule(min_samples, samples) after which at most max_fraction of
    the pixels has a relative standard error above rel_error (`floor`: the
    least pixel mean the error is taken relative to).  The image equals
    render()'s at samples = the returned samples_done bit for bit.  Returns
    the report: samples_done, passes, converged, pixels, pixels_over, max_rho,
    mean_rho, pass_samples, pass_over."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    if image.dtype != np.float64 or not image.flags["C_CONTIGUOUS"] or image.size != width * height * 3:
        raise ValueError("image must be a C-contiguous float64 array of width*height*3 values")
    p = make_params(width, height, samples, num_subpixels, seed, flags=flags)
    target = NoiseTarget(float(rel_error), float(floor), float(max_fraction), int(min_samples), 0)
    rep = NoiseReport()
    check(lib().ptg_render_to_noise(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                    C.byref(p), int(device), C.byref(target), image.ctypes.data_as(C.c_void_p),
                                    C.byref(rep)), "ptg_render_to_noise")
    return _noise_report(rep)


def _noise_report(rep: NoiseReport) -> dict:
    return {"samples_done": rep.samples_done, "passes": rep.passes, "converged": rep.converged,
            "pixels": rep.pixels, "pixels_over": rep.pixels_over, "max_rho": rep.max_rho, "mean_rho": rep.mean_rho,
            "pass_samples": list(rep.pass_samples[:rep.passes]), "pass_over": list(rep.pass_over[:rep.passes])}


def _adaptive_report(rep: AdaptiveReport) -> dict:
    n = rep.passes
    return {"passes": n, "converged": rep.converged, "max_samples": rep.max_samples, "pixels": rep.pixels,
            "pixels_over": rep.pixels_over, "max_rho": rep.max_rho, "mean_rho": rep.mean_rho,
            "total_samples": rep.total_samples,
            "mean_samples": rep.total_samples / rep.pixels if rep.pixels else 0.0,
            "counters": list(rep.counters), "pass_added": list(rep.pass_added[:n]),
            "pass_over": list(rep.pass_over[:n]), "pass_active": list(rep.pass_active[:n])}


def render_adaptive(scn, cam, image: np.ndarray, width: int, height: int, samples: int, rel_error: float,
                    floor: float = 0.01, max_fraction: float = 0.01, min_samples: int = 16, dilate: int = 1,
                    num_subpixels: int = 2, seed: int = DEFAULT_SEED, device: int = -1, flags: int = 0,
                    sample_counts: bool = False):
    """ptg_render_adaptive: render_to_noise() whose later passes sample only
    the pixels still over the target, or within `dilate` pixels of one that
    is.  A pixel's value equals render()'s at samples = its own count bit for
    bit.  Returns the report (passes, converged, max_samples, pixels,
    pixels_over, max_rho, mean_rho, total_samples = the sum of the pixels'
    counts, mean_samples, counters, and per pass: pass_added, pass_over,
    pass_active); with sample_counts=True returns (report, counts) with
    counts the int32 [height, width] samples per sub-pixel of every pixel,
    in the image's row order."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    if image.dtype != np.float64 or not image.flags["C_CONTIGUOUS"] or image.size != width * height * 3:
        raise ValueError("image must be a C-contiguous float64 array of width*height*3 values")
    p = make_params(width, height, samples, num_subpixels, seed, flags=flags)
    target = AdaptiveTarget(float(rel_error), float(floor), float(max_fraction), int(min_samples), int(dilate))
    rep = AdaptiveReport()
    counts = np.zeros((height, width), dtype=np.int32) if sample_counts else None
    check(lib().ptg_render_adaptive(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                    C.byref(p), int(device), C.byref(target), image.ctypes.data_as(C.c_void_p),
                                    counts.ctypes.data_as(C.c_void_p) if sample_counts else None, C.byref(rep)),
          "ptg_render_adaptive")
    out = _adaptive_report(rep)
    return (out, counts) if sample_counts else out


def render_multi(scn, cam, image: np.ndarray, width: int, height: int, samples: int, devices,
                 num_subpixels: int = 2, seed: int = DEFAULT_SEED, band_rows: int = DEFAULT_BAND_ROWS,
                 flags: int = 0) -> np.ndarray:
    """ptg_render_multi: the drop-in render over several GPUs of this process
    (distinct devices) -- shards rendered concurrently, ONE RCCL gather to
    devices[0], un-shard there; the image equals render()'s bit for bit."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    if image.dtype != np.float64 or not image.flags["C_CONTIGUOUS"] or image.size != width * height * 3:
        raise ValueError("image must be a C-contiguous float64 array of width*height*3 values")
    p = make_params(width, height, samples, num_subpixels, seed, band_rows, flags=flags)
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    check(lib().ptg_render_multi(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p), C.byref(p),
                                 devs, len(devices), image.ctypes.data_as(C.c_void_p)), "ptg_render_multi")
    return image


class MultiContext:
    """A persistent multi-GPU context (ptg_multi): the scene on every device,
    the RCCL communicator of the device set, the root's gather buffers --
    repeated frames and progressive passes reuse them.  `local_shards=n`
    (tests) puts n shards on the one device `devices[0]`, gathered by device
    copies into the layout an n-rank ncclGather produces."""

    def __init__(self, scn, cam, devices, local_shards: int = 0):
        sp = _spheres_array(scn)
        ca = _camera_array(cam)
        h = C.c_void_p()
        if local_shards:
            check(lib().ptg_multi_create_local_(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                                int(devices[0]), int(local_shards), C.byref(h)),
                  "ptg_multi_create_local_")
        else:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            check(lib().ptg_multi_create(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p), devs,
                                         len(devices), C.byref(h)), "ptg_multi_create")
        self._h = h
        self.n_devices = int(local_shards) if local_shards else len(devices)

    def close(self):
        if self._h:
            lib().ptg_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _image(image, params, dtype):
        if image.dtype != dtype or not image.flags["C_CONTIGUOUS"] or \
                image.size != params.width * params.height * 3:
            raise ValueError(f"image must be a C-contiguous {np.dtype(dtype).name} array of width*height*3 values")
        return image.ctypes.data_as(C.c_void_p)

    def render(self, image: np.ndarray, params: Params) -> np.ndarray:
        """The frame over all devices, added into `image` (float64, like render())."""
        check(lib().ptg_multi_render(self._h, C.byref(params), self._image(image, params, np.float64)),
              "ptg_multi_render")
        return image

    def frame_device(self, params: Params, counters: bool = False):
        """ptg_multi_frame_device: the frame over all devices, kept in HBM
        (render, ONE gather, un-shard; synchronous).  With counters=True
        (params needs FLAG_COUNT_TESTS) returns the 4 summed kernel counters."""
        c = np.zeros(4, dtype=np.uint64)
        check(lib().ptg_multi_frame_device(self._h, C.byref(params), c.ctypes.data_as(C.c_void_p) if counters else None),
              "ptg_multi_frame_device")
        return c if counters else None

    def frame_timing(self):
        """(render_ms per device, frame_ms on the root) of the last frame_device."""
        r = np.zeros(self.n_devices, dtype=np.float32)
        f = np.zeros(1, dtype=np.float32)
        check(lib().ptg_multi_frame_timing(self._h, r.ctypes.data_as(C.c_void_p), self.n_devices,
                                           f.ctypes.data_as(C.c_void_p)), "ptg_multi_frame_timing")
        return r.astype(float).tolist(), float(f[0])

    def image(self, params: Params) -> np.ndarray:
        """The last frame_device image, [H, W, 3] float32 in the reference's row order."""
        out = np.empty(params.width * params.height * 3, dtype=np.float32)
        check(lib().ptg_multi_image(self._h, C.byref(params), out.ctypes.data_as(C.c_void_p)), "ptg_multi_image")
        return out.reshape(params.height, params.width, 3)

    def comm_info(self):
        """ptg_multi_comm_info: per shard (ncclCommCount, ncclCommCuDevice,
        ncclCommUserRank) of its RCCL communicator -- (0, the shard's device,
        -1) for local shards (no communicator)."""
        n = self.n_devices
        ranks = np.zeros(n, dtype=np.int32)
        devs = np.zeros(n, dtype=np.int32)
        user = np.zeros(n, dtype=np.int32)
        check(lib().ptg_multi_comm_info(self._h, ranks.ctypes.data_as(C.c_void_p), devs.ctypes.data_as(C.c_void_p),
                                        user.ctypes.data_as(C.c_void_p), n), "ptg_multi_comm_info")
        return [(int(r), int(d), int(u)) for r, d, u in zip(ranks, devs, user)]

    def inject_gather_fault_(self, shard: int) -> None:
        """Tests: the next RCCL gather fails at `shard` (-1: off)."""
        check(lib().ptg_multi_inject_gather_fault_(self._h, int(shard)), "ptg_multi_inject_gather_fault_")

    def reset_accumulation(self, params: Params) -> None:
        check(lib().ptg_multi_reset_accumulation(self._h, C.byref(params)), "ptg_multi_reset_accumulation")

    def accumulate(self, params: Params, sample_begin: int, sample_end: int) -> None:
        check(lib().ptg_multi_accumulate(self._h, C.byref(params), int(sample_begin), int(sample_end)),
              "ptg_multi_accumulate")

    def resolve(self, image: np.ndarray, params: Params, samples_done: int) -> np.ndarray:
        """The image of the samples accumulated so far, written to `image` (float32)."""
        check(lib().ptg_multi_resolve(self._h, C.byref(params), int(samples_done),
                                      self._image(image, params, np.float32)), "ptg_multi_resolve")
        return image

    # ---- noise-target and adaptive frames over all devices (ptg_multi_noise ... ptg_multi_render_adaptive)
    def noise(self, params: Params, samples_done: int, rel_error: float, floor: float) -> np.ndarray:
        """Context.noise's four statistics (uint64 [4]) of the whole frame,
        after accumulate() passes with FLAG_MOMENTS."""
        st = np.zeros(4, dtype=np.uint64)
        check(lib().ptg_multi_noise(self._h, C.byref(params), int(samples_done), float(rel_error), float(floor),
                                    st.ctypes.data_as(C.c_void_p)), "ptg_multi_noise")
        return st

    def set_active_mask(self, params: Params, mask: Optional[np.ndarray] = None) -> None:
        """The active list from a host byte mask ([H, W] uint8 in the image's
        row order, != 0 is active; None: every pixel): each shard gets its rows."""
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.size != params.width * params.height:
                raise ValueError("mask must hold width*height bytes")
        check(lib().ptg_multi_set_active_mask(self._h, C.byref(params),
                                              mask.ctypes.data_as(C.c_void_p) if mask is not None else None),
              "ptg_multi_set_active_mask")

    def select_active(self, params: Params, rel_error: float, floor: float, dilate: int = 0) -> np.ndarray:
        """Context.select_active for the whole frame (one all-gather of the
        over bytes, so any dilate in 0..8): its six statistics (uint64 [6])."""
        st = np.zeros(6, dtype=np.uint64)
        check(lib().ptg_multi_select_active(self._h, C.byref(params), float(rel_error), float(floor), int(dilate),
                                            st.ctypes.data_as(C.c_void_p)), "ptg_multi_select_active")
        return st

    def accumulate_active(self, params: Params, add_samples: int) -> None:
        check(lib().ptg_multi_accumulate_active(self._h, C.byref(params), int(add_samples)),
              "ptg_multi_accumulate_active")

    def resolve_active(self, image: np.ndarray, params: Params) -> np.ndarray:
        """Each pixel averaged over its own count, written to `image` (float32)."""
        check(lib().ptg_multi_resolve_active(self._h, C.byref(params), self._image(image, params, np.float32)),
              "ptg_multi_resolve_active")
        return image

    def read_sample_counts(self, params: Params) -> np.ndarray:
        """The samples per sub-pixel of every pixel: int32 [H, W], the image's row order."""
        counts = np.zeros((params.height, params.width), dtype=np.int32)
        check(lib().ptg_multi_read_sample_counts(self._h, C.byref(params), counts.ctypes.data_as(C.c_void_p)),
              "ptg_multi_read_sample_counts")
        return counts

    def render_to_noise(self, image: np.ndarray, params: Params, rel_error: float, floor: float = 0.01,
                        max_fraction: float = 0.01, min_samples: int = 16) -> dict:
        """render_to_noise() over all devices (added into `image`, float64):
        the same image and report for any device count and band_rows."""
        target = NoiseTarget(float(rel_error), float(floor), float(max_fraction), int(min_samples), 0)
        rep = NoiseReport()
        check(lib().ptg_multi_render_to_noise(self._h, C.byref(params), C.byref(target),
                                              self._image(image, params, np.float64), C.byref(rep)),
              "ptg_multi_render_to_noise")
        return _noise_report(rep)

    def render_adaptive(self, image: np.ndarray, params: Params, rel_error: float, floor: float = 0.01,
                        max_fraction: float = 0.01, min_samples: int = 16, dilate: int = 1,
                        sample_counts: bool = False):
        """render_adaptive() over all devices (added into `image`, float64):
        the same image, counts and report for any device count, band_rows and
        dilate.  With sample_counts=True returns (report, counts [H, W] int32)."""
        target = AdaptiveTarget(float(rel_error), float(floor), float(max_fraction), int(min_samples), int(dilate))
        rep = AdaptiveReport()
        counts = np.zeros((params.height, params.width), dtype=np.int32) if sample_counts else None
        check(lib().ptg_multi_render_adaptive(self._h, C.byref(params), C.byref(target),
                                              self._image(image, params, np.float64),
                                              counts.ctypes.data_as(C.c_void_p) if sample_counts else None,
                                              C.byref(rep)), "ptg_multi_render_adaptive")
        out = _adaptive_report(rep)
        return (out, counts) if sample_counts else out

    # ---- denoised frames over all devices (ptg_multi_resolve_denoised ... ptg_multi_render_adaptive_denoised):
    # the filtered image equals the one-device driver's bit for bit for any device count, band_rows and dilate
    @staticmethod
    def _dn(denoise):
        return C.byref(denoise) if denoise is not None else None

    def resolve_denoised(self, image: np.ndarray, params: Params, samples_done: int,
                         denoise: Optional[DenoiseParams] = None) -> np.ndarray:
        """The sums of accumulate() passes with FLAG_MOMENTS, resolved at
        samples_done (>= 2) and filtered on the root, written to `image`
        (float32); the sums are kept.  denoise None: the defaults with the
        camera's pixel_spread."""
        check(lib().ptg_multi_resolve_denoised(self._h, C.byref(params), int(samples_done), self._dn(denoise),
                                               self._image(image, params, np.float32)), "ptg_multi_resolve_denoised")
        return image

    def resolve_active_denoised(self, image: np.ndarray, params: Params,
                                denoise: Optional[DenoiseParams] = None) -> np.ndarray:
        """resolve_active() through the filter, its variance from each
        pixel's own count (Context.noise_active); the sums, counts and active
        lists are kept."""
        check(lib().ptg_multi_resolve_active_denoised(self._h, C.byref(params), self._dn(denoise),
                                                      self._image(image, params, np.float32)),
              "ptg_multi_resolve_active_denoised")
        return image

    def render_denoised(self, image: np.ndarray, params: Params, denoise: Optional[DenoiseParams] = None) -> np.ndarray:
        """render_denoised() over all devices (added into `image`, float64)."""
        check(lib().ptg_multi_render_denoised(self._h, C.byref(params), self._dn(denoise),
                                              self._image(image, params, np.float64)), "ptg_multi_render_denoised")
        return image

    def render_to_noise_denoised(self, image: np.ndarray, params: Params, rel_error: float, floor: float = 0.01,
                                 max_fraction: float = 0.01, min_samples: int = 16,
                                 denoise: Optional[DenoiseParams] = None) -> dict:
        """render_to_noise_denoised() over all devices (added into `image`,
        float64); render_to_noise()'s report."""
        target = NoiseTarget(float(rel_error), float(floor), float(max_fraction), int(min_samples), 0)
        rep = NoiseReport()
        check(lib().ptg_multi_render_to_noise_denoised(self._h, C.byref(params), C.byref(target), self._dn(denoise),
                                                       self._image(image, params, np.float64), C.byref(rep)),
              "ptg_multi_render_to_noise_denoised")
        return _noise_report(rep)

    def render_adaptive_denoised(self, image: np.ndarray, params: Params, rel_error: float, floor: float = 0.01,
                                 max_fraction: float = 0.01, min_samples: int = 16, dilate: int = 1,
                                 sample_counts: bool = False, denoise: Optional[DenoiseParams] = None):
        """render_adaptive_denoised() over all devices (added into `image`,
        float64); render_adaptive()'s report (and counts)."""
        target = AdaptiveTarget(float(rel_error), float(floor), float(max_fraction), int(min_samples), int(dilate))
        rep = AdaptiveReport()
        counts = np.zeros((params.height, params.width), dtype=np.int32) if sample_counts else None
        check(lib().ptg_multi_render_adaptive_denoised(self._h, C.byref(params), C.byref(target), self._dn(denoise),
                                                       self._image(image, params, np.float64),
                                                       counts.ctypes.data_as(C.c_void_p) if sample_counts else None,
                                                       C.byref(rep)), "ptg_multi_render_adaptive_denoised")
        out = _adaptive_report(rep)
        return (out, counts) if sample_counts else out


# ptg_render.hip (its launchers fix the block size and the LDS bytes), the seven headers of device code it
# includes by topic and the other csrc files the timed kernels and their launch plan are made of; not ref64.hpp
# (the reference-arithmetic kernel) nor follow_features.hpp (the followed-feature kernel): neither holds a
# timed kernel (tests/test_kernel_sources.py: no file with device code is left out unnoticed)
KERNEL_SOURCES = ("ptg_render.hip", "render_config.hpp", "scan_linear.hpp", "scan_bvh.hpp", "shade.hpp",
                  "render_unit.hpp", "accum_kernels.hpp", "probe_kernels.hpp", "pt_device.hpp", "bvh_build.hpp",
                  "kernel_args.hpp", "scene_prep.hpp", "launch_plan.hpp", "ptg_error.hpp", "sobol_pairs.hpp")


def kernel_source_hash() -> str:
    """sha256 (12 hex digits) of the render kernels' sources (csrc/): names
    the kernel a committed rocprofv3 profile was taken on (profiles/
    summarize.py records it, bench.py compares it with this tree's)."""
    import hashlib
    import os
    h = hashlib.sha256()
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
    for name in KERNEL_SOURCES:
        try:
            with open(os.path.join(src, name), "rb") as f:
                h.update(f.read())
        except OSError:
            return "unavailable"
    return h.hexdigest()[:12]


def pci_bus_id(device: int) -> str:
    """ptg_device_pci_bus_id: the PCI bus id of HIP device `device`."""
    buf = C.create_string_buffer(64)
    check(lib().ptg_device_pci_bus_id(int(device), buf, len(buf)), "ptg_device_pci_bus_id")
    return buf.value.decode()


def scene_layout(scn, cam):
    """Host-side scene preparation (ptg_scene_layout, no device needed): the
    anchor axis of each huge sphere (-1: camera-facing anchor, or not huge)
    and the linear scan order (scene indices in the order they are tested)."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    n = len(sp)
    axis = np.zeros(max(n, 1), dtype=np.int32)
    order = np.zeros(max(n, 1), dtype=np.int32)
    check(lib().ptg_scene_layout(sp.ctypes.data, n, ca.ctypes.data, axis.ctypes.data, order.ctypes.data),
          "ptg_scene_layout")
    return axis[:n].tolist(), order[:n].tolist()


def light_list(scn, cam):
    """FLAG_LIGHT_SAMPLING's light list (ptg_light_list, no device needed):
    the scene indices of the emissive spheres that are not huge, ascending.
    More than MAX_LIGHTS of them raises PtgError (PTG_ERR_UNSUPPORTED), as
    rendering the scene with the flag does."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    ids = np.zeros(MAX_LIGHTS, dtype=np.int32)
    n = C.c_int(0)
    check(lib().ptg_light_list(sp.ctypes.data, len(sp), ca.ctypes.data, ids.ctypes.data, MAX_LIGHTS, C.byref(n)),
          "ptg_light_list")
    return ids[:n.value].tolist()


class Context:
    """A scene prepared in HBM on one device (ptg_context)."""

    def __init__(self, scn, cam, device: Optional[int] = None):
        sp = _spheres_array(scn)
        ca = _camera_array(cam)
        h = C.c_void_p()
        check(lib().ptg_context_create(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                       -1 if device is None else int(device), C.byref(h)), "ptg_context_create")
        self._h = h
        self.n_spheres = len(sp)
        if device is None or int(device) < 0:
            import torch
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.device = int(device)

    def _stream(self, stream):
        """The HIP stream handle: `stream`, or torch's current stream on the
        context's device (not the current device)."""
        import torch
        return (stream or torch.cuda.current_stream(torch.device("cuda", self.device))).cuda_stream

    def _check(self, t, dtype, min_numel):
        _check_tensor(t, dtype, min_numel)
        if t.device.index != self.device:
            raise ValueError(f"tensor on {t.device}, context on cuda:{self.device}")

    def close(self):
        if self._h:
            lib().ptg_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def render_device(self, out, params: Params, segments=None, stream=None) -> None:
        """Asynchronous render into `out` (torch float32 CUDA tensor of
        shard_rows*W*3 values) on `stream` (torch.cuda.Stream or None =
        torch's current stream)."""
        import torch
        self._check(out, torch.float32, shard_rows(params.height, params.band_rows, params.shard_count)
                    * params.width * 3)
        if segments is not None:
            self._check(segments, torch.int64, _n_counters(params.flags))
        s = self._stream(stream)
        check(lib().ptg_render_device(self._h, C.byref(params), C.c_void_p(out.data_ptr()),
                                      C.c_void_p(segments.data_ptr()) if segments is not None else None,
                                      C.c_void_p(s)), "ptg_render_device")

    LAUNCH_INFO = ("box_mode", "box_walls_out", "bvh", "units", "workgroups", "levels", "resolve_pass",
                   "wall_pairs")  # include/ptgpu.h ptg_launch_info

    def launch_info(self, params: Params) -> dict:
        """ptg_launch_info: how ptg_render_device would launch this frame
        (scan mode, work units, levels) -- host-side, nothing is launched."""
        v = np.zeros(len(self.LAUNCH_INFO), dtype=np.int64)
        check(lib().ptg_launch_info(self._h, C.byref(params), v.ctypes.data_as(C.c_void_p), len(v)),
              "ptg_launch_info")
        return dict(zip(self.LAUNCH_INFO, (int(x) for x in v)))

    # ---- progressive accumulation (ptg_accumulate_device / ptg_resolve_device)
    def reset_accumulation(self, params: Params, stream=None) -> None:
        s = self._stream(stream)
        check(lib().ptg_reset_accumulation_device(self._h, C.byref(params), C.c_void_p(s)), "ptg_reset_accumulation_device")

    def accumulate(self, params: Params, sample_begin: int, sample_end: int, segments=None, stream=None) -> None:
        """Add samples [sample_begin, sample_end) of every sub-pixel."""
        import torch
        if segments is not None:
            self._check(segments, torch.int64, _n_counters(params.flags))
        s = self._stream(stream)
        check(lib().ptg_accumulate_device(self._h, C.byref(params), int(sample_begin), int(sample_end),
                                          C.c_void_p(segments.data_ptr()) if segments is not None else None,
                                          C.c_void_p(s)), "ptg_accumulate_device")

    def resolve(self, out, params: Params, samples_done: int, stream=None) -> None:
        """Preview/final image from the samples accumulated so far."""
        import torch
        self._check(out, torch.float32, shard_rows(params.height, params.band_rows, params.shard_count)
                    * params.width * 3)
        s = self._stream(stream)
        check(lib().ptg_resolve_device(self._h, C.byref(params), int(samples_done), C.c_void_p(out.data_ptr()),
                                       C.c_void_p(s)), "ptg_resolve_device")

    # ---- per-pixel noise estimates (ptg_noise_device, after FLAG_MOMENTS passes)
    def noise(self, params: Params, samples_done: int, rel_error: float, floor: float, var=None, rho=None,
              stats=None, stream=None) -> None:
        """Noise of the samples accumulated so far: `var` (float32, slab
        rows*W*3: variance of every pixel value), `rho` (float32, slab rows*W:
        relative standard error) and `stats` (int64 [4], zeroed by the caller:
        += pixels with rho > rel_error, += fixed-point sum of rho, max of
        rho's bits, += pixels), each optional."""
        import torch
        pixels = shard_rows(params.height, params.band_rows, params.shard_count) * params.width
        if var is not None:
            self._check(var, torch.float32, pixels * 3)
        if rho is not None:
            self._check(rho, torch.float32, pixels)
        if stats is not None:
            self._check(stats, torch.int64, 4)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        s = self._stream(stream)
        check(lib().ptg_noise_device(self._h, C.byref(params), int(samples_done), float(rel_error), float(floor),
                                     ptr(var), ptr(rho), ptr(stats), C.c_void_p(s)), "ptg_noise_device")

    def read_moments(self, params: Params, sums=None, sumsq=None, stream=None) -> None:
        """The raw exact sums (int64 tensors of slab rows*W*nsub^2*3 values,
        index ((row*W + x)*nsub^2 + sub)*3 + c): `sums` of q(c), `sumsq` of
        q(cl(c)^2) (after FLAG_MOMENTS passes only)."""
        import torch
        n = (shard_rows(params.height, params.band_rows, params.shard_count) * params.width
             * params.num_subpixels ** 2 * 3)
        for t in (sums, sumsq):
            if t is not None:
                self._check(t, torch.int64, n)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        s = self._stream(stream)
        check(lib().ptg_read_moments_device(self._h, C.byref(params), ptr(sums), ptr(sumsq), C.c_void_p(s)),
              "ptg_read_moments_device")

    # ---- adaptive sampling (ptg_*_active_device): later passes only where the image is still noisy
    def _pixels(self, params: Params) -> int:
        return shard_rows(params.height, params.band_rows, params.shard_count) * params.width

    def set_active_mask(self, params: Params, mask=None, info=None, stream=None) -> None:
        """The active list from `mask` (uint8, slab rows*W: != 0 is active;
        None: every pixel of the image).  `info` (int64 [2], optional)
        receives the active pixels and the active work units."""
        import torch
        if mask is not None:
            self._check(mask, torch.uint8, self._pixels(params))
        if info is not None:
            self._check(info, torch.int64, 2)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().ptg_set_active_mask_device(self._h, C.byref(params), ptr(mask), ptr(info),
                                               C.c_void_p(self._stream(stream))), "ptg_set_active_mask_device")

    def select_active(self, params: Params, rel_error: float, floor: float, dilate: int = 0, rho=None, stats=None,
                      stream=None) -> None:
        """The active list from the noise of the samples so far, each pixel
        with its own count: active = within `dilate` pixels of a pixel whose
        rho > rel_error.  `rho` (float32, slab rows*W) and `stats` (int64 [6],
        zeroed by the caller: noise()'s four, += active pixels, += active
        units) are optional."""
        import torch
        if rho is not None:
            self._check(rho, torch.float32, self._pixels(params))
        if stats is not None:
            self._check(stats, torch.int64, 6)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().ptg_select_active_device(self._h, C.byref(params), float(rel_error), float(floor), int(dilate),
                                             ptr(rho), ptr(stats), C.c_void_p(self._stream(stream))),
              "ptg_select_active_device")

    def select_over(self, params: Params, rel_error: float, floor: float, over, rho=None, stats=None,
                    stream=None) -> None:
        """select_active's first step alone: this shard's over bytes to `over`
        (uint8, slab rows*W: 1 where rho > rel_error), `rho` and `stats`
        [0..3] (int64 [6]) as there; no list is built."""
        import torch
        self._check(over, torch.uint8, self._pixels(params))
        if rho is not None:
            self._check(rho, torch.float32, self._pixels(params))
        if stats is not None:
            self._check(stats, torch.int64, 6)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().ptg_select_over_device(self._h, C.byref(params), float(rel_error), float(floor), ptr(over),
                                           ptr(rho), ptr(stats), C.c_void_p(self._stream(stream))),
              "ptg_select_over_device")

    def set_active_gathered(self, params: Params, over_gathered, dilate: int = 0, stats=None, stream=None) -> None:
        """This shard's active list from the over bytes of the whole frame:
        `over_gathered` (uint8) holds shard_count slabs of slab rows*W bytes,
        rank-major (what an all-gather of select_over's slabs gives); active =
        within `dilate` pixels of a set byte, across shard boundaries.  `stats`
        (int64 [6], optional): [4] += active pixels, [5] += active units."""
        import torch
        self._check(over_gathered, torch.uint8, self._pixels(params) * params.shard_count)
        if stats is not None:
            self._check(stats, torch.int64, 6)
        check(lib().ptg_set_active_gathered_device(self._h, C.byref(params), C.c_void_p(over_gathered.data_ptr()),
                                                   int(dilate),
                                                   C.c_void_p(stats.data_ptr()) if stats is not None else None,
                                                   C.c_void_p(self._stream(stream))),
              "ptg_set_active_gathered_device")

    def accumulate_active(self, params: Params, add_samples: int, max_units: int = 0, segments=None,
                          stream=None) -> None:
        """The next `add_samples` samples of every pixel of the active list
        (max_units: the unit count read back from stats[5] / info[1], or 0)."""
        import torch
        if segments is not None:
            self._check(segments, torch.int64, _n_counters(params.flags))
        check(lib().ptg_accumulate_active_device(self._h, C.byref(params), int(add_samples), int(max_units),
                                                 C.c_void_p(segments.data_ptr()) if segments is not None else None,
                                                 C.c_void_p(self._stream(stream))), "ptg_accumulate_active_device")

    def resolve_active(self, out, params: Params, stream=None) -> None:
        """The image of the samples so far, each pixel averaged over its own count."""
        import torch
        self._check(out, torch.float32, self._pixels(params) * 3)
        check(lib().ptg_resolve_active_device(self._h, C.byref(params), C.c_void_p(out.data_ptr()),
                                              C.c_void_p(self._stream(stream))), "ptg_resolve_active_device")

    def read_sample_counts(self, params: Params, counts, stream=None) -> None:
        """The samples per sub-pixel every pixel holds (int32, slab rows*W)."""
        import torch
        self._check(counts, torch.int32, self._pixels(params))
        check(lib().ptg_read_sample_counts_device(self._h, C.byref(params), C.c_void_p(counts.data_ptr()),
                                                  C.c_void_p(self._stream(stream))), "ptg_read_sample_counts_device")

    def noise_active(self, params: Params, floor: float, var=None, rho=None, stream=None) -> None:
        """noise()'s `var` and `rho` with each pixel's own sample count (the
        guide of denoise() for an adaptive frame); a pixel with fewer than 2
        samples gets rho = +inf and the variance of the clamp's bound, 1 / (4
        num_subpixels^2) per channel.  The sums, counts and list are kept."""
        import torch
        if var is not None:
            self._check(var, torch.float32, self._pixels(params) * 3)
        if rho is not None:
            self._check(rho, torch.float32, self._pixels(params))
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().ptg_noise_active_device(self._h, C.byref(params), float(floor), ptr(var), ptr(rho),
                                            C.c_void_p(self._stream(stream))), "ptg_noise_active_device")

    # ---- denoising (ptg_features_device; the filter itself needs no context: denoise())
    def features(self, params: Params, out=None, stream=None, *, follow_bounces: Optional[int] = None):
        """The first-hit features of every slab pixel (float32, slab rows*W*12:
        {n.xyz, z}, {P.xyz, hit}, {albedo.rgb, 0}), the guide of denoise().
        Deterministic camera rays through the renderer's exact scan: no
        dependence on seed, samples or flags.  Returns `out` ([rows, W, 12]
        when allocated here).  follow_bounces (keyword; None or 0..16):
        ptg_features_follow_device -- each ray followed through at most that
        many mirror and glass surfaces to the first diffuse one, word 11 the
        mean number of bounces; None is ptg_features_device, which 0 equals
        bit for bit."""
        import torch
        rows = shard_rows(params.height, params.band_rows, params.shard_count)
        if out is None:
            out = torch.zeros((rows, params.width, 12), dtype=torch.float32, device=torch.device("cuda", self.device))
        self._check(out, torch.float32, rows * params.width * 12)
        if follow_bounces is not None:
            check(lib().ptg_features_follow_device(self._h, C.byref(params), int(follow_bounces),
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(self._stream(stream))),
                  "ptg_features_follow_device")
            return out
        check(lib().ptg_features_device(self._h, C.byref(params), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(self._stream(stream))), "ptg_features_device")
        return out

    def trace_samples(self, coords, params: Params):
        """Parity probe: radiance + segment count of individual paths
        (coords: int32 CUDA tensor [n, 5] = x, y, sx, sy, sample)."""
        import torch
        if coords.dim() != 2 or coords.shape[1] != 5:
            raise ValueError("coords must be [n, 5] (x, y, sx, sy, sample)")
        coords = coords.contiguous()
        self._check(coords, torch.int32, coords.numel())
        n = coords.shape[0]
        out = torch.empty((n, 3), dtype=torch.float32, device=coords.device)
        segs = torch.empty((n,), dtype=torch.int32, device=coords.device)
        s = self._stream(None)
        check(lib().ptg_trace_samples_device(self._h, C.byref(params), C.c_void_p(coords.data_ptr()), n,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(segs.data_ptr()),
                                             C.c_void_p(s)), "ptg_trace_samples_device")
        return out, segs

    def sampler_pairs(self, coords, params: Params):
        """FLAG_STRATIFIED's pairs 0..3 of individual paths (coords: int32
        CUDA tensor [n, 5] = x, y, sx, sy, sample) -> int32 [n, 4, 2], the
        24-bit integers (m0, m1) of each pair (ptg_sampler_pairs_device)."""
        import torch
        if coords.dim() != 2 or coords.shape[1] != 5:
            raise ValueError("coords must be [n, 5] (x, y, sx, sy, sample)")
        coords = coords.contiguous()
        self._check(coords, torch.int32, coords.numel())
        n = coords.shape[0]
        out = torch.empty((n, 4, 2), dtype=torch.int32, device=coords.device)
        check(lib().ptg_sampler_pairs_device(self._h, C.byref(params), C.c_void_p(coords.data_ptr()), n,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(self._stream(None))),
              "ptg_sampler_pairs_device")
        return out

    PROBE_OPS = {"sqrt": 0, "rsqrt": 1, "div": 2, "sincos": 3}  # include/ptgpu.h PTG_PROBE_*

    def math_probe(self, op: str, x, exact: bool):
        """The kernels' arithmetic primitive `op` on a float32 CUDA tensor:
        sqrt / rsqrt of x [n]; div of x [n, 2] (x[:, 0] / x[:, 1]); sincos of
        24-bit integers m (x: int32 [n]) -> [n, 2] (cos, sin of 2 pi m 2^-24)."""
        import torch
        code = self.PROBE_OPS[op]
        x = x.contiguous()
        if op == "div":
            if x.dim() != 2 or x.shape[1] != 2:
                raise ValueError("div takes [n, 2] operands")
            n = x.shape[0]
        else:
            n = x.numel()
        if op == "sincos":
            self._check(x, torch.int32, n)
            x = x.view(torch.float32)
        else:
            self._check(x, torch.float32, x.numel())
        out = torch.empty((n, 2) if op == "sincos" else (n,), dtype=torch.float32, device=x.device)
        s = self._stream(None)
        check(lib().ptg_math_probe_device(self._h, code, 1 if exact else 0, C.c_void_p(x.data_ptr()),
                                          C.c_void_p(out.data_ptr()), n, C.c_void_p(s)), "ptg_math_probe_device")
        return out


def _check_tensor(t, dtype, min_numel):
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() < min_numel:
        raise ValueError(f"expected a contiguous CUDA {dtype} tensor with >= {min_numel} elements")


def denoise_defaults() -> DenoiseParams:
    """ptg_denoise_defaults (host only).  pixel_spread is a generic 1/1024:
    set it from pixel_spread(cam, width, height)."""
    k = DenoiseParams()
    check(lib().ptg_denoise_defaults(C.byref(k)), "ptg_denoise_defaults")
    return k


def pixel_spread(cam, width: int, height: int) -> float:
    """ptg_pixel_spread (host only): the world size of a pixel at distance 1."""
    ca = _camera_array(cam)
    v = C.c_float(0.0)
    check(lib().ptg_pixel_spread(ca.ctypes.data_as(C.c_void_p), int(width), int(height), C.byref(v)),
          "ptg_pixel_spread")
    return v.value


def denoise_scratch_bytes(width: int, height: int) -> int:
    n = C.c_size_t(0)
    check(lib().ptg_denoise_scratch_bytes(int(width), int(height), C.byref(n)), "ptg_denoise_scratch_bytes")
    return n.value


def denoise(color, var, feat, params: Optional[DenoiseParams] = None, var_out: bool = False, scratch=None,
            stream=None, kernel_: int = 0):
    """ptg_denoise_device on whole frames held as torch CUDA tensors: color
    and var [H, W, 3] float32 (Context.resolve / Context.noise of a
    shard_count = 1 slab cut to its H rows, or a gathered frame), feat
    [H, W, 12] (Context.features).  Returns the filtered colour, or (colour,
    variance) with var_out=True.  `scratch`: a float32 tensor of at least
    denoise_scratch_bytes(W, H) bytes to reuse (allocated here otherwise; the
    call itself allocates nothing).  Asynchronous on `stream`.  kernel_ (tests
    and tools): 1 runs the plain filter kernel at every step instead of the
    tiled one where its tile fits; the result is the same bit for bit."""
    import torch
    if color.dim() != 3 or color.shape[2] != 3:
        raise ValueError("color must be [H, W, 3]")
    H, W = int(color.shape[0]), int(color.shape[1])
    _check_tensor(color, torch.float32, H * W * 3)
    for t, n in ((var, 3), (feat, 12)):
        _check_tensor(t, torch.float32, H * W * n)
        if t.device != color.device or t.numel() != H * W * n:
            raise ValueError("var must be [H, W, 3] and feat [H, W, 12] on color's device")
    k = params if params is not None else denoise_defaults()
    need = denoise_scratch_bytes(W, H)
    if scratch is None:
        scratch = torch.empty(need // 4, dtype=torch.float32, device=color.device)
    _check_tensor(scratch, torch.float32, 0)
    out = torch.empty_like(color)
    vout = torch.empty_like(color) if var_out else None
    s = (stream or torch.cuda.current_stream(color.device)).cuda_stream
    with torch.cuda.device(color.device):
        args = (C.c_void_p(color.data_ptr()), C.c_void_p(var.data_ptr()), C.c_void_p(feat.data_ptr()), W, H,
                C.byref(k), C.c_void_p(out.data_ptr()), C.c_void_p(vout.data_ptr()) if var_out else None,
                C.c_void_p(scratch.data_ptr()), scratch.numel() * 4, C.c_void_p(s))
        if kernel_:
            check(lib().ptg_denoise_device_kernel_(*args, int(kernel_)), "ptg_denoise_device_kernel_")
        else:
            check(lib().ptg_denoise_device(*args), "ptg_denoise_device")
    return (out, vout) if var_out else out


def denoise_host(color: np.ndarray, var: np.ndarray, feat: np.ndarray, params: Optional[DenoiseParams] = None,
                 var_out: bool = False):
    """ptg_denoise_host: the filter's CPU statement on numpy arrays ([H, W, 3],
    [H, W, 3], [H, W, 12] float32) -- the same arithmetic, bit for bit."""
    color = np.ascontiguousarray(color, dtype=np.float32)
    var = np.ascontiguousarray(var, dtype=np.float32)
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    H, W = color.shape[:2]
    if color.shape != (H, W, 3) or var.shape != (H, W, 3) or feat.shape != (H, W, 12):
        raise ValueError("color and var must be [H, W, 3], feat [H, W, 12]")
    k = params if params is not None else denoise_defaults()
    out = np.empty_like(color)
    vout = np.empty_like(color) if var_out else None
    check(lib().ptg_denoise_host(color.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p),
                                 feat.ctypes.data_as(C.c_void_p), W, H, C.byref(k), out.ctypes.data_as(C.c_void_p),
                                 vout.ctypes.data_as(C.c_void_p) if var_out else None), "ptg_denoise_host")
    return (out, vout) if var_out else out


def render_denoised(scn, cam, image: np.ndarray, width: int, height: int, samples: int, num_subpixels: int = 2,
                    seed: int = DEFAULT_SEED, device: int = -1, flags: int = 0,
                    params: Optional[DenoiseParams] = None) -> np.ndarray:
    """ptg_render_denoised: render() at `samples` (>= 2) with the moments
    kept, then the filter guided by the frame's variance and first-hit
    features; added into `image` like render().  params None: the defaults
    with the camera's pixel_spread."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    if image.dtype != np.float64 or not image.flags["C_CONTIGUOUS"] or image.size != width * height * 3:
        raise ValueError("image must be a C-contiguous float64 array of width*height*3 values")
    p = make_params(width, height, samples, num_subpixels, seed, flags=flags)
    check(lib().ptg_render_denoised(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                    C.byref(p), int(device), C.byref(params) if params is not None else None,
                                    image.ctypes.data_as(C.c_void_p)), "ptg_render_denoised")
    return image


def render_to_noise_denoised(scn, cam, image: np.ndarray, width: int, height: int, samples: int, rel_error: float,
                             floor: float = 0.01, max_fraction: float = 0.01, min_samples: int = 16,
                             num_subpixels: int = 2, seed: int = DEFAULT_SEED, device: int = -1, flags: int = 0,
                             params: Optional[DenoiseParams] = None) -> dict:
    """ptg_render_to_noise_denoised: render_to_noise() whose frame, at the
    samples it stopped at, goes through the filter (its passes carry the
    moments: nothing is rendered twice).  Returns render_to_noise()'s report."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    if image.dtype != np.float64 or not image.flags["C_CONTIGUOUS"] or image.size != width * height * 3:
        raise ValueError("image must be a C-contiguous float64 array of width*height*3 values")
    p = make_params(width, height, samples, num_subpixels, seed, flags=flags)
    target = NoiseTarget(float(rel_error), float(floor), float(max_fraction), int(min_samples), 0)
    rep = NoiseReport()
    check(lib().ptg_render_to_noise_denoised(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                             C.byref(p), int(device), C.byref(target),
                                             C.byref(params) if params is not None else None,
                                             image.ctypes.data_as(C.c_void_p), C.byref(rep)),
          "ptg_render_to_noise_denoised")
    return _noise_report(rep)


def render_adaptive_denoised(scn, cam, image: np.ndarray, width: int, height: int, samples: int, rel_error: float,
                             floor: float = 0.01, max_fraction: float = 0.01, min_samples: int = 16, dilate: int = 1,
                             num_subpixels: int = 2, seed: int = DEFAULT_SEED, device: int = -1, flags: int = 0,
                             sample_counts: bool = False, params: Optional[DenoiseParams] = None):
    """ptg_render_adaptive_denoised: render_adaptive() whose frame goes
    through the filter, guided by the variance of each pixel at its own sample
    count (Context.noise_active).  Returns render_adaptive()'s report, or
    (report, counts) with sample_counts=True."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    if image.dtype != np.float64 or not image.flags["C_CONTIGUOUS"] or image.size != width * height * 3:
        raise ValueError("image must be a C-contiguous float64 array of width*height*3 values")
    p = make_params(width, height, samples, num_subpixels, seed, flags=flags)
    target = AdaptiveTarget(float(rel_error), float(floor), float(max_fraction), int(min_samples), int(dilate))
    rep = AdaptiveReport()
    counts = np.zeros((height, width), dtype=np.int32) if sample_counts else None
    check(lib().ptg_render_adaptive_denoised(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                             C.byref(p), int(device), C.byref(target),
                                             C.byref(params) if params is not None else None,
                                             image.ctypes.data_as(C.c_void_p),
                                             counts.ctypes.data_as(C.c_void_p) if sample_counts else None,
                                             C.byref(rep)), "ptg_render_adaptive_denoised")
    out = _adaptive_report(rep)
    return (out, counts) if sample_counts else out


def features(scn, cam, width: int, height: int, num_subpixels: int = 2, device: int = -1,
             follow_bounces: int = 0) -> np.ndarray:
    """ptg_features: the first-hit feature frame on the host, float32
    [height, width, 12] in render()'s row order.  follow_bounces 1..16:
    ptg_features_follow, the first diffuse hit behind mirrors and glass."""
    sp = _spheres_array(scn)
    ca = _camera_array(cam)
    out = np.zeros((height, width, 12), dtype=np.float32)
    p = make_params(width, height, 1, num_subpixels)
    if follow_bounces:
        check(lib().ptg_features_follow(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                        C.byref(p), int(device), int(follow_bounces),
                                        out.ctypes.data_as(C.c_void_p)), "ptg_features_follow")
        return out
    check(lib().ptg_features(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p), C.byref(p),
                             int(device), out.ctypes.data_as(C.c_void_p)), "ptg_features")
    return out


def unshard_device(gathered, image, width, height, band_rows, shard_count, stream=None):
    import torch
    s = (stream or torch.cuda.current_stream(image.device)).cuda_stream
    check(lib().ptg_unshard_device(C.c_void_p(gathered.data_ptr()), C.c_void_p(image.data_ptr()), width, height,
                                   band_rows, shard_count, C.c_void_p(s)), "ptg_unshard_device")


def tonemap_device(image, out_u8, stream=None):
    """utils.cpp:11-16 on the GPU: uint8 gamma-2.2 values of every channel."""
    import torch
    s = (stream or torch.cuda.current_stream(image.device)).cuda_stream
    check(lib().ptg_tonemap_device(C.c_void_p(image.data_ptr()), C.c_void_p(out_u8.data_ptr()), image.numel(),
                                   C.c_void_p(s)), "ptg_tonemap_device")


def render_sharded(params: Params, slab, group=None,
                   tile_renderer: Optional[Callable] = None, ctx: Optional[Context] = None,
                   unshard: Optional[Callable] = None):
    """One rank's part of a tile-sharded frame.

    Renders this rank's bands into `slab`, then ONE gather collects every
    slab on rank 0 (torch.distributed: RCCL over xGMI on the nccl backend,
    gloo on CPU).  Rank 0 returns the reassembled image tensor [H, W, 3];
    other ranks return None.  `tile_renderer(slab, params)` defaults to the
    HIP megakernel (ctx.render_device); tests substitute a CPU renderer to
    exercise the sharding logic with gloo."""
    import torch
    import torch.distributed as dist
    if tile_renderer is None:
        if ctx is None:
            raise ValueError("render_sharded needs ctx (HIP path) or tile_renderer")
        tile_renderer = lambda out, p: ctx.render_device(out, p)  # noqa: E731
    tile_renderer(slab, params)
    rank = dist.get_rank(group)
    world = dist.get_world_size(group)
    assert params.shard_count == world and params.shard_rank == rank
    # gloo cannot gather device tensors: stage through host memory (CPU
    # rehearsals only; the nccl backend (RCCL) gathers HBM to HBM over xGMI)
    staged = slab.is_cuda and dist.get_backend(group) == "gloo"
    send = slab.cpu() if staged else slab
    if rank == 0:
        gathered = torch.empty((world,) + tuple(send.shape), dtype=send.dtype, device=send.device)
        dist.gather(send, gather_list=list(gathered.unbind(0)), dst=0, group=group)
        if staged:
            gathered = gathered.to(slab.device)
        image = torch.empty((params.height, params.width, 3), dtype=slab.dtype, device=slab.device)
        if unshard is not None:
            unshard(gathered, image, params)
        elif slab.is_cuda:
            unshard_device(gathered, image, params.width, params.height, params.band_rows, world)
        else:
            image.copy_(torch.from_numpy(unshard_host(gathered.numpy(), params.width, params.height,
                                                       params.band_rows, world)))
        return image
    dist.gather(send, gather_list=None, dst=0, group=group)
    return None
