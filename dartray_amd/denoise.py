"""The edge-avoiding a-trous denoiser (dr_denoise_atrous*): a post-process beside the render path, guided by the
images of the first-hit feature integrator.

    atrous(rgb, normal, depth, ...)          filters one image
    render_denoised(renderer, scene, ...)    renders the beauty image and its two guides, and filters

and its variance-guided form over two half-sample renders (dr_denoise_pair*):

    atrous_pair(a, b, normal, depth, ...)         filters the mean of two renders, guided by the variance their difference estimates
    render_denoised_pair(renderer, scene, ...)    renders the two halves and the two guides, and filters

and the joint bilateral upsampler that lets a render trace 1/4 or 1/16 of the camera pixels (dr_upsample*):

    upsample(rgb_lo, normal_lo, depth_lo, normal, depth, ...)    a low-resolution image becomes a full-resolution one under full-resolution guides
    render_upsampled(low_renderer, full_renderer, scene, ...)    renders the low-resolution image and both sets of guides, and upsamples

and temporal accumulation with reprojection for the frames of a camera animation (dr_temporal*):

    temporal_matrices(camera, prev_camera)                       the three f64 matrices that take a pixel to the previous frame's raster
    temporal(rgb, normal, depth, history, matrices, ...)         blends one frame into the history of the frames before it
    render_sequence(renderers, scene, ...)                       renders one frame per camera pose and accumulates them

and the variance-guided filter fed by that history's luminance moments (dr_denoise_moments*):

    atrous_moments(frame, ...)                                   filters a TemporalFrame's colour, guided by the variance its moments estimate
    render_sequence(renderers, scene, denoise="moments", ...)    ... on every frame of a sequence

and firefly suppression, the outlier clamp that runs ahead of all of them (dr_firefly*):

    firefly(rgb, normal, depth, ...)                             scales a pixel far brighter than its same-surface neighbours down to their level
    render_firefly(renderer, scene, ...)                         renders the beauty image and its two guides, and clamps
    render_denoised / _pair / render_upsampled / render_sequence(..., firefly=True)    ... ahead of the filter, the upsampler, the history

and demodulation, which takes what is known without noise out of the beauty image before all of them and puts it back after the last
(dr_demodulate*, dr_remodulate*; the images are core.MaterialIntegrator's):

    demodulate(rgb, emission, albedo, ...)                       max(0, rgb - emission) / (albedo + eps)
    remodulate(rgb, emission, albedo, ...)                       rgb * (albedo + eps) + emission
    render_denoised / _pair / render_sequence(..., demodulate=True)    ... around the filter: the emitters' pixels are never filtered

The library takes sharpness values k = 1 / sigma^2 (k = 0: the term is off); this module takes the sigmas.
"""
import copy
import ctypes as C
import math

import numpy as np

from . import _abi
from ._image import _beauty_and_guides, _check_channel, _check_one_pass, _entry, _guides, _images, _rerender, _whole_film_refusals
from .core.cameras import PerspectiveCamera
from .core.renderer import FeatureIntegrator, MaterialIntegrator, OutputImage, SamplerRenderer  # noqa: F401  (the first and last: read from here by tools/)
from .core.samplers import AdaptiveSampler

# The defaults: five levels reach 2 * 16 pixels to either side; the colour sigma is one unit of radiance at the first
# level (a diffuse surface's radiance in the BASELINE scenes is of that order) and halves per level; the normal term halves a tap's
# weight at about 11 degrees between the normals (the guide is 0.5 * (n + 1): |dn|^2 / 4 = 0.01 there); the depth sigma is one scene unit.
ITERATIONS = 5
SIGMA_COLOR = 1.0
SIGMA_NORMAL = 0.1
SIGMA_DEPTH = 1.0
# The pair filter's own two.  Its colour sigma has no unit: a luminance difference is measured in standard deviations of
# the local noise, and a tap four of them away has half its weight (SVGF's sigma_l = 4).  The variance floor is the square of 0.01, one
# hundredth of a lit diffuse surface's radiance in the BASELINE scenes: where both halves agree the one-sample estimate is exactly 0, and
# the floor is what a difference is then measured against.
SIGMA_COLOR_PAIR = 4.0
VAR_FLOOR = 1.0e-4
SEED_B_XOR = 0x2545F491


def sharpness(sigma):
    """k = 1 / sigma^2 as the f32 the library takes; an infinite sigma gives 0, which switches the term off."""
    sigma = float(sigma)
    if math.isnan(sigma) or sigma <= 0.0:
        raise ValueError("denoise: a sigma must be positive (inf switches the term off), got %r" % (sigma,))
    return 0.0 if math.isinf(sigma) else float(np.float32(1.0 / (sigma * sigma)))


def params(iterations=ITERATIONS, sigma_color=SIGMA_COLOR, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH):
    return _abi.DrDenoiseParams(int(iterations), sharpness(sigma_color), sharpness(sigma_normal), sharpness(sigma_depth))


def atrous(rgb, normal, depth, iterations=ITERATIONS, sigma_color=SIGMA_COLOR, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH,
           device=True):
    """rgb [h, w, 3], normal [h, w, 3], depth [h, w] -> the filtered [h, w, 3] f32.  device=True: dr_denoise_atrous, on the GPU;
    device=False: dr_denoise_atrous_host, which needs none and writes the same bytes."""
    rgb, normal, depth = _images("denoise", "rgb and normal must be [h, w, 3] and depth [h, w]", (rgb, normal), depth)
    h, w = depth.shape
    p = params(iterations, sigma_color, sigma_normal, sigma_depth)
    out = np.zeros_like(rgb)
    _abi.check(_entry("dr_denoise_atrous", device)(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data))
    return out


def render_denoised(renderer, scene, normal_channel="ns", firefly=False, one_pass=False, demodulate=False, **filter_kw):
    """Renders the beauty image with `renderer` as given and two FeatureIntegrator images -- `normal_channel` ("ns" or "ng") and "depth" --
    with the same camera, film, sampler and work split, filters, and returns an OutputImage whose rgb is the result; the three unfiltered
    images stay on it as `noisy` [h, w, 3], `normal` [h, w, 3] and `depth` [h, w].  filter_kw: atrous()'s keywords.  firefly: True, or a
    dict of firefly()'s parameters, clamps the beauty image's outliers before the filter; `noisy` stays the unclamped
    render and the luminance taken away stays on the result as `removed`.  one_pass=True: the beauty image and both guides come from one
    render (render_with_guides) instead of three, the same bytes; an integrator it does not serve raises ValueError.
    demodulate: True, or a tuple of "emission" and / or "albedo", renders those MaterialIntegrator images with the renderer's own sampler and
    work split, takes them out of the beauty image before every other stage, the firefly clamp included, and puts them back after the filter
    (DESIGN.md 2.27); the images stay on the result as `emission` / `albedo`, the demodulated render as `demodulated`.  It runs where the
    filter runs (filter_kw's `device`).  It cannot be combined with one_pass."""
    _check_channel("render_denoised", normal_channel)
    fkw = _firefly_kw("render_denoised", firefly)
    dm = _demodulate_kw("render_denoised", demodulate, one_pass)
    if isinstance(renderer.sampler, AdaptiveSampler):
        raise ValueError("render_denoised: the adaptive sampler is not supported (the feature integrator refuses it)")
    _check_one_pass("render_denoised", one_pass, renderer, scene, normal_channel)
    beauty, normal, depth = _beauty_and_guides(renderer, scene, normal_channel, one_pass)
    mats = _material_images(renderer, scene, dm)
    on_device = filter_kw.get("device", True)
    base = _demodulated(dm, mats, beauty.rgb, on_device)
    clamped, removed = _clamped(fkw, base, normal, depth)
    rgb = _remodulated(dm, mats, atrous(clamped, normal, depth, **filter_kw), on_device)
    out = OutputImage(beauty.xOffset, beauty.yOffset, beauty.width, beauty.height, rgb, beauty.film)
    out.noisy, out.normal, out.depth = beauty.rgb, normal, depth
    if fkw is not None:
        out.removed = removed
    if dm is not None:
        _keep_material(out, mats, base)
    return out


def pair_params(iterations=ITERATIONS, sigma_color=SIGMA_COLOR_PAIR, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH, var_floor=VAR_FLOOR):
    return _abi.DrDenoisePairParams(int(iterations), sharpness(sigma_color), sharpness(sigma_normal), sharpness(sigma_depth), float(var_floor))


def atrous_pair(a, b, normal, depth, iterations=ITERATIONS, sigma_color=SIGMA_COLOR_PAIR, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH,
                var_floor=VAR_FLOOR, device=True, return_variance=False):
    """a [h, w, 3] and b [h, w, 3], two renders of one scene that differ in the sampler's seed alone, normal [h, w, 3], depth [h, w] -> their
    mean, filtered, [h, w, 3] f32; with return_variance=True also the variance [h, w] the last level leaves (-1: the pixel is not valid).
    sigma_color is in standard deviations of the local noise.  device=True: dr_denoise_pair, on the GPU; device=False:
    dr_denoise_pair_host, which needs none and writes the same bytes."""
    a, b, normal, depth = _images("denoise", "a, b and normal must be [h, w, 3] and depth [h, w]", (a, b, normal), depth)
    h, w = depth.shape
    p = pair_params(iterations, sigma_color, sigma_normal, sigma_depth, var_floor)
    out = np.zeros_like(a)
    var = np.zeros_like(depth) if return_variance else None
    _abi.check(_entry("dr_denoise_pair", device)(a.ctypes.data, b.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data,
                  var.ctypes.data if return_variance else None))
    return (out, var) if return_variance else out


def pair_seed(seed):
    """The second half's default seed: the sampler's with the bits of 0x2545F491 flipped, so it always differs."""
    return int(seed) ^ SEED_B_XOR


def render_denoised_pair(renderer, scene, seed_b=None, normal_channel="ns", firefly=False, one_pass=False, demodulate=False, **filter_kw):
    """Renders the scene twice -- half A with `renderer` as given, half B with a shallow copy of its sampler whose seed is `seed_b` (default:
    pair_seed of the sampler's seed) -- and the two guides as render_denoised does, all four with the same camera, integrators and work
    split, and filters the halves' mean with atrous_pair.  Returns an OutputImage whose rgb is the result; `a`, `b`, `noisy` (the mean),
    `normal`, `depth` and `variance` (the last level's, -1 where a pixel is not valid) stay on it.  filter_kw: atrous_pair()'s keywords.

    Each half costs a full render at the sampler's spp: the fair comparison with render_denoised at N samples per pixel is this function
    with a sampler of N / 2.

    firefly: True, or a dict of firefly()'s parameters, clamps each half's outliers before the filter, so that a bright
    pixel of one half no longer inflates the variance estimate its neighbours share; `a`, `b` and `noisy` stay the unclamped renders, and
    the luminance taken from the halves stays on the result as `removed` = (removed_a, removed_b).

    one_pass=True: the guides ride on half A's render (render_with_guides) -- three renders instead of four, the same bytes.

    demodulate: as for render_denoised; the material images are rendered once, with half A's sampler, and each half is demodulated by the
    same images before its firefly clamp (the images are noise-free: what differs between two seeds is the film's sub-pixel coverage at
    an edge).  `variance` is then the demodulated colour's; `demodulated` = (a, b) demodulated."""
    _check_channel("render_denoised_pair", normal_channel)
    fkw = _firefly_kw("render_denoised_pair", firefly)
    dm = _demodulate_kw("render_denoised_pair", demodulate, one_pass)
    sampler = renderer.sampler
    if isinstance(sampler, AdaptiveSampler):
        raise ValueError("render_denoised_pair: the adaptive sampler is not supported (the feature integrator refuses it)")
    if getattr(sampler, "seed", None) is None:
        raise ValueError("render_denoised_pair: %s has no seed to vary" % (type(sampler).__name__,))
    seed_b = pair_seed(sampler.seed) if seed_b is None else int(seed_b)
    if seed_b == sampler.seed:
        raise ValueError("render_denoised_pair: seed_b equals the sampler's seed (%d): the two halves would be one render" % (seed_b,))
    sampler_b = copy.copy(sampler)
    sampler_b.seed = seed_b
    _check_one_pass("render_denoised_pair", one_pass, renderer, scene, normal_channel)
    if one_pass:
        half_a, normal, depth = _beauty_and_guides(renderer, scene, normal_channel, True)
        half_b = _rerender(renderer, scene, renderer.surfaceIntegrator, sampler_b)
    else:
        half_a = renderer.render(scene)
        half_b = _rerender(renderer, scene, renderer.surfaceIntegrator, sampler_b)
        normal, depth = _guides(renderer, scene, normal_channel)
    mats = _material_images(renderer, scene, dm)
    on_device = filter_kw.get("device", True)
    filter_kw = dict(filter_kw, return_variance=True)
    base_a, base_b = _demodulated(dm, mats, half_a.rgb, on_device), _demodulated(dm, mats, half_b.rgb, on_device)
    (a, removed_a), (b, removed_b) = _clamped(fkw, base_a, normal, depth), _clamped(fkw, base_b, normal, depth)
    rgb, variance = atrous_pair(a, b, normal, depth, **filter_kw)
    rgb = _remodulated(dm, mats, rgb, on_device)
    out = OutputImage(half_a.xOffset, half_a.yOffset, half_a.width, half_a.height, rgb, half_a.film)
    out.a, out.b, out.normal, out.depth, out.variance = half_a.rgb, half_b.rgb, normal, depth, variance
    if fkw is not None:
        out.removed = (removed_a, removed_b)
    if dm is not None:
        _keep_material(out, mats, (base_a, base_b))
    with np.errstate(all="ignore"):
        out.noisy = np.float32(0.5) * (out.a + out.b)
    return out


def upsample_params(factor, taps=2, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH):
    return _abi.DrUpsampleParams(int(factor), int(taps), sharpness(sigma_normal), sharpness(sigma_depth))


def upsample(rgb_lo, normal_lo, depth_lo, normal, depth, factor=None, taps=2, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH, device=True):
    """rgb_lo [hl, wl, 3], normal_lo [hl, wl, 3], depth_lo [hl, wl] -- an image rendered at 1/factor of the resolution per axis and the guides
    aligned with it -- and the full-resolution guides normal [h, w, 3], depth [h, w], h = factor * hl, w = factor * wl -> the upsampled
    [h, w, 3] f32.  factor: 2 or 4; None derives it from the shapes.  taps: 2 or 4, the footprint's side in low-resolution pixels.
    device=True: dr_upsample, on the GPU; device=False: dr_upsample_host, which needs none and writes the same bytes."""
    rgb_lo, normal_lo, depth_lo = _images("upsample", "rgb_lo and normal_lo must be [hl, wl, 3] and depth_lo [hl, wl]", (rgb_lo, normal_lo), depth_lo)
    normal, depth = _images("upsample", "normal must be [h, w, 3] and depth [h, w]", (normal,), depth)
    hl, wl = depth_lo.shape
    h, w = depth.shape
    if factor is None:
        factor = h // hl if hl else 0
        if factor not in (2, 4):
            raise ValueError("upsample: the full-resolution guides must be 2 or 4 times the low-resolution image in both axes (got %r for %r)"
                             % (depth.shape, depth_lo.shape))
    factor = int(factor)
    if (h, w) != (factor * hl, factor * wl):
        raise ValueError("upsample: the full-resolution guides must be %d times the low-resolution image in both axes (got %r for %r)"
                         % (factor, depth.shape, depth_lo.shape))
    p = upsample_params(factor, taps, sigma_normal, sigma_depth)
    out = np.zeros_like(normal)
    _abi.check(_entry("dr_upsample", device)(rgb_lo.ctypes.data, normal_lo.ctypes.data, depth_lo.ctypes.data, wl, hl, normal.ctypes.data, depth.ctypes.data, C.byref(p),
                  out.ctypes.data))
    return out


def _upsample_refusals(who, low, full):
    """What render_upsampled asks of its two renderers, each refusal by name; returns the factor."""
    for name, r in (("low_renderer", low), ("full_renderer", full)):
        _whole_film_refusals(who, name, r, "upsampling")
    lf, ff = low.camera.film, full.camera.film
    lo, hi = (lf.xResolution, lf.yResolution), (ff.xResolution, ff.yResolution)
    factor = next((f for f in (2, 4) if hi == (f * lo[0], f * lo[1])), None)
    if factor is None:
        raise ValueError("%s: full_renderer's film must be exactly 2 or 4 times low_renderer's in both axes (got %d x %d for %d x %d)"
                         % (who, hi[0], hi[1], lo[0], lo[1]))
    pose = [getattr(r.camera, "cameraToWorld", None) for r in (low, full)]
    if pose[0] is not None and pose[1] is not None and not np.array_equal(np.asarray(pose[0]), np.asarray(pose[1])):
        raise ValueError("%s: low_renderer's and full_renderer's cameras differ in their pose" % (who,))
    return factor


def render_upsampled(low_renderer, full_renderer, scene, normal_channel="ns", taps=2, denoise=False, firefly=False, one_pass=False, **kw):
    """Renders the beauty image and two FeatureIntegrator images -- `normal_channel` ("ns" or "ng") and "depth" -- with `low_renderer`, whose
    film is 1/2 or 1/4 of `full_renderer`'s in both axes over the same camera pose, the same two guides with `full_renderer`'s sampler and
    camera -- its own surface integrator is never run -- and upsamples.  Returns an OutputImage of the full size whose rgb is the result;
    with denoise=True it is atrous(upsampled, normal, depth, **kw).  The parts stay on it as `low` [hl, wl, 3], `normal_lo`, `depth_lo`,
    `normal` and `depth`, and `upsampled` [h, w, 3].  kw: sigma_normal and sigma_depth go to both stages; atrous()'s other keywords need
    denoise=True.  firefly: True, or a dict of firefly()'s parameters, clamps the low-resolution beauty image's outliers under the
    low-resolution guides before it is upsampled; `low` stays the unclamped render, and the luminance taken away stays on
    the result as `removed` [hl, wl].  one_pass=True: the low-resolution image and its two guides come from one render (render_with_guides,
    DESIGN.md 2.26), the same bytes; the full-resolution guides have no beauty render to ride on and stay FeatureIntegrator renders."""
    who = "render_upsampled"
    _check_channel(who, normal_channel)
    fkw = _firefly_kw(who, firefly)
    factor = _upsample_refusals(who, low_renderer, full_renderer)
    _check_one_pass(who, one_pass, low_renderer, scene, normal_channel)
    guide_kw = {k: kw[k] for k in ("sigma_normal", "sigma_depth") if k in kw}
    if not denoise and len(guide_kw) != len(kw):
        raise ValueError("%s: %s given without denoise=True" % (who, ", ".join(sorted(set(kw) - set(guide_kw)))))
    low, normal_lo, depth_lo = _beauty_and_guides(low_renderer, scene, normal_channel, one_pass)
    normal, depth = _guides(full_renderer, scene, normal_channel)
    low_rgb, removed = _clamped(fkw, low.rgb, normal_lo, depth_lo)
    up = upsample(low_rgb, normal_lo, depth_lo, normal, depth, factor=factor, taps=taps, **guide_kw)
    film = full_renderer.camera.film
    out = OutputImage(film.left, film.top, film.width, film.height, atrous(up, normal, depth, **kw) if denoise else up)
    out.low, out.normal_lo, out.depth_lo, out.normal, out.depth, out.upsampled = low.rgb, normal_lo, depth_lo, normal, depth, up
    if fkw is not None:
        out.removed = removed
    return out


# Temporal accumulation's defaults, set by reasoning and not tuned on any animation.  depth_tol: the reprojected distance and
# the stored one are two roundings of one length where the surface is the same, and differ by the surface's depth gradient over the one
# pixel a bilinear tap may lie away: a 35-degree lens at 64 pixels has pixels of 0.01 rad, so 2 % keeps a surface seen at up to 63 degrees
# from its normal (tan 63 x 0.01), steeper ones at higher resolutions, and drops a step of more than 2 % of the distance.  normal_tol: the
# guide is 0.5 * (n + 1), so a squared distance of 0.05 is |dn| = 0.45, about 26 degrees: wider than the a-trous filters' 11 degrees because
# a rejected tap costs the whole history, not a part of one weight.  max_history: a new frame's weight never falls below 1/32; SVGF's fixed
# alpha = 0.2 forgets within about five frames because it follows moving lights and objects, which are out of scope here, and a static
# scene gains nothing from forgetting.
DEPTH_TOL = 0.02
NORMAL_TOL = 0.05
MAX_HISTORY = 32


def _camera_refusals(who, name, camera):
    if type(camera) is not PerspectiveCamera:
        raise ValueError("%s: %s is a %s: only a PerspectiveCamera is supported" % (who, name, type(camera).__name__))
    if camera.lensRadius != 0.0:
        raise ValueError("%s: %s has lensRadius %r: a camera with a lens is not supported" % (who, name, camera.lensRadius))


def temporal_matrices(camera, prev_camera):
    """The three row-major f64 4 x 4 matrices dr_temporal* takes -- (raster_to_camera, cur_to_prev, prev_to_raster) -- composed with numpy from
    the two cameras' rasterToCamera and cameraToWorld: cur_to_prev = inv(prev.cameraToWorld) . cur.cameraToWorld and prev_to_raster =
    inv(prev.rasterToCamera).  Both must be a PerspectiveCamera with lensRadius 0 over films of one size."""
    who = "temporal_matrices"
    _camera_refusals(who, "camera", camera)
    _camera_refusals(who, "prev_camera", prev_camera)
    cf, pf = camera.film, prev_camera.film
    if (cf.xResolution, cf.yResolution) != (pf.xResolution, pf.yResolution):
        raise ValueError("%s: the two cameras' films differ in size (%d x %d and %d x %d)"
                         % (who, cf.xResolution, cf.yResolution, pf.xResolution, pf.yResolution))
    r2c = np.array(camera.rasterToCamera, dtype=np.float64).reshape(4, 4)
    cur_to_prev = np.linalg.inv(np.array(prev_camera.cameraToWorld, dtype=np.float64).reshape(4, 4)) @ np.array(camera.cameraToWorld, dtype=np.float64).reshape(4, 4)
    prev_to_raster = np.linalg.inv(np.array(prev_camera.rasterToCamera, dtype=np.float64).reshape(4, 4))
    return r2c, cur_to_prev, prev_to_raster


def temporal_params(matrices, depth_tol=DEPTH_TOL, normal_tol=NORMAL_TOL, max_history=MAX_HISTORY):
    if len(matrices) != 3:
        raise ValueError("temporal: matrices must be (raster_to_camera, cur_to_prev, prev_to_raster), got %d of them" % (len(matrices),))
    p = _abi.DrTemporalParams()
    for name, m in zip(("raster_to_camera", "cur_to_prev", "prev_to_raster"), matrices):
        m = np.asarray(m, dtype=np.float64)
        if m.size != 16:
            raise ValueError("temporal: %s must be a 4 x 4 matrix (got shape %r)" % (name, m.shape))
        getattr(p, name)[:] = [float(v) for v in m.reshape(-1)]
    p.depth_tol, p.normal_tol, p.max_history = float(depth_tol), float(normal_tol), int(max_history)
    return p


class TemporalFrame:
    """What temporal() returns and takes back as `history`: the accumulated colour `rgb` [h, w, 3], the accumulated second moment of the
    luminance `m2` [h, w], the history length `len` [h, w] (f32; 0: none), and the frame's own guides `normal` and `depth`."""

    def __init__(self, rgb, m2, len, normal, depth):
        self.rgb, self.m2, self.len, self.normal, self.depth = rgb, m2, len, normal, depth

    @property
    def variance(self):
        """max(0, m2 - lum(rgb)^2) [h, w]: the luminance variance the accumulated moments estimate (0 after one frame)."""
        rgb = self.rgb
        with np.errstate(all="ignore"):
            lum = (np.float32(0.212671) * rgb[..., 0] + np.float32(0.715160) * rgb[..., 1]) + np.float32(0.072169) * rgb[..., 2]
            return np.maximum(np.float32(0), self.m2 - lum * lum)


def temporal(rgb, normal, depth, history, matrices, depth_tol=DEPTH_TOL, normal_tol=NORMAL_TOL, max_history=MAX_HISTORY, device=True):
    """One frame of temporal accumulation.  rgb [h, w, 3], normal [h, w, 3] and depth [h, w] are the current frame and its
    FeatureIntegrator guides; `history` is None (the first frame) or the TemporalFrame the previous call returned; `matrices` is
    temporal_matrices(camera, prev_camera) (read only with a history, but always checked).  Returns a TemporalFrame.  device=True:
    dr_temporal, on the GPU; device=False: dr_temporal_host, which needs none and writes the same bytes."""
    rgb, normal, depth = _images("temporal", "rgb and normal must be [h, w, 3] and depth [h, w]", (rgb, normal), depth)
    h, w = depth.shape
    hist = [None] * 5
    if history is not None:
        hist = [np.ascontiguousarray(a, dtype=np.float32) for a in (history.rgb, history.m2, history.len, history.normal, history.depth)]
        if hist[0].shape != rgb.shape or hist[3].shape != rgb.shape or any(a.shape != depth.shape for a in (hist[1], hist[2], hist[4])):
            raise ValueError("temporal: the history is of another size (%r for %r)" % (hist[0].shape, rgb.shape))
    p = temporal_params(matrices, depth_tol, normal_tol, max_history)
    out = TemporalFrame(np.zeros_like(rgb), np.zeros_like(depth), np.zeros_like(depth), normal, depth)
    _abi.check(_entry("dr_temporal", device)(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, *[a.ctypes.data if a is not None else None for a in hist], w, h,
                  C.byref(p), out.rgb.ctypes.data, out.m2.ctypes.data, out.len.ctypes.data))
    return out


# Firefly suppression's defaults, reasoned and not tuned on any scene.  radius 1: the eight nearest pixels are the ones most
# likely to show the same surface under the same light.  rank 2: the limit comes from the second brightest member, so two fireflies side by
# side do not shield each other, while a bright line one pixel wide and the corner of an emitter survive -- each of their pixels has two
# equally bright neighbours on the same surface.  threshold 4: a pixel may be four times as bright as that neighbour before it is taken for
# an outlier.  floor 0: nothing is added, so in a neighbourhood whose members are black any lit pixel is clamped to black.  The two
# tolerances are temporal accumulation's: the same question -- is this the same surface? -- asked of the same guides.
FIREFLY_RADIUS = 1
FIREFLY_RANK = 2
FIREFLY_THRESHOLD = 4.0
FIREFLY_FLOOR = 0.0


def firefly_params(radius=FIREFLY_RADIUS, rank=FIREFLY_RANK, threshold=FIREFLY_THRESHOLD, floor=FIREFLY_FLOOR, depth_tol=DEPTH_TOL,
                   normal_tol=NORMAL_TOL):
    return _abi.DrFireflyParams(int(radius), int(rank), float(threshold), float(floor), float(depth_tol), float(normal_tol))


def firefly(rgb, normal, depth, radius=FIREFLY_RADIUS, rank=FIREFLY_RANK, threshold=FIREFLY_THRESHOLD, floor=FIREFLY_FLOOR, depth_tol=DEPTH_TOL,
            normal_tol=NORMAL_TOL, device=True, return_removed=False):
    """rgb [h, w, 3], normal [h, w, 3], depth [h, w] -> the clamped [h, w, 3] f32: a pixel whose luminance exceeds
    threshold * m + floor, m the rank-th largest luminance among the pixels of its (2 radius + 1)^2 window that show the same surface, is
    scaled down to that limit; every other pixel keeps its bits.  return_removed=True adds the luminance taken away [h, w] (0 where the
    pixel is unchanged).  device=True: dr_firefly, on the GPU; device=False: dr_firefly_host, which needs none and writes the same bytes."""
    rgb, normal, depth = _images("firefly", "rgb and normal must be [h, w, 3] and depth [h, w]", (rgb, normal), depth)
    h, w = depth.shape
    p = firefly_params(radius, rank, threshold, floor, depth_tol, normal_tol)
    out = np.zeros_like(rgb)
    removed = np.zeros_like(depth) if return_removed else None
    _abi.check(_entry("dr_firefly", device)(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data,
                  removed.ctypes.data if return_removed else None))
    return (out, removed) if return_removed else out


def _firefly_kw(who, firefly):
    """The `firefly` keyword of a render_* function as firefly()'s keywords, or None where the stage is off."""
    if firefly is False or firefly is None:
        return None
    if firefly is True:
        return {}
    if isinstance(firefly, dict):
        unknown = sorted(set(firefly) - {"radius", "rank", "threshold", "floor", "depth_tol", "normal_tol", "device"})
        if unknown:
            raise ValueError("%s: firefly has no parameter %s" % (who, ", ".join(unknown)))
        return dict(firefly)
    raise ValueError("%s: firefly must be False, True or a dict of firefly()'s parameters, got %r" % (who, firefly))


def _clamped(kw, rgb, normal, depth):
    """(rgb after the stage, removed) -- or (rgb, None) where the stage is off (kw None)."""
    return (rgb, None) if kw is None else firefly(rgb, normal, depth, **dict(kw, return_removed=True))


# Demodulation's one parameter, reasoned and not tuned on any scene.  eps only matters where the albedo is close to 0: the
# same a + eps divides and multiplies back, so on an unfiltered pixel it cancels up to two roundings.  What it sets is the gain, 1 / (a + eps),
# with which a dark surface's noise enters the filter: at most 1000.  The darkest common materials reflect about 3 % (a = 0.03: gain 32, which
# eps changes by 3 %); a surface of a = 0 reflects nothing, so rgb - e is 0 there and the gain multiplies 0.  1e-3 is also far above f32's
# spacing at 1, so a + eps != a for every albedo up to 1.
DEMODULATE_EPS = 1.0e-3
MATERIAL_CHANNELS = ("emission", "albedo")


def demodulate_params(eps=DEMODULATE_EPS):
    return _abi.DrDemodulateParams(float(eps))


def _modulate(entry, who, rgb, emission, albedo, eps, device):
    present = [a for a in (emission, albedo) if a is not None]
    imgs = _images(who, "rgb, emission and albedo must be [h, w, 3]", [rgb] + present)
    rgb, rest = imgs[0], iter(imgs[1:])
    emission = next(rest) if emission is not None else None
    albedo = next(rest) if albedo is not None else None
    h, w = rgb.shape[:2]
    p = demodulate_params(eps)
    out = np.zeros_like(rgb)
    _abi.check(_entry(entry, device)(rgb.ctypes.data, emission.ctypes.data if emission is not None else None,
                                     albedo.ctypes.data if albedo is not None else None, w, h, C.byref(p), out.ctypes.data))
    return out


def demodulate(rgb, emission=None, albedo=None, eps=DEMODULATE_EPS, device=True):
    """rgb [h, w, 3], emission [h, w, 3] or None, albedo [h, w, 3] or None -> max(0, rgb - emission) / (albedo + eps), [h, w, 3] f32
    (DESIGN.md 2.27).  An absent emission is 0; an absent albedo makes the divisor 1.  A pixel with a value that is not finite keeps its rgb
    bits.  device=True: dr_demodulate, on the GPU; device=False: dr_demodulate_host, which needs none and writes the same bytes."""
    return _modulate("dr_demodulate", "demodulate", rgb, emission, albedo, eps, device)


def remodulate(rgb, emission=None, albedo=None, eps=DEMODULATE_EPS, device=True):
    """The inverse after the filters: rgb * (albedo + eps) + emission, with demodulate()'s images and eps.  device as for demodulate()."""
    return _modulate("dr_remodulate", "remodulate", rgb, emission, albedo, eps, device)


def _demodulate_kw(who, demodulate, one_pass=False):
    """The `demodulate` keyword of a render_* function as the tuple of material channels to render, or None where the stage is off."""
    if demodulate is False or demodulate is None:
        return None
    if demodulate is True:
        channels = MATERIAL_CHANNELS
    elif isinstance(demodulate, (tuple, list)) and demodulate and all(c in MATERIAL_CHANNELS for c in demodulate) \
            and len(set(demodulate)) == len(demodulate):
        channels = tuple(c for c in MATERIAL_CHANNELS if c in demodulate)
    else:
        raise ValueError("%s: demodulate must be False, True or a tuple of \"emission\" and / or \"albedo\", got %r" % (who, demodulate))
    if one_pass:
        raise ValueError("%s: one_pass=True together with demodulate is not supported (the one-pass guide render has no material channels: "
                         "render the guides separately)" % (who,))
    return channels


def _material_images(renderer, scene, channels, sampler=None):
    """{channel: [h, w, 3]} of the MaterialIntegrator renders of `channels` (None: {}) with `renderer`'s camera, sampler and work split."""
    return {c: _rerender(renderer, scene, MaterialIntegrator(c), sampler).rgb for c in (channels or ())}


def _demodulated(channels, mats, rgb, device=True):
    """rgb after demodulate() by the rendered images -- or rgb itself where the stage is off (channels None)."""
    return rgb if channels is None else demodulate(rgb, mats.get("emission"), mats.get("albedo"), device=device)


def _remodulated(channels, mats, rgb, device=True):
    return rgb if channels is None else remodulate(rgb, mats.get("emission"), mats.get("albedo"), device=device)


def _keep_material(out, mats, demodulated):
    """The material images and the demodulated render(s), beside the other parts on a render_* function's result."""
    for c, img in mats.items():
        setattr(out, c, img)
    out.demodulated = demodulated


def render_firefly(renderer, scene, normal_channel="ns", one_pass=False, **firefly_kw):
    """Renders the beauty image and the two guides as render_denoised does and clamps its fireflies.  Returns an OutputImage whose rgb is
    the result; `noisy` (the unclamped render), `normal`, `depth` and `removed` stay on it.  firefly_kw: firefly()'s keywords.
    one_pass=True: one render instead of three, as for render_denoised."""
    _check_channel("render_firefly", normal_channel)
    if isinstance(renderer.sampler, AdaptiveSampler):
        raise ValueError("render_firefly: the adaptive sampler is not supported (the feature integrator refuses it)")
    _check_one_pass("render_firefly", one_pass, renderer, scene, normal_channel)
    beauty, normal, depth = _beauty_and_guides(renderer, scene, normal_channel, one_pass)
    rgb, removed = firefly(beauty.rgb, normal, depth, **dict(firefly_kw, return_removed=True))
    out = OutputImage(beauty.xOffset, beauty.yOffset, beauty.width, beauty.height, rgb, beauty.film)
    out.noisy, out.normal, out.depth, out.removed = beauty.rgb, normal, depth, removed
    return out


# The moments filter's own two, SVGF's and reasoned, not tuned on any animation.  min_history: below four frames the sample
# variance of the per-frame luminance has two degrees of freedom or fewer and is mostly noise itself, so the neighbours are asked instead.
# radius: a 7 x 7 window is 49 accumulated values, the fewest at which a spatial estimate is steadier than a four-frame temporal one.
MIN_HISTORY = 4
RADIUS = 3


def moments_params(iterations=ITERATIONS, sigma_color=SIGMA_COLOR_PAIR, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH, var_floor=VAR_FLOOR,
                   min_history=MIN_HISTORY, radius=RADIUS):
    return _abi.DrDenoiseMomentsParams(int(iterations), sharpness(sigma_color), sharpness(sigma_normal), sharpness(sigma_depth), float(var_floor),
                                       int(min_history), int(radius))


def atrous_moments(frame, iterations=ITERATIONS, sigma_color=SIGMA_COLOR_PAIR, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH,
                   var_floor=VAR_FLOOR, min_history=MIN_HISTORY, radius=RADIUS, device=True, return_variance=False, return_estimate=False):
    """frame: a TemporalFrame, or anything with rgb [h, w, 3], m2 [h, w], len [h, w], normal [h, w, 3] and depth [h, w] -> its colour, filtered,
    [h, w, 3] f32, guided by the per-pixel variance its moments estimate: the temporal one where len >= min_history, else the spatial one over
    the (2 radius + 1)^2 window.  return_variance=True adds the variance [h, w] the last level leaves, return_estimate=True the estimate
    [h, w] before any level (-1: the pixel is not valid), in that order.  sigma_color is in standard deviations of the local noise.
    device=True: dr_denoise_moments, on the GPU; device=False: dr_denoise_moments_host, which needs none and writes the same bytes."""
    for name in ("rgb", "m2", "len", "normal", "depth"):
        if not hasattr(frame, name):
            raise ValueError("denoise: frame has no %s (a TemporalFrame, or anything with rgb, m2, len, normal and depth)" % (name,))
    rgb, normal, depth = _images("denoise", "rgb and normal must be [h, w, 3] and depth [h, w]", (frame.rgb, frame.normal), frame.depth)
    m2, length = (np.ascontiguousarray(a, dtype=np.float32) for a in (frame.m2, frame.len))
    if m2.shape != depth.shape or length.shape != depth.shape:
        raise ValueError("denoise: m2 and len must be [h, w] like depth (got %r and %r for %r)" % (m2.shape, length.shape, depth.shape))
    h, w = depth.shape
    p = moments_params(iterations, sigma_color, sigma_normal, sigma_depth, var_floor, min_history, radius)
    out = np.zeros_like(rgb)
    var = np.zeros_like(depth) if return_variance else None
    var0 = np.zeros_like(depth) if return_estimate else None
    _abi.check(_entry("dr_denoise_moments", device)(rgb.ctypes.data, m2.ctypes.data, length.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h,
                  C.byref(p), out.ctypes.data, var.ctypes.data if return_variance else None, var0.ctypes.data if return_estimate else None))
    extra = [a for a in (var, var0) if a is not None]
    return (out, *extra) if extra else out


def render_sequence(renderers, scene, normal_channel="ns", denoise=False, depth_tol=DEPTH_TOL, normal_tol=NORMAL_TOL, max_history=MAX_HISTORY,
                    firefly=False, one_pass=False, demodulate=False, **kw):
    """Renders one frame per renderer -- one camera pose each, in the order of the animation -- with its beauty image and two
    FeatureIntegrator images, `normal_channel` ("ns" or "ng") and "depth", as render_denoised does, and accumulates each into the history of
    the frames before it with temporal().  Returns the list of frames: OutputImages whose rgb is the accumulated colour, or with denoise=True
    atrous(accumulated, normal, depth, **kw), or with denoise="moments" atrous_moments(history, **kw), whose last level's variance then stays
    on the frame as `filtered_variance`; the parts stay on each as `noisy` (the frame's own render), `accumulated`, `normal`, `depth`,
    `m2`, `len`, `variance` and `history` (the TemporalFrame).  The history itself is never filtered: the next frame accumulates onto the
    unfiltered colour.  firefly: True, or a dict of firefly()'s parameters, clamps each frame's beauty image before temporal() (DESIGN.md
    2.25), so that an outlier never enters `rgb`, `m2` or the history; `noisy` stays the unclamped render, and the luminance taken away
    stays on each frame as `removed`.

    Give each renderer's sampler its own seed.  The samplers are keyed by pixel and seed: two frames that share a seed draw the same sample
    pattern in every pixel, so a surface that stays under one pixel is sampled with the same numbers again, the frames' errors are the same
    error, and their mean is no better than one of them.  The guides are another matter: they are filtered over the sampler's positions too,
    so where a pixel straddles a silhouette two seeds give two depths, and a static camera would lose its history there in every frame.
    Every frame's guides are therefore rendered with a copy of its sampler that carries the first renderer's seed: at one pose the guides are
    the same bytes whatever the beauty image's seed.

    one_pass=True: a frame whose sampler carries the guides' seed -- the first frame, and every frame of a sequence that shares one seed or
    whose sampler has none -- takes its beauty image and its guides from one render (render_with_guides), the same bytes.  A
    frame with a seed of its own keeps its two FeatureIntegrator renders: its guides are sampled with another seed than its beauty image, so
    they have no beauty render to ride on.

    demodulate: as for render_denoised.  Each frame's material images are rendered with the frame's own sampler, the frame is demodulated
    before its firefly clamp and temporal(), and the filter's output (or, without a filter, the accumulated colour) is remodulated by the
    frame's own images: the history -- `accumulated`, `m2`, `variance`, `history` -- holds demodulated colour, so an emitter that comes into
    view is never blended with what the history saw there before.  The images stay on each frame as `emission` / `albedo`.  Measured on C2
    with a seed per frame this makes the moments filter worse, not better (MEASUREMENTS.md, "Demodulation": the history's frames were
    demodulated by their own images and are remodulated by the last frame's alone)."""
    who = "render_sequence"
    _check_channel(who, normal_channel)
    renderers = list(renderers)
    fkw = _firefly_kw(who, firefly)
    dm = _demodulate_kw(who, demodulate, one_pass)
    if not any(denoise is v for v in (False, True)) and denoise != "moments":
        raise ValueError("%s: denoise must be False, True or \"moments\", got %r" % (who, denoise))
    if kw and not denoise:
        raise ValueError("%s: %s given without denoise=True" % (who, ", ".join(sorted(kw))))
    for k, r in enumerate(renderers):
        name = "renderers[%d]" % k
        _whole_film_refusals(who, name, r, "accumulation", each=False)
        _camera_refusals(who, name + ".camera", r.camera)
    _check_one_pass(who, one_pass)
    for r in renderers if one_pass else ():
        _check_one_pass(who, one_pass, r, scene, normal_channel)
    mats = [temporal_matrices(r.camera, renderers[max(k - 1, 0)].camera) for k, r in enumerate(renderers)]

    guide_seed = getattr(renderers[0].sampler, "seed", None) if renderers else None
    frames, history = [], None
    for r, m in zip(renderers, mats):
        guide_sampler = r.sampler
        if guide_seed is not None and getattr(guide_sampler, "seed", None) is not None:
            guide_sampler = copy.copy(r.sampler)
            guide_sampler.seed = guide_seed
        if one_pass and (guide_sampler is r.sampler or guide_sampler.seed == r.sampler.seed):
            beauty, normal, depth = _beauty_and_guides(r, scene, normal_channel, True)
        else:
            beauty = r.render(scene)
            normal, depth = _guides(r, scene, normal_channel, guide_sampler)
        mats = _material_images(r, scene, dm)
        on_device = kw.get("device", True)
        base = _demodulated(dm, mats, beauty.rgb, on_device)
        clamped, removed = _clamped(fkw, base, normal, depth)
        history = temporal(clamped, normal, depth, history, m, depth_tol=depth_tol, normal_tol=normal_tol, max_history=max_history)
        filtered_variance = None
        if denoise == "moments":
            rgb, filtered_variance = atrous_moments(history, **dict(kw, return_variance=True, return_estimate=False))
        else:
            rgb = atrous(history.rgb, normal, depth, **kw) if denoise else history.rgb
        rgb = _remodulated(dm, mats, rgb, on_device)
        out = OutputImage(beauty.xOffset, beauty.yOffset, beauty.width, beauty.height, rgb, beauty.film)
        if filtered_variance is not None:
            out.filtered_variance = filtered_variance
        out.noisy, out.accumulated, out.normal, out.depth = beauty.rgb, history.rgb, normal, depth
        out.m2, out.len, out.variance, out.history = history.m2, history.len, history.variance, history
        if fkw is not None:
            out.removed = removed
        if dm is not None:
            _keep_material(out, mats, base)
        frames.append(out)
    return frames
