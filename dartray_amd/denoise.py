"""The edge-avoiding a-trous denoiser (dr_denoise_atrous*): a post-process beside the render path, guided by the
images of the first-hit feature integrator.

    atrous(rgb, normal, depth, ...)          filters one image
    render_denoised(renderer, scene, ...)    renders the beauty image and its two guides, and filters

and its variance-guided form over two half-sample renders (dr_denoise_pair*):

    atrous_pair(a, b, normal, depth, ...)         filters the mean of two renders, guided by the variance their difference estimates
    render_denoised_pair(renderer, scene, ...)    renders the two halves and the two guides, and filters

The library takes sharpness values k = 1 / sigma^2 (k = 0: the term is off); this module takes the sigmas.
"""
import copy
import ctypes as C
import math

import numpy as np

from . import _abi
from .core.renderer import FeatureIntegrator, OutputImage, SamplerRenderer
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
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or normal.shape != rgb.shape or depth.shape != rgb.shape[:2]:
        raise ValueError("denoise: rgb and normal must be [h, w, 3] and depth [h, w] (got %r, %r, %r)" % (rgb.shape, normal.shape, depth.shape))
    h, w = depth.shape
    p = params(iterations, sigma_color, sigma_normal, sigma_depth)
    out = np.zeros_like(rgb)
    lib = _abi.lib()
    if device:
        _abi.init(_abi._initialised if _abi._initialised is not None else 0)
    fn = lib.dr_denoise_atrous if device else lib.dr_denoise_atrous_host
    _abi.check(fn(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data))
    return out


def render_denoised(renderer, scene, normal_channel="ns", **filter_kw):
    """Renders the beauty image with `renderer` as given and two FeatureIntegrator images -- `normal_channel` ("ns" or "ng") and "depth" --
    with the same camera, film, sampler and work split, filters, and returns an OutputImage whose rgb is the result; the three unfiltered
    images stay on it as `noisy` [h, w, 3], `normal` [h, w, 3] and `depth` [h, w].  filter_kw: atrous()'s keywords."""
    if normal_channel not in ("ns", "ng"):
        raise ValueError("render_denoised: normal_channel must be ns or ng (got %r)" % (normal_channel,))
    if isinstance(renderer.sampler, AdaptiveSampler):
        raise ValueError("render_denoised: the adaptive sampler is not supported (the feature integrator refuses it)")

    def guide(channel):
        return SamplerRenderer(renderer.sampler, renderer.camera, FeatureIntegrator(channel), renderer.volumeIntegrator,
                               taskNum=renderer.taskNum, taskCount=renderer.taskCount, tileRank=renderer.tileRank,
                               tileCount=renderer.tileCount, tileSize=renderer.tileSize).render(scene)
    beauty = renderer.render(scene)
    normal = guide(normal_channel).rgb
    depth = np.ascontiguousarray(guide("depth").rgb[..., 0])
    out = OutputImage(beauty.xOffset, beauty.yOffset, beauty.width, beauty.height, atrous(beauty.rgb, normal, depth, **filter_kw), beauty.film)
    out.noisy, out.normal, out.depth = beauty.rgb, normal, depth
    return out


def pair_params(iterations=ITERATIONS, sigma_color=SIGMA_COLOR_PAIR, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH, var_floor=VAR_FLOOR):
    return _abi.DrDenoisePairParams(int(iterations), sharpness(sigma_color), sharpness(sigma_normal), sharpness(sigma_depth), float(var_floor))


def atrous_pair(a, b, normal, depth, iterations=ITERATIONS, sigma_color=SIGMA_COLOR_PAIR, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH,
                var_floor=VAR_FLOOR, device=True, return_variance=False):
    """a [h, w, 3] and b [h, w, 3], two renders of one scene that differ in the sampler's seed alone, normal [h, w, 3], depth [h, w] -> their
    mean, filtered, [h, w, 3] f32; with return_variance=True also the variance [h, w] the last level leaves (-1: the pixel is not valid).
    sigma_color is in standard deviations of the local noise.  device=True: dr_denoise_pair, on the GPU; device=False:
    dr_denoise_pair_host, which needs none and writes the same bytes."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3 or b.shape != a.shape or normal.shape != a.shape or depth.shape != a.shape[:2]:
        raise ValueError("denoise: a, b and normal must be [h, w, 3] and depth [h, w] (got %r, %r, %r, %r)"
                         % (a.shape, b.shape, normal.shape, depth.shape))
    h, w = depth.shape
    p = pair_params(iterations, sigma_color, sigma_normal, sigma_depth, var_floor)
    out = np.zeros_like(a)
    var = np.zeros_like(depth) if return_variance else None
    lib = _abi.lib()
    if device:
        _abi.init(_abi._initialised if _abi._initialised is not None else 0)
    fn = lib.dr_denoise_pair if device else lib.dr_denoise_pair_host
    _abi.check(fn(a.ctypes.data, b.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data,
                  var.ctypes.data if return_variance else None))
    return (out, var) if return_variance else out


def pair_seed(seed):
    """The second half's default seed: the sampler's with the bits of 0x2545F491 flipped, so it always differs."""
    return int(seed) ^ SEED_B_XOR


def render_denoised_pair(renderer, scene, seed_b=None, normal_channel="ns", **filter_kw):
    """Renders the scene twice -- half A with `renderer` as given, half B with a shallow copy of its sampler whose seed is `seed_b` (default:
    pair_seed of the sampler's seed) -- and the two guides as render_denoised does, all four with the same camera, integrators and work
    split, and filters the halves' mean with atrous_pair.  Returns an OutputImage whose rgb is the result; `a`, `b`, `noisy` (the mean),
    `normal`, `depth` and `variance` (the last level's, -1 where a pixel is not valid) stay on it.  filter_kw: atrous_pair()'s keywords.

    Each half costs a full render at the sampler's spp: the fair comparison with render_denoised at N samples per pixel is this function
    with a sampler of N / 2."""
    if normal_channel not in ("ns", "ng"):
        raise ValueError("render_denoised_pair: normal_channel must be ns or ng (got %r)" % (normal_channel,))
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

    def with_(smp, surface):
        return SamplerRenderer(smp, renderer.camera, surface, renderer.volumeIntegrator, taskNum=renderer.taskNum, taskCount=renderer.taskCount,
                               tileRank=renderer.tileRank, tileCount=renderer.tileCount, tileSize=renderer.tileSize).render(scene)
    half_a = renderer.render(scene)
    half_b = with_(sampler_b, renderer.surfaceIntegrator)
    normal = with_(sampler, FeatureIntegrator(normal_channel)).rgb
    depth = np.ascontiguousarray(with_(sampler, FeatureIntegrator("depth")).rgb[..., 0])
    filter_kw = dict(filter_kw, return_variance=True)
    rgb, variance = atrous_pair(half_a.rgb, half_b.rgb, normal, depth, **filter_kw)
    out = OutputImage(half_a.xOffset, half_a.yOffset, half_a.width, half_a.height, rgb, half_a.film)
    out.a, out.b, out.normal, out.depth, out.variance = half_a.rgb, half_b.rgb, normal, depth, variance
    with np.errstate(all="ignore"):
        out.noisy = np.float32(0.5) * (out.a + out.b)
    return out
