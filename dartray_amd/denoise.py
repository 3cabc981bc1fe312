"""The edge-avoiding a-trous denoiser (dr_denoise_atrous*): a post-process beside the render path, guided by the
images of the first-hit feature integrator.

    atrous(rgb, normal, depth, ...)          filters one image
    render_denoised(renderer, scene, ...)    renders the beauty image and its two guides, and filters

The library takes sharpness values k = 1 / sigma^2 (k = 0: the term is off); this module takes the sigmas.
"""
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
