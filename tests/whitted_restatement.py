"""WhittedIntegrator.Li (surface_integrators/whitted_integrator.dart:26-72) and the two calls it recurses through,
Integrator.SpecularReflect / SpecularTransmit (core/integrator.dart:187-290), restated in plain Python line by line -- the test
side's own reading of the reference, on top of the intersection, BSDF and light functions of tests/golden/dart_restatement.py
(imported, not copied).  The point and the spot light, which that file does not have, are restated here from lights/point_light.dart
and lights/spot_light.dart.

Cited by file.dart:line of the reference.  Spectrum arithmetic is dart_restatement.RGB: three f32 stores per operation.

Every random number comes from the `rng` the caller hands in (anything with randomFloat()), in the reference's call order: the three
of a LightSample.random per light, then the three BSDFSample.random burns of each Specular* call, depth first.  DESIGN.md 2.12 makes
that order the device's contract: draw number d of a sample's walk is the d-th randomFloat() of its keyed in-Li stream, so for the
tests the callable is simply that stream read in order (`keyed_rng`, built on tests/random_restatement.py's own generator and key).
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import dart_restatement as dr  # noqa: E402
from dart_restatement import (BSDF_ALL, BSDF_REFLECTION, BSDF_SPECULAR, BSDF_TRANSMISSION, INFINITY, RGB, AbsDot, Normalize, Ray, Vec,  # noqa: E402
                              f32, getBSDF, isect_Le, transformVector)
import random_restatement as rr  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------
# lights/point_light.dart, lights/spot_light.dart (sampleLAtPoint in the form of dart_restatement's lights:
# (p, pEpsilon, uPos, uComponent) -> (Li, wi, pdf, shadow ray); delta lights ignore the sample)
# ---------------------------------------------------------------------------------------------------------------
def _segment(p, pEpsilon, p2, eps2):                               # VisibilityTester.setSegment (visibility_tester.dart:26-29)
    dist = (p2 - p).length()
    return Ray(p, (p2 - p) / dist, pEpsilon, dist * (1.0 - eps2))


class PointLight:
    def __init__(self, lightPos, intensity):                       # point_light.dart:36-39
        self.lightPos = Vec(*lightPos)
        self.intensity = RGB(*intensity)

    def Le(self, ray):                                             # light.dart:70-72
        return RGB(0.0)

    def sampleLAtPoint(self, p, pEpsilon, uPos, uComponent):       # point_light.dart:41-47
        wi = Normalize(self.lightPos - p)
        return self.intensity / (self.lightPos - p).lengthSquared(), wi, 1.0, _segment(p, pEpsilon, self.lightPos, 0.0)


class SpotLight(PointLight):
    def __init__(self, lightPos, intensity, worldToLight, width, fall):   # spot_light.dart:42-48
        PointLight.__init__(self, lightPos, intensity)
        self.worldToLight = [f32(float(v)) for v in worldToLight]
        self.cosTotalWidth = math.cos(dr.Radians(width))
        self.cosFalloffStart = math.cos(dr.Radians(fall))

    def falloff(self, w):                                          # spot_light.dart:54-70
        wl = Normalize(transformVector(self.worldToLight, w))
        costheta = wl.z
        if costheta < self.cosTotalWidth:
            return 0.0
        if costheta > self.cosFalloffStart:
            return 1.0
        delta = (costheta - self.cosTotalWidth) / (self.cosFalloffStart - self.cosTotalWidth)
        return delta * delta * delta * delta

    def sampleLAtPoint(self, p, pEpsilon, uPos, uComponent):       # spot_light.dart:77-85
        wi = Normalize(self.lightPos - p)
        return (self.intensity * self.falloff(-wi) / (self.lightPos - p).lengthSquared(), wi, 1.0,
                _segment(p, pEpsilon, self.lightPos, 0.0))


# ---------------------------------------------------------------------------------------------------------------
# surface_integrators/whitted_integrator.dart:26-72
# ---------------------------------------------------------------------------------------------------------------
def WhittedLi(scene, ray, isect, rng, maxDepth):
    L = RGB(0.0)                                                   # :28
    # (this module's getBSDF keeps the geometric frame: no golden scene has per-vertex N / S.  tests/test_gpu_whitted.py's case with such a
    # mesh sets the name to prt_restatement.getBSDF, which applies Triangle.getShadingGeometry first and is the same function elsewhere.)
    bsdf = getBSDF(isect)                                          # :32
    p = bsdf.p                                                     # :35  bsdf.dgShading.p
    n = bsdf.nn                                                    # :36  bsdf.dgShading.nn
    wo = -ray.d                                                    # :37
    L = L + isect_Le(isect, wo)                                    # :40
    for light in scene.lights:                                     # :43
        # :47-48  new LightSample.random(rng) (light_sample.dart:46-51): uPos is a Float32List
        uPos0 = f32(rng.randomFloat())
        uPos1 = f32(rng.randomFloat())
        uComponent = rng.randomFloat()
        Li, wi, pdf, shadow = light.sampleLAtPoint(p, isect.rayEpsilon, (uPos0, uPos1), uComponent)
        if Li.isBlack() or pdf == 0.0:                             # :50-52
            continue
        f = bsdf.f(wo, wi, BSDF_ALL)                               # :54  the default flags
        if not f.isBlack() and not scene.bvh.intersectP(shadow):   # :56  visibility.unoccluded(scene)
            T = RGB(1.0)                                           # :58  visibility.transmittance: no VolumeRegion
            L = L + f * Li * AbsDot(wi, n) * T / pdf               # :57-58
    if ray.depth + 1 < maxDepth:                                   # :62
        L = L + SpecularReflect(ray, bsdf, rng, isect, scene, maxDepth)    # :64-65
        L = L + SpecularTransmit(ray, bsdf, rng, isect, scene, maxDepth)   # :67-68
    return L


# ---------------------------------------------------------------------------------------------------------------
# core/integrator.dart:187-231 / :233-290 (the ray differentials, :203-222 / :250-281, feed nothing on this path: no textures)
# ---------------------------------------------------------------------------------------------------------------
def SpecularReflect(ray, bsdf, rng, isect, scene, maxDepth):
    wo = -ray.d                                                    # :190
    p = bsdf.p                                                     # :193
    n = bsdf.nn                                                    # :194
    bs = (f32(rng.randomFloat()), f32(rng.randomFloat()), rng.randomFloat())   # :195  BSDFSample.random (bsdf_sample.dart:37-42)
    f, wi, pdf, _ = bsdf.sample_f(wo, (bs[0], bs[1]), bs[2], BSDF_REFLECTION | BSDF_SPECULAR)   # :195-196
    L = RGB(0.0)                                                   # :197
    if pdf > 0.0 and not f.isBlack() and AbsDot(wi, n) != 0.0:     # :199
        rd = Ray(p, wi, isect.rayEpsilon, INFINITY, ray.depth + 1)  # :201-202  RayDifferential.child
        Li = RendererLi(scene, rd, rng, maxDepth)                  # :225
        L = f * Li * (AbsDot(wi, n) / pdf)                         # :226
    return L


def SpecularTransmit(ray, bsdf, rng, isect, scene, maxDepth):
    wo = -ray.d                                                    # :236
    p = bsdf.p                                                     # :239
    n = bsdf.nn                                                    # :240
    bs = (f32(rng.randomFloat()), f32(rng.randomFloat()), rng.randomFloat())   # :241
    f, wi, pdf, _ = bsdf.sample_f(wo, (bs[0], bs[1]), bs[2], BSDF_TRANSMISSION | BSDF_SPECULAR)   # :241-242
    L = RGB(0.0)                                                   # :243
    if pdf > 0.0 and not f.isBlack() and AbsDot(wi, n) != 0.0:     # :245
        rd = Ray(p, wi, isect.rayEpsilon, INFINITY, ray.depth + 1)  # :247-248
        Li = RendererLi(scene, rd, rng, maxDepth)                  # :284
        L = f * Li * (AbsDot(wi, n) / pdf)                         # :285
    return L


def RendererLi(scene, ray, rng, maxDepth):
    """SamplerRenderer.Li (sampler_renderer.dart:67-98): the surface integrator at the hit, else the lights' Le along the ray; the
    volume integrator transmits 1 and adds 0."""
    isect = scene.bvh.intersect(ray)                               # :84
    if isect is not None:
        Li = WhittedLi(scene, ray, isect, rng, maxDepth)           # :85
    else:
        Li = RGB(0.0)                                              # :87
        for light in scene.lights:                                 # :89-91
            Li = Li + light.Le(ray)
    return RGB(1.0) * Li + RGB(0.0)                                # :97  T * Li + Lvi


def sample_Li(scene, camera, px, py, sv, rng, maxDepth):
    """One camera sample: generateRayDifferential, Li, * rayWeight, the guards (sampler_renderer.dart:160-193) -> (Ls, imageX, imageY)."""
    imageX = px + float(sv[0])                                     # montecarlo.dart:451-452
    imageY = py + float(sv[1])
    ray = camera.generateRay(imageX, imageY, float(sv[2]), float(sv[3]))
    Ls = RendererLi(scene, ray, rng, maxDepth) * 1.0
    if Ls.hasNaNs():
        Ls = RGB(0.0)
    elif Ls.luminance() < -1e-5:
        Ls = RGB(0.0)
    elif math.isinf(Ls.luminance()):
        Ls = RGB(0.0)
    return Ls, imageX, imageY


def render(scene, camera, film_desc, maxDepth, spp, pixels, vectors, rng_of):
    """The film of the samples `vectors` ([len(pixels) * spp][nFloats], a pixel's samples adjacent) of the raster pixels `pixels`, in
    that order; rng_of(px, py, i) is the draw source of sample i of pixel (px, py).  A pixel's samples reach the film after all of
    them were traced (sampler_renderer.dart:199-203).  -> [H][W][4] f32: X, Y, Z, weightSum."""
    film = dr.ImageFilm(film_desc.xResolution, film_desc.yResolution, film_desc.filter.xWidth, film_desc.filter.yWidth, film_desc.filterTable)
    for k, (px, py) in enumerate(np.asarray(pixels).reshape(-1, 2)):
        pending = []
        for i in range(spp):
            L, ix, iy = sample_Li(scene, camera, int(px), int(py), vectors[k * spp + i], rng_of(int(px), int(py), i), maxDepth)
            pending.append((ix, iy, L))
        for a in pending:
            film.addSample(*a)
    H, W = film_desc.yResolution, film_desc.xResolution
    lx = np.array(film.Lxyz, np.float32).reshape(H, W, 3)
    return np.concatenate([lx, np.array(film.weightSum, np.float32).reshape(H, W, 1)], axis=2)


def keyed_rng(seed, extent):
    """DESIGN.md 2.12 in Python: the draws of sample i of pixel (px, py) are the randomFloat() of the stream keyed
    (seed, pixelIndex, i, kind 2), read in the order the walk draws them.  extent: the sampler extent (x0, x1, y0, y1)."""
    return lambda px, py, i: rr.RNG(rr.counter_key(seed, rr.pixel_index(extent, px, py), i, rr.LI_KIND))
