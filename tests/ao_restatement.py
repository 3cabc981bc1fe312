"""AmbientOcclusionIntegrator.Li (surface_integrators/ambient_occlusion_integrator.dart:28-53) restated in plain Python line by line -- the
test side's own reading of the reference, on top of the intersection, getBSDF and intersectP of tests/golden/dart_restatement.py and the keyed
streams of tests/random_restatement.py (both imported, not copied).

Cited by file.dart:line of the reference.  The two rng.randomUint() of the scramble come from the `rng` the caller hands in (anything with
randomUint()).  DESIGN.md 2.13 makes them draws 0 and 1 of the sample's keyed in-Li stream (`keyed_rng`: dart_restatement's generator, which
has randomUint, seeded with random_restatement's key)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import dart_restatement as dr  # noqa: E402
from dart_restatement import INFINITY, RGB, Dot, Ray, RoundUpPow2, Sobol2, UniformSampleSphere, VanDerCorput, Vec, getBSDF  # noqa: E402,F401
import random_restatement as rr  # noqa: E402


def Sample02(n, scramble):                                         # montecarlo.dart:507-511
    return VanDerCorput(n, scramble[0]), Sobol2(n, scramble[1])


def FaceForward(n, n2):                                            # normal.dart:59-61
    return -n if Dot(n, n2) < 0.0 else n


class AmbientOcclusionIntegrator:
    def __init__(self, ns=2048, minDist=1.0e-4, maxDist=INFINITY):  # :24-26, defaults of Create :55-60
        self.nSamples = RoundUpPow2(ns)
        self.minDist, self.maxDist = minDist, maxDist

    def Li(self, scene, ray, isect, rng):
        bsdf = getBSDF(isect)                                      # :31
        p = bsdf.p                                                 # :32  bsdf.dgShading.p
        n = FaceForward(isect.dg.nn, -ray.d)                       # :33
        scramble = [rng.randomUint(), rng.randomUint()]            # :35
        nClear = 0                                                 # :37
        for i in range(self.nSamples):                             # :38
            u = Sample02(i, scramble)                              # :39
            w = UniformSampleSphere(u[0], u[1])                    # :40
            if Dot(w, n) < 0.0:                                    # :41-43
                w = -w
            r = Ray(p, w, self.minDist, self.maxDist)              # :45
            if not scene.bvh.intersectP(r):                        # :47-49
                nClear += 1
        return RGB(nClear / self.nSamples)                         # :52


def RendererLi(scene, integrator, ray, rng):
    """SamplerRenderer.Li (sampler_renderer.dart:67-98): the surface integrator at the hit, else the lights' Le along the ray; the
    volume integrator transmits 1 and adds 0."""
    isect = scene.bvh.intersect(ray)                               # :84
    if isect is not None:
        Li = integrator.Li(scene, ray, isect, rng)                 # :85
    else:
        Li = RGB(0.0)                                              # :87
        for light in scene.lights:                                 # :89-91
            Li = Li + light.Le(ray)
    return RGB(1.0) * Li + RGB(0.0)                                # :97  T * Li + Lvi


def sample_Li(scene, integrator, camera, px, py, sv, rng):
    """One camera sample: generateRayDifferential, Li, * rayWeight, the guards (sampler_renderer.dart:160-193) -> (Ls, imageX, imageY)."""
    imageX = px + float(sv[0])                                     # montecarlo.dart:451-452
    imageY = py + float(sv[1])
    ray = camera.generateRay(imageX, imageY, float(sv[2]), float(sv[3]))
    Ls = RendererLi(scene, integrator, ray, rng) * 1.0
    if Ls.hasNaNs():
        Ls = RGB(0.0)
    elif Ls.luminance() < -1e-5:
        Ls = RGB(0.0)
    elif math.isinf(Ls.luminance()):
        Ls = RGB(0.0)
    return Ls, imageX, imageY


def render(scene, integrator, camera, film_desc, spp, pixels, vectors, rng_of):
    """The film of the samples `vectors` ([len(pixels) * spp][nFloats], a pixel's samples adjacent) of the raster pixels `pixels`, in
    that order; rng_of(px, py, i) is the draw source of sample i of pixel (px, py).  A pixel's samples reach the film after all of
    them were traced (sampler_renderer.dart:199-203).  -> [H][W][4] f32: X, Y, Z, weightSum."""
    film = dr.ImageFilm(film_desc.xResolution, film_desc.yResolution, film_desc.filter.xWidth, film_desc.filter.yWidth, film_desc.filterTable)
    for k, (px, py) in enumerate(np.asarray(pixels).reshape(-1, 2)):
        pending = []
        for i in range(spp):
            L, ix, iy = sample_Li(scene, integrator, camera, int(px), int(py), vectors[k * spp + i], rng_of(int(px), int(py), i))
            pending.append((ix, iy, L))
        for a in pending:
            film.addSample(*a)
    H, W = film_desc.yResolution, film_desc.xResolution
    lx = np.array(film.Lxyz, np.float32).reshape(H, W, 3)
    return np.concatenate([lx, np.array(film.weightSum, np.float32).reshape(H, W, 1)], axis=2)


def keyed_rng(seed, extent):
    """DESIGN.md 2.13 in Python: the draws of sample i of pixel (px, py) are those of the stream keyed (seed, pixelIndex, i, kind 2), read
    in the order Li draws them.  extent: the sampler extent (x0, x1, y0, y1)."""
    return lambda px, py, i: dr.RNG(rr.counter_key(seed, rr.pixel_index(extent, px, py), i, rr.LI_KIND))
