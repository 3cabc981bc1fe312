"""StratifiedSampler.getMoreSamples restated in plain Python (the test side's own reading of the reference, written
apart from dartray_amd.core and from the kernels), on top of tests/golden/dart_restatement.py's DartRandom / RNG / Shuffle.

Cited by file.dart:line of the reference, as dart_restatement.py does.  A "Float32List" here is a numpy float32 array:
a store rounds the f64 expression to f32, an element-wise `+=` rounds the f32 sum to f32.

Two ways to feed it: `keyed_vectors` (the device mode: per-pixel and per-sample DartRandom streams seeded by the counter
key) and `serial_vectors` (the reference's own: one RNG(taskNum) for everything).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from dart_restatement import RNG, DartRandom, Shuffle  # noqa: E402

from montecarlo_restatement import ONE_MINUS_EPSILON, LatinHypercube  # noqa: E402,F401  (shared with halton_restatement.py)

_M64 = (1 << 64) - 1


def StratifiedSample1D(samples, nSamples, rng, jitter=True):      # montecarlo.dart:270-277
    invTot = 1.0 / nSamples
    for i in range(nSamples):
        delta = rng.randomFloat() if jitter else 0.5
        samples[i] = min((i + delta) * invTot, ONE_MINUS_EPSILON)


def StratifiedSample2D(samples, nx, ny, rng, jitter=True):        # montecarlo.dart:279-292
    dx, dy = 1.0 / nx, 1.0 / ny
    si = 0
    for y in range(ny):
        for x in range(nx):
            jx = rng.randomFloat() if jitter else 0.5
            jy = rng.randomFloat() if jitter else 0.5
            samples[si] = min((x + jx) * dx, ONE_MINUS_EPSILON)
            samples[si + 1] = min((y + jy) * dy, ONE_MINUS_EPSILON)
            si += 2


def get_more_samples(px, py, xs, ys, jitter, n1D, n2D, pixel_rng, sample_rng):
    """stratified_sampler.dart:80-121 for the pixel (px, py).  Returns (vectors, imageXY): vectors [spp][nFloats] f32 in
    the sample vector's field order (imageU, imageV, lensU, lensV, time, oneD..., twoD...) with the image sample as the
    fraction the C ABI stores, f32(imageX) - px, and imageXY [spp][2] the reference's own imageX / imageY (f32 values).
    pixel_rng: the stream of :85-104; sample_rng(i): the stream of sample i's :114-120."""
    n = xs * ys
    imageSamples = np.zeros(2 * n, np.float32)                     # :51-53
    lensSamples = np.zeros(2 * n, np.float32)
    timeSamples = np.zeros(n, np.float32)
    StratifiedSample2D(imageSamples, xs, ys, pixel_rng, jitter)    # :85-92
    StratifiedSample2D(lensSamples, xs, ys, pixel_rng, jitter)
    StratifiedSample1D(timeSamples, n, pixel_rng, jitter)
    for o in range(0, 2 * n, 2):                                   # :97-100 (inside the Float32List)
        imageSamples[o] += np.float32(px)
        imageSamples[o + 1] += np.float32(py)
    Shuffle(lensSamples, 0, n, 2, pixel_rng)                       # :103-104
    Shuffle(timeSamples, 0, n, 1, pixel_rng)
    nf = 5 + sum(n1D) + 2 * sum(n2D)
    vec = np.zeros((n, nf), np.float32)
    xy = np.zeros((n, 2), np.float64)
    for i in range(n):                                             # :107-121
        xy[i] = (imageSamples[2 * i], imageSamples[2 * i + 1])
        vec[i, 0] = imageSamples[2 * i] - np.float32(px)           # exact in f32 (the two are within one of each other)
        vec[i, 1] = imageSamples[2 * i + 1] - np.float32(py)
        vec[i, 2], vec[i, 3] = lensSamples[2 * i], lensSamples[2 * i + 1]
        vec[i, 4] = timeSamples[i]                                 # (the Lerp over the shutter happens in the consumer)
        rng, o = sample_rng(i), 5
        for c in n1D:
            buf = np.zeros(c, np.float32)
            LatinHypercube(buf, c, 1, rng)
            vec[i, o:o + c] = buf
            o += c
        for c in n2D:
            buf = np.zeros(2 * c, np.float32)
            LatinHypercube(buf, c, 2, rng)
            vec[i, o:o + 2 * c] = buf
            o += 2 * c
    return vec, xy


def _mix64(n):                                                     # the product's dr_mix64 (csrc/dr_rng.h), public constants
    n = ((~n) + (n << 21)) & _M64
    n ^= n >> 24
    n = (n * 265) & _M64
    n ^= n >> 14
    n = (n * 21) & _M64
    n ^= n >> 28
    return (n + (n << 31)) & _M64


def counter_key(seed, a, b, kind):                                 # dr_counter_key; the tests compare it with the oracle's orc_counter_key
    h = _mix64((seed & _M64) ^ 0x9E3779B97F4A7C15)
    h = _mix64(h ^ ((a * 0xD1B54A32D192ED03 + kind) & _M64))
    h = _mix64(h ^ ((b * 0x8CB92BA72F3D8DD7 + 0x5851F42D4C957F2D) & _M64))
    return h & 0x7fffffffffffffff


def keyed_rng(seed, a, b, kind):
    r = RNG(0)
    r.random = DartRandom(counter_key(seed, a, b, kind))
    return r


def sample_extent(film):                                           # image_film.dart:247-252
    import math
    return (math.floor(film.left + 0.5 - film.filter.xWidth), math.ceil(film.left + 0.5 + film.width + film.filter.xWidth),
            math.floor(film.top + 0.5 - film.filter.yWidth), math.ceil(film.top + 0.5 + film.height + film.filter.yWidth))


def keyed_vectors(film, pixels, xs, ys, jitter, seed, n1D, n2D):
    """The device mode for the raster pixels `pixels`: stream kind 3 of (pixelIndex, 0) per pixel, kind 4 of
    (pixelIndex, i) per sample; pixelIndex counts the FULL sampler extent row by row."""
    e = sample_extent(film)
    vecs, xys = [], []
    for px, py in np.asarray(pixels).reshape(-1, 2):
        idx = (int(py) - e[2]) * (e[1] - e[0]) + (int(px) - e[0])
        v, xy = get_more_samples(int(px), int(py), xs, ys, jitter, n1D, n2D, keyed_rng(seed, idx, 0, 3),
                                 lambda i: keyed_rng(seed, idx, i, 4))
        vecs.append(v)
        xys.append(xy)
    return np.concatenate(vecs), np.concatenate(xys)


def serial_vectors(pixels, xs, ys, jitter, n1D, n2D, rng):
    """The reference's mode: ONE rng through every pixel in order (no draws inside Li: DirectLighting, or a path of depth <= 2)."""
    vecs, xys = [], []
    for px, py in np.asarray(pixels).reshape(-1, 2):
        v, xy = get_more_samples(int(px), int(py), xs, ys, jitter, n1D, n2D, rng, lambda i: rng)
        vecs.append(v)
        xys.append(xy)
    return np.concatenate(vecs), np.concatenate(xys)


def li_stream_tail(seed, film, pixels, spp, max_tail):
    """The first max_tail randomFloat() of every sample's in-Li stream (kind 2 of (pixelIndex, i)): [npix * spp][max_tail] f64."""
    e = sample_extent(film)
    out = np.zeros((len(pixels) * spp, max(1, max_tail)), np.float64)
    for k, (px, py) in enumerate(np.asarray(pixels).reshape(-1, 2)):
        idx = (int(py) - e[2]) * (e[1] - e[0]) + (int(px) - e[0])
        for i in range(spp):
            r = keyed_rng(seed, idx, i, 2)
            for t in range(max_tail):
                out[k * spp + i, t] = r.randomFloat()
    return out


def slot_counts(integrator_kind, light_nsamples):
    """(n1D, n2D) the integrators request, in request order (path_integrator.dart:37-47, direct_lighting_integrator.dart:70-96,
    emission_integrator.dart's two 1-D slots); integrator_kind as DR_INTEGRATOR_*: 0 = direct "all", 1 = path, 2 = direct "one"."""
    if integrator_kind == 1:
        return [1] * 14, [1] * 9
    if integrator_kind == 2:
        return [1] * 5, [1] * 2
    a = [n for k in light_nsamples for n in (k, k)]
    return a + [1, 1], list(a)


def need_tail(integrator_kind, max_depth, nlights):
    """In-Li draws a path can make (the product's planRender: P.needTail)."""
    if integrator_kind != 1 or max_depth < 3:
        return 0
    per_nee = 7 if nlights > 0 else 0
    return (max_depth - 2) * (per_nee + 3) + max(0, max_depth - 3)
