"""RandomSampler.getMoreSamples (samplers/random_sampler.dart:47-88, FULL_SAMPLING) restated in plain Python: the test side's own
reading of the reference and of the stream contract of DESIGN.md 2.11, written apart from dartray_amd.core and from the kernels.  It
carries its own few lines of the generator (dart:math Random as core/rng.dart:27-43 uses it) and of the counter
key, so nothing here is shared with the code under test.

Cited by file.dart:line of the reference.  A "Float32List" here is a numpy float32 array: a store rounds the f64 value to f32.

Two ways to feed it: `keyed_vectors` (the device mode: one stream per (pixel, sample), kind 6) and `RandomSampler` driven by one
serial RNG (the reference's own: getMoreSamples called until it answers 0).
"""
import math

import numpy as np

_M64 = (1 << 64) - 1
STREAM_KIND = 6   # DESIGN.md 2.11 (1: LD blocks, 2: inside Li, 3 / 4: stratified, 5: Halton)
LI_KIND = 2


def _mix64(n):                                                     # Thomas Wang's 64-bit mix (dart:math Random's seeding; the counter key)
    n = ((~n) + (n << 21)) & _M64
    n ^= n >> 24
    n = (n * 265) & _M64
    n ^= n >> 14
    n = (n * 21) & _M64
    n ^= n >> 28
    return (n + (n << 31)) & _M64


class RNG:
    """core/rng.dart:27-43 over dart:math Random(seed): multiply-with-carry, A = 0xffffda61, four warm-up steps."""

    def __init__(self, seed):
        n = _mix64(seed & _M64) or 0x5A17
        self.lo, self.hi = n & 0xffffffff, n >> 32
        for _ in range(4):
            self._next()

    def _next(self):
        s = (0xffffda61 * self.lo + self.hi) & _M64
        self.lo, self.hi = s & 0xffffffff, s >> 32

    def randomFloat(self):                                         # rng.dart:36-38: Random.nextDouble(), 26 + 27 bits of two steps
        self._next()
        a = self.lo & ((1 << 26) - 1)
        self._next()
        return (a * float(1 << 27) + (self.lo & ((1 << 27) - 1))) / float(1 << 53)


def counter_key(seed, a, b, kind):                                 # the key of stream `kind` of (a, b)
    h = _mix64((seed & _M64) ^ 0x9E3779B97F4A7C15)
    h = _mix64(h ^ ((a * 0xD1B54A32D192ED03 + kind) & _M64))
    h = _mix64(h ^ ((b * 0x8CB92BA72F3D8DD7 + 0x5851F42D4C957F2D) & _M64))
    return h & 0x7fffffffffffffff


def draw_sample(px, py, n1D, n2D, rng):
    """random_sampler.dart:67-84 for one sample of the pixel (px, py).  Returns (vector, imageXY): the vector [nFloats] f32 in the sample
    vector's field order (imageU, imageV, lensU, lensV, time, oneD..., twoD...) with the image sample as the f32 of its fraction inside the
    pixel and time raw (the Lerp of :71 over the shutter is the consumer's); imageXY the reference's own doubles of :67-68."""
    ux, uy = rng.randomFloat(), rng.randomFloat()                  # :67-68
    lensU, lensV = rng.randomFloat(), rng.randomFloat()            # :69-70
    time = rng.randomFloat()                                       # :71
    oneD = [np.zeros(n, np.float32) for n in n1D]                  # Float32Lists (sample.dart)
    twoD = [np.zeros(2 * n, np.float32) for n in n2D]
    for i in range(len(n1D)):                                      # :74-78
        for j in range(n1D[i]):
            oneD[i][j] = rng.randomFloat()
    for i in range(len(n2D)):                                      # :80-84
        for j in range(2 * n2D[i]):
            twoD[i][j] = rng.randomFloat()
    head = np.array([ux, uy, lensU, lensV, time], np.float32)      # the one rounding of this project's vector
    return np.concatenate([head] + oneD + twoD), (ux + px, uy + py)


class RandomSampler:
    """random_sampler.dart:31-107 as written, FULL_SAMPLING, over a given pixel list (the PixelSampler's)."""

    def __init__(self, pixels, ns):
        self.pixels = [tuple(int(v) for v in p) for p in np.asarray(pixels).reshape(-1, 2)]
        self.samplesPerPixel = ns
        self.pixelIndex = 0                                        # :39-40
        self.sampleCount = 0

    def getMoreSamples(self, n1D, n2D, rng):
        """:47-88 -> (pixel, [numSamples][nFloats] f32) or None for the reference's 0."""
        if self.pixelIndex >= len(self.pixels):                    # :50-56
            self.sampleCount += 1
            if self.sampleCount >= self.samplesPerPixel:
                return None
            self.pixelIndex = 0
        pixel = self.pixels[self.pixelIndex]                       # :58
        self.pixelIndex += 1
        numSamples = self.samplesPerPixel                          # :61-63, mode == FULL_SAMPLING
        return pixel, np.stack([draw_sample(pixel[0], pixel[1], n1D, n2D, rng)[0] for _ in range(numSamples)])


def serial_vectors(pixels, spp, n1D, n2D, rng):
    """The reference's mode: ONE rng through getMoreSamples until it answers 0 (no draws inside Li: DirectLighting, or a path of depth
    <= 2).  Returns (pixel_xy [ncalls][2], vectors [ncalls * spp][nFloats]): as written the sampler walks the pixel list spp times."""
    s = RandomSampler(pixels, spp)
    xy, vecs = [], []
    while True:
        got = s.getMoreSamples(n1D, n2D, rng)
        if got is None:
            return np.array(xy, np.int32).reshape(-1, 2), np.concatenate(vecs)
        xy.append(got[0])
        vecs.append(got[1])


def sample_extent(film):                                           # image_film.dart:247-252
    return (math.floor(film.left + 0.5 - film.filter.xWidth), math.ceil(film.left + 0.5 + film.width + film.filter.xWidth),
            math.floor(film.top + 0.5 - film.filter.yWidth), math.ceil(film.top + 0.5 + film.height + film.filter.yWidth))


def pixel_index(extent, px, py):
    """A pixel's position in the FULL sampler extent, row by row."""
    return (int(py) - extent[2]) * (extent[1] - extent[0]) + (int(px) - extent[0])


def keyed_vectors(seed, extent, pixels, spp, n1D, n2D):
    """The device mode for the raster pixels `pixels`: sample i of a pixel draws from the stream keyed (seed, pixelIndex, i, kind 6).
    extent: the sampler extent (x0, x1, y0, y1).  Returns [len(pixels) * spp][nFloats] f32, a pixel's samples adjacent."""
    out = []
    for px, py in np.asarray(pixels).reshape(-1, 2):
        idx = pixel_index(extent, px, py)
        for i in range(spp):
            out.append(draw_sample(int(px), int(py), n1D, n2D, RNG(counter_key(seed, idx, i, STREAM_KIND)))[0])
    return np.stack(out)


def li_stream_tail(seed, extent, pixels, spp, max_tail):
    """The first max_tail randomFloat() of every sample's in-Li stream (kind 2 of (pixelIndex, i)): [npix * spp][max_tail] f64."""
    out = np.zeros((len(pixels) * spp, max(1, max_tail)), np.float64)
    for k, (px, py) in enumerate(np.asarray(pixels).reshape(-1, 2)):
        idx = pixel_index(extent, px, py)
        for i in range(spp):
            r = RNG(counter_key(seed, idx, i, LI_KIND))
            for t in range(max_tail):
                out[k * spp + i, t] = r.randomFloat()
    return out


def slot_counts(integrator_kind, light_nsamples):
    """(n1D, n2D) the integrators request, in request order (path_integrator.dart:37-47, direct_lighting_integrator.dart:70-96,
    emission_integrator.dart's two 1-D slots); integrator_kind as DR_INTEGRATOR_*: 0 = direct "all", 1 = path, 2 = direct "one".
    RandomSampler.roundSize is the identity (:90-92): a light's nsamples as given."""
    if integrator_kind == 1:
        return [1] * 14, [1] * 9
    if integrator_kind == 2:
        return [1] * 5, [1] * 2
    a = [n for k in light_nsamples for n in (k, k)]
    return a + [1, 1], list(a)


def need_tail(integrator_kind, max_depth, nlights):
    """In-Li draws a path can make at most: per bounce from the fourth vertex on 7 for the light sample + 3 for the BSDF sample,
    and one Russian-roulette draw per bounce beyond the third (path_integrator.dart:60-130)."""
    if integrator_kind != 1 or max_depth < 3:
        return 0
    per_nee = 7 if nlights > 0 else 0
    return (max_depth - 2) * (per_nee + 3) + max(0, max_depth - 3)
