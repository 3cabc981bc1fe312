"""lib/samplers/ and lib/pixel_samplers/ (with core/rng.dart and the montecarlo.dart helpers they draw with).  A sampler's to_abi(d)
writes its mode into the DrRenderDesc and returns the arrays that must outlive the call."""
import math

import numpy as np

from .. import _abi


def RoundUpPow2(v):  # common.dart:113-123
    v -= 1
    v |= v >> 1
    v |= v >> 2
    v |= v >> 4
    v |= v >> 8
    v |= v >> 16
    return v + 1


class DartRandom:
    """dart:math Random(seed) of the Dart VM as used by core/rng.dart:27-43 (multiply-with-carry, A = 0xffffda61,
    Thomas-Wang seeding, four warm-up steps) -- host side only: the pixel samplers below shuffle
    with their own RNG(5489)."""
    _M64 = (1 << 64) - 1

    def __init__(self, seed=5489):
        n = seed & self._M64
        n = ((~n) + (n << 21)) & self._M64
        n ^= n >> 24
        n = (n * 265) & self._M64
        n ^= n >> 14
        n = (n * 21) & self._M64
        n ^= n >> 28
        n = (n + (n << 31)) & self._M64
        n = n or 0x5A17
        self.lo, self.hi = n & 0xffffffff, n >> 32
        for _ in range(4):
            self._step()

    def _step(self):
        s = (0xffffda61 * self.lo + self.hi) & self._M64
        self.lo, self.hi = s & 0xffffffff, s >> 32

    def randomUint(self):  # Random.nextInt(0xffffffff): only lo == 0xffffffff is rejected
        while True:
            self._step()
            if self.lo != 0xffffffff:
                return self.lo

    def randomFloat(self):  # Random.nextDouble(): 26 + 27 bits from two steps
        self._step()
        a = self.lo & ((1 << 26) - 1)
        self._step()
        return (a * 134217728.0 + (self.lo & ((1 << 27) - 1))) / 9007199254740992.0


def GetSubWindow(w, h, num, count):  # common.dart:52-73 -> (x0, x1, y0, y1), from 0 as the reference computes them
    nx, ny = count, 1
    while (nx & 1) == 0 and 2 * w * ny < h * nx:
        nx >>= 1
        ny <<= 1
    xo, yo = num % nx, num // nx
    lerp = lambda t, v1, v2: v1 * (1.0 - t) + v2 * t
    return (math.floor(lerp(xo / nx, 0, w)), min(math.floor(lerp((xo + 1) / nx, 0, w)), w),
            math.floor(lerp(yo / ny, 0, h)), min(math.floor(lerp((yo + 1) / ny, 0, h)), h))


class LinearPixelSampler:
    """Pixels "linear" (pixel_samplers/linear_pixel_sampler.dart:29-40): rows top to bottom."""
    kind, tileSize, randomize = 0, 32, False

    def setup(self, x, y, width, height):
        ys, xs = np.meshgrid(np.arange(y, y + height, dtype=np.int32), np.arange(x, x + width, dtype=np.int32), indexing="ij")
        return np.stack([xs, ys], axis=-1).reshape(-1, 2)


class TilePixelSampler(LinearPixelSampler):
    """Pixels "tile" (tile_pixel_sampler.dart:33-100), the reference's default: tileSize^2 tiles in row-major order,
    shuffled (from tile 1 on, each with a uniformly drawn partner) by the sampler's own RNG(5489)."""
    kind = 1

    def __init__(self, tileSize=32, randomize=True):
        self.tileSize, self.randomize = int(tileSize), bool(randomize)

    def setup(self, x, y, width, height):
        ts = self.tileSize
        nx = width // ts + (0 if width % ts == 0 else 1)
        ny = height // ts + (0 if height % ts == 0 else 1)
        tiles = [(xi, yi) for yi in range(ny) for xi in range(nx)]
        if self.randomize:
            rng = DartRandom()
            for ti in range(1, len(tiles)):
                r = rng.randomUint() % len(tiles)
                tiles[ti], tiles[r] = tiles[r], tiles[ti]
        right, bottom = x + width - 1, y + height - 1
        out = []
        for tx, ty in tiles:
            sx, sy = x + tx * ts, y + ty * ts
            xs = np.arange(sx, min(sx + ts - 1, right) + 1, dtype=np.int32)
            ys = np.arange(sy, min(sy + ts - 1, bottom) + 1, dtype=np.int32)
            gy, gx = np.meshgrid(ys, xs, indexing="ij")
            out.append(np.stack([gx, gy], axis=-1).reshape(-1, 2))
        return np.concatenate(out) if out else np.zeros((0, 2), np.int32)


class RandomPixelSampler(LinearPixelSampler):
    """Pixels "random" (random_pixel_sampler.dart:27-58): the linear list, entry i swapped with a uniformly drawn one."""
    kind = 2

    def setup(self, x, y, width, height):
        p = LinearPixelSampler.setup(self, x, y, width, height).copy()
        rng = DartRandom()
        n = len(p)
        for i in range(n):
            l = rng.randomUint() % n
            p[[i, l]] = p[[l, i]]
        return p


class _Sampler:
    """What every sampler tells the C ABI (core/sampler.dart's samplesPerPixel, the seed of the device's keyed streams, and the mode
    that names its kernel): to_abi(d) writes them into the DrRenderDesc and returns the arrays d points into."""

    def to_abi(self, d):
        d.sampler_mode = self.sampler_mode
        d.spp = self.samplesPerPixel
        d.seed = self.seed
        return []

    @property
    def generatedSamplesPerPixel(self):
        """Vectors per pixel SamplerRenderer.generate_samples returns."""
        return self.samplesPerPixel

    def slot_counts(self, renderer, scene):
        """(n1D, n2D): entries of the 1-D and 2-D sample slots the integrators request of this sampler, in request order."""
        return renderer.requestSamples(self, scene)


class LowDiscrepancySampler(_Sampler):
    """samplers/low_discrepancy_sampler.dart:32-88.  The reference threads ONE
    serial RNG through sampler and integrator (sampler_renderer.dart:137); on
    the device every (pixel, LD block) owns a keyed stream instead
    (DR_SAMPLER_COUNTER), or the caller supplies recorded sample vectors
    (HostBufferSampler)."""

    def __init__(self, camera, nsamp=4, seed=5489, pixels=None):
        self.camera = camera
        self.samplesPerPixel = RoundUpPow2(int(nsamp))
        self.seed = int(seed)
        # PixelSampler: the ORDER in which pixels are sampled only matters to the serial reference stream (which RNG
        # numbers a pixel gets); the device's keyed streams give every pixel the same samples in any order
        self.pixelSampler = pixels or LinearPixelSampler()

    sampler_mode = _abi.DR_SAMPLER_COUNTER

    def roundSize(self, size):
        return RoundUpPow2(size)


ONE_MINUS_EPSILON = 0.9999999403953552  # montecarlo.dart:23


def _latin_hypercube_slots(n1D, n2D, rng):
    """LatinHypercube (montecarlo.dart:305-325) of every 1-D slot, then of every 2-D slot, drawn from rng -> their f32 values in the C ABI's field order."""
    out = []
    for n, dims in [(n, 1) for n in n1D] + [(n, 2) for n in n2D]:
        v = np.zeros((n, dims), np.float32)
        for j in range(n):
            for d in range(dims):
                v[j, d] = min((j + rng.randomFloat()) * (1.0 / n), ONE_MINUS_EPSILON)
        for d in range(dims):
            for j in range(n):
                other = j + rng.randomUint() % (n - j)
                v[j, d], v[other, d] = v[other, d], v[j, d]
        out.append(v.reshape(-1))
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def _pack_tails(tails):
    """The in-Li draws of every sample (lists of different lengths; possibly none) -> (tail [n, longest or 1] f64 zero filled, count [n])."""
    cnt = np.array([len(t) for t in tails], np.int32)
    tail = np.zeros((len(tails), max(1, int(cnt.max()) if len(cnt) else 1)), np.float64)
    for i, t in enumerate(tails):
        tail[i, :len(t)] = t
    return tail, cnt


def _serial_host_buffer(sampler, renderer, scene, li_draws, spp, walk):
    """What the samplers' serial_samples share: the reference's ONE RNG(taskNum) (sampler_renderer.dart:137) threaded through the sampler and
    through Li.  walk(n1D, n2D, rng) is the sampler's own loop: it yields one pixel_xy row at a time, (px, py, vectors [spp, nFloats]), in the stream's order,
    drawing from rng; behind every yield li_draws(px, py, vector, rng) -> the randomFloat() values Li draws for each of its vectors, taken from the same rng
    (the host has no integrator of its own to count them): required where the integrator's Li draws from that stream, unused otherwise.
    Returns the HostBufferSampler of the vectors and the recorded draws, at spp vectors per pixel_xy row."""
    recorded = renderer.surfaceIntegrator.li_draws_recorded
    if recorded and li_draws is None:
        raise ValueError("serial_samples: a PathIntegrator with maxDepth >= 3 draws inside Li; pass li_draws")
    n1D, n2D = sampler.slot_counts(renderer, scene)
    rng = DartRandom(renderer.taskNum)
    pixels, vecs, tails = [], [], []
    for px, py, v in walk(n1D, n2D, rng):
        pixels.append((px, py))
        vecs.append(v)
        if recorded:
            tails += [list(li_draws(px, py, row, rng)) for row in v]
    tail, cnt = _pack_tails(tails) if recorded else (None, None)
    nf = 5 + sum(n1D) + 2 * sum(n2D)
    return HostBufferSampler(sampler.camera, spp, np.array(pixels, np.int32).reshape(-1, 2),
                             np.concatenate(vecs) if vecs else np.zeros((0, nf), np.float32), tail, cnt)


class StratifiedSampler(_Sampler):
    """samplers/stratified_sampler.dart:38-128: xsamples x ysamples jittered strata per pixel for the image and the lens
    sample, xsamples * ysamples strata for the time sample, the lens and time samples shuffled, and a LatinHypercube per
    integrator slot.  On the device (DR_SAMPLER_STRATIFIED / _NOJITTER) every pixel and every sample owns a keyed stream
    (DESIGN.md 2.7); serial_samples() walks the reference's ONE serial RNG(taskNum) instead and
    returns the vectors as a HostBufferSampler.  The device needs xsamples * ysamples to be a power of two."""

    def __init__(self, camera, xsamples=2, ysamples=2, jitter=True, seed=5489, pixels=None):
        self.camera = camera
        self.xPixelSamples, self.yPixelSamples = int(xsamples), int(ysamples)
        if self.xPixelSamples < 1 or self.yPixelSamples < 1:
            raise ValueError("StratifiedSampler: xsamples and ysamples must be positive")
        self.samplesPerPixel = self.xPixelSamples * self.yPixelSamples
        self.jitterSamples = bool(jitter)
        self.seed = int(seed)
        self.pixelSampler = pixels or LinearPixelSampler()

    @property
    def sampler_mode(self):
        return _abi.DR_SAMPLER_STRATIFIED if self.jitterSamples else _abi.DR_SAMPLER_STRATIFIED_NOJITTER

    def to_abi(self, d):
        d.strat_xsamples = self.xPixelSamples
        return super().to_abi(d)

    def roundSize(self, size):  # :63-65
        return size

    def maximumSampleCount(self):  # :126-128
        return self.samplesPerPixel

    def pixel_samples(self, px, py, n1D, n2D, pixel_rng, sample_rng):
        """getMoreSamples (:67-124) for the pixel (px, py): [spp, 5 + sum(n1D) + 2 sum(n2D)] f32 in the C ABI's field order, the
        image sample as its fraction inside the pixel (f32(f32(u) + px) - px: the shift happens inside the Float32List, :97-100).
        pixel_rng draws the strata and the two shuffles; sample_rng(i) is the generator of sample i's LatinHypercube draws
        (the same object everywhere: the reference's serial stream)."""
        f32 = np.float32
        xs, ys, spp, jit = self.xPixelSamples, self.yPixelSamples, self.samplesPerPixel, self.jitterSamples

        def strat2d():  # StratifiedSample2D, montecarlo.dart:279-292
            out = np.zeros((spp, 2), f32)
            dx, dy = 1.0 / xs, 1.0 / ys
            for i in range(spp):
                x, y = i % xs, i // xs
                jx = pixel_rng.randomFloat() if jit else 0.5
                jy = pixel_rng.randomFloat() if jit else 0.5
                out[i] = (min((x + jx) * dx, ONE_MINUS_EPSILON), min((y + jy) * dy, ONE_MINUS_EPSILON))
            return out

        def shuffle(a):  # Shuffle, montecarlo.dart:294-303 (rows of `a` are the dims-tuples)
            for i in range(len(a)):
                other = i + pixel_rng.randomUint() % (len(a) - i)
                a[[i, other]] = a[[other, i]]

        image, lens = strat2d(), strat2d()
        time = np.zeros((spp, 1), f32)
        for i in range(spp):  # StratifiedSample1D, montecarlo.dart:270-277
            time[i, 0] = min((i + (pixel_rng.randomFloat() if jit else 0.5)) * (1.0 / spp), ONE_MINUS_EPSILON)
        fp = np.array([px, py], f32)
        image = (image + fp) - fp  # f32 arithmetic: the reference's imageX is f32(f32(u) + px)
        shuffle(lens)
        shuffle(time)
        nf = 5 + sum(n1D) + 2 * sum(n2D)
        vec = np.zeros((spp, nf), f32)
        vec[:, 0:2], vec[:, 2:4], vec[:, 4:5] = image, lens, time
        for i in range(spp):
            vec[i, 5:] = _latin_hypercube_slots(n1D, n2D, sample_rng(i))
        return vec

    def serial_samples(self, renderer, scene, li_draws=None):
        """The reference's own stream (_serial_host_buffer), pixel after pixel in the pixel sampler's order.  Returns a HostBufferSampler.
        li_draws(px, py, vector, rng): required for a PathIntegrator with maxDepth >= 3 (beyond its third vertex), unused otherwise."""
        def walk(n1D, n2D, rng):
            e = renderer.camera.film.getSampleExtent()
            x0, x1, y0, y1 = GetSubWindow(e[1] - e[0], e[3] - e[2], renderer.taskNum, max(1, renderer.taskCount))
            for px, py in self.pixelSampler.setup(x0, y0, x1 - x0, y1 - y0):
                yield int(px), int(py), self.pixel_samples(int(px), int(py), n1D, n2D, rng, lambda i: rng)
        return _serial_host_buffer(self, renderer, scene, li_draws, self.samplesPerPixel, walk)


class AdaptiveSampler(_Sampler):
    """samplers/adaptive_sampler.dart:36-220: every pixel gets minSamples low-discrepancy samples; a pixel whose samples' contrast
    exceeds 0.5 (needsSupersampling, method "contrast") is sampled again with maxSamples, and only that second set reaches the
    film.  On the device (DR_SAMPLER_ADAPTIVE) both passes are the LD sampler's keyed streams and the decision is a
    kernel.  The constructor applies the reference's rules (:40-83) in its order: swap, round each up to a power of two, at least two
    initial samples, more maximum than minimum samples."""

    METHODS = ("contrast", "shapeid")

    def __init__(self, camera, minsamples=4, maxsamples=32, method="contrast", seed=5489, pixels=None):
        if method == "shapeid":
            raise ValueError("AdaptiveSampler method 'shapeid' is not supported: the camera hit's shape and primitive ids are not "
                             "kept per sample on the device (method 'contrast' is)")
        if method != "contrast":
            raise ValueError("AdaptiveSampler method must be 'contrast' (got %r)" % (method,))
        self.camera = camera
        self.method = method
        mins, maxs = int(minsamples), int(maxsamples)
        if mins < 1 or maxs < 1:
            raise ValueError("AdaptiveSampler: minsamples and maxsamples must be positive")
        self.samplesPerPixel = RoundUpPow2(max(mins, maxs))  # the Sampler base class's count, from the arguments as given (:42-43)
        if mins > maxs:
            mins, maxs = maxs, mins
        self.minSamples = RoundUpPow2(mins)
        self.maxSamples = RoundUpPow2(maxs)
        if self.minSamples < 2:
            self.minSamples = 2
        if self.minSamples == self.maxSamples:
            self.maxSamples *= 2
        if self.minSamples > self.maxSamples:  # (maxsamples 1: the two initial samples exceed it and nothing in the reference mends that)
            raise ValueError("AdaptiveSampler needs more maximum than minimum samples (got minsamples %d, maxsamples %d)" % (int(minsamples), int(maxsamples)))
        if self.maxSamples > 4096:
            raise ValueError("AdaptiveSampler: maxsamples %d exceeds the device sampler's 4096" % self.maxSamples)
        self.seed = int(seed)
        self.pixelSampler = pixels or LinearPixelSampler()

    sampler_mode = _abi.DR_SAMPLER_ADAPTIVE

    def to_abi(self, d):
        keep = super().to_abi(d)
        d.spp = self.maxSamples
        d.strat_xsamples = self.minSamples  # (the field doubles as minSamples in this mode)
        return keep

    @property
    def generatedSamplesPerPixel(self):  # the first pass's
        return self.minSamples

    def roundSize(self, size):  # :93-95
        return RoundUpPow2(size)

    def maximumSampleCount(self):  # :97-99
        return self.maxSamples


def RadicalInverse(n, base):  # montecarlo.dart:327-339, as written: the next n is the truncated PRODUCT n * (1 / base)
    val = 0.0
    invBase = 1.0 / base
    invBi = invBase
    while n > 0:
        d_i = n % base
        val += d_i * invBi
        n = int(n * invBase)
        invBi *= invBase
    return val


def Lerp(t, v1, v2):  # common.dart:80-81
    return v1 * (1.0 - t) + v2 * t


class HaltonSampler(_Sampler):
    """samplers/halton_sampler.dart:31-104: ONE sequence per task over the task's window -- sample k lands where RadicalInverse(k, 3) /
    RadicalInverse(k, 2) put it in the delta x delta square over the window's corner (delta = max(width, height)) and is rejected when it
    falls outside the window, so pixels receive different numbers of samples; pixelsamples is any positive integer.  On the device
    (DR_SAMPLER_HALTON) the LatinHypercube draws of the integrator's slots and the draws inside Li come from streams keyed by
    k; serial_samples() walks the reference's ONE serial RNG(taskNum) instead and returns the vectors as a HostBufferSampler."""

    def __init__(self, camera, pixelsamples=4, seed=5489):
        self.camera = camera
        self.samplesPerPixel = int(pixelsamples)
        if self.samplesPerPixel < 1:
            raise ValueError("HaltonSampler: pixelsamples must be positive")
        self.seed = int(seed)

    sampler_mode = _abi.DR_SAMPLER_HALTON  # (spp = pixelsamples as given: nothing is rounded)

    def roundSize(self, size):  # :102-104
        return size

    def maximumSampleCount(self):  # :50-52
        return 1

    @staticmethod
    def window(renderer):
        """(left, top, width, height) of the renderer's task: GetSubWindow's extents of the sampler extent, as the reference hands them on."""
        e = renderer.camera.film.getSampleExtent()
        x0, x1, y0, y1 = GetSubWindow(e[1] - e[0], e[3] - e[2], renderer.taskNum, max(1, renderer.taskCount))
        return x0, y0, x1 - x0, y1 - y0

    def accepted(self, left, top, width, height):
        """The rejection loop (:63-83): yields (k, imageX, imageY) of every index of [0, pixelsamples * delta^2) inside the window."""
        if width <= 0 or height <= 0:
            return
        delta = max(width, height)
        right, bottom = left + width - 1, top + height - 1  # inclusive (sampler.dart:52-54)
        for k in range(self.samplesPerPixel * delta * delta):
            imageX = Lerp(RadicalInverse(k, 3), left, left + float(delta))
            imageY = Lerp(RadicalInverse(k, 2), top, top + float(delta))
            if imageX > right or imageY > bottom:
                continue
            yield k, imageX, imageY

    def sample_vector(self, k, imageX, imageY, n1D, n2D, rng):
        """(anchor pixel, vector) of the accepted index k in the C ABI's field order: the image sample as the f32 fraction behind
        floor(imageX / imageY), lens and time the radical inverses of k + 1 (the reference increments currentSample first, :76-89; time raw:
        the Lerp over the shutter is the consumer's), then LatinHypercube(oneD...), LatinHypercube(twoD...) drawn from rng (:91-97)."""
        f32 = np.float32
        px, py = math.floor(imageX), math.floor(imageY)
        vec = np.zeros(5 + sum(n1D) + 2 * sum(n2D), f32)
        vec[0:5] = (imageX - px, imageY - py, RadicalInverse(k + 1, 5), RadicalInverse(k + 1, 7), RadicalInverse(k + 1, 11))
        vec[5:] = _latin_hypercube_slots(n1D, n2D, rng)
        return (px, py), vec

    def serial_samples(self, renderer, scene, li_draws=None):
        """The reference's own stream: ONE RNG(taskNum) (sampler_renderer.dart:137) through the accepted samples' LatinHypercube draws and
        through Li, in index order.  Returns a HostBufferSampler at one sample per pixel_xy row (samples are not grouped by pixel).
        li_draws(px, py, vector, rng): as for StratifiedSampler.serial_samples."""
        def walk(n1D, n2D, rng):
            for k, imageX, imageY in self.accepted(*self.window(renderer)):
                xy, v = self.sample_vector(k, imageX, imageY, n1D, n2D, rng)
                yield xy[0], xy[1], v[None, :]
        return _serial_host_buffer(self, renderer, scene, li_draws, 1, walk)


class RandomSampler(_Sampler):
    """samplers/random_sampler.dart:31-107, FULL_SAMPLING: every value of a sample vector is one RNG.randomFloat() -- image x, image y,
    lens u, lens v, time, then the entries of every 1-D and of every 2-D slot in request order; nothing is stratified or shuffled.  On the
    device (DR_SAMPLER_RANDOM) every (pixel, sample) owns a keyed stream; serial_samples() walks the reference's ONE serial
    RNG(taskNum) instead and returns the vectors as a HostBufferSampler.  The device needs pixelsamples to be a power of two, at most 4096:
    the reference's default of 10 (Create, :94-101) has to be given as one."""

    def __init__(self, camera, pixelsamples=10, seed=5489, pixels=None):
        self.camera = camera
        self.samplesPerPixel = int(pixelsamples)
        if self.samplesPerPixel < 1:
            raise ValueError("RandomSampler: pixelsamples must be positive")
        self.seed = int(seed)
        self.pixelSampler = pixels or LinearPixelSampler()

    sampler_mode = _abi.DR_SAMPLER_RANDOM

    def to_abi(self, d):
        n = self.samplesPerPixel
        if n & (n - 1) or n > 4096:
            raise ValueError("RandomSampler: pixelsamples must be a power of two, at most 4096, on the device (got %d; the slot -> pixel "
                             "maps of the batches are shifts)" % n)
        return super().to_abi(d)

    def roundSize(self, size):  # :90-92
        return size

    def maximumSampleCount(self):  # :43-45
        return self.samplesPerPixel

    def pixel_samples(self, px, py, n1D, n2D, sample_rng):
        """The loop of getMoreSamples (:65-85) for one pixel: [spp, 5 + sum(n1D) + 2 sum(n2D)] f32 in the C ABI's field order, the image
        sample as the f32 of its fraction inside the pixel (the reference's imageX is the double u + px), time raw (the Lerp over the shutter
        is the consumer's).  sample_rng(i) is the generator of sample i's draws (the same object everywhere: the reference's serial stream)."""
        nf = 5 + sum(n1D) + 2 * sum(n2D)
        vec = np.zeros((self.samplesPerPixel, nf), np.float32)
        for i in range(self.samplesPerPixel):
            rng = sample_rng(i)
            for f in range(nf):  # (the field order is the draw order: image, lens, time, oneD..., twoD...)
                vec[i, f] = rng.randomFloat()
        return vec

    def serial_samples(self, renderer, scene, li_draws=None, passes=1):
        """The reference's own stream: ONE RNG(taskNum) (sampler_renderer.dart:137) threaded through the sampler, pixel after pixel in the
        pixel sampler's order, and through Li.  Returns a HostBufferSampler.  li_draws(px, py, vector, rng): as for
        StratifiedSampler.serial_samples.  passes: as written, getMoreSamples walks the pixel list samplesPerPixel times in FULL_SAMPLING
        (:50-56 count walks, :62 hands out samplesPerPixel samples per call); the device traces the first walk, the default here, and
        passes = samplesPerPixel continues the same stream through all of them (the pixel list repeats)."""
        def walk(n1D, n2D, rng):
            if not 1 <= int(passes) <= self.samplesPerPixel:  # (behind the shared helper's own refusal, where it always ran)
                raise ValueError("serial_samples: passes must be between 1 and samplesPerPixel")
            e = renderer.camera.film.getSampleExtent()
            x0, x1, y0, y1 = GetSubWindow(e[1] - e[0], e[3] - e[2], renderer.taskNum, max(1, renderer.taskCount))
            for px, py in np.concatenate([self.pixelSampler.setup(x0, y0, x1 - x0, y1 - y0)] * int(passes)):
                yield int(px), int(py), self.pixel_samples(int(px), int(py), n1D, n2D, lambda i: rng)
        return _serial_host_buffer(self, renderer, scene, li_draws, self.samplesPerPixel, walk)


class HostBufferSampler(_Sampler):
    """Explicit camera samples: pixel_xy [npix,2] int32, sample_vec [npix*spp, nfloats] f32
    (imageU, imageV, lensU, lensV, time, oneD..., twoD...), tail [npix*spp, max_tail] f64 =
    the RNG.randomFloat() values PathIntegrator.Li draws for bounces >= 3.  tail_count [npix*spp] (how many of its
    max_tail slots each sample actually drew: the oracle's recording has it) selects the PACKED form of the C ABI
    (DrRenderDesc.tail_offsets): only the drawn values cross the host link.  `seed`: read by a WhittedIntegrator render alone, whose
    LightSample.random draws are keyed streams, not a recorded tail."""

    def __init__(self, camera, spp, pixel_xy, sample_vec, tail=None, tail_count=None, seed=None):
        self.camera = camera
        self.samplesPerPixel = int(spp)
        self.li_seed = None if seed is None else int(seed)  # WhittedIntegrator only (required there: SamplerRenderer.describe): its draws inside Li are the keyed (pixel, sample) streams in every mode
        self.pixel_xy = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
        self.sample_vec = np.ascontiguousarray(sample_vec, dtype=np.float32)
        self.tail = None if tail is None else np.ascontiguousarray(tail, dtype=np.float64)
        self.tail_offsets = None
        if len(self.sample_vec) != len(self.pixel_xy) * self.samplesPerPixel:
            raise ValueError("sample_vec must hold spp vectors per pixel")
        if tail_count is not None and self.tail is not None:
            cnt = np.minimum(np.asarray(tail_count, dtype=np.int64), self.tail.shape[1])
            if len(cnt) != len(self.sample_vec):
                raise ValueError("tail_count must hold one entry per sample")
            self.max_tail = int(self.tail.shape[1])
            self.tail_offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
            self.tail = np.ascontiguousarray(self.tail[np.arange(self.tail.shape[1])[None, :] < cnt[:, None]])  # row-major: draw order per sample
            if len(self.tail) == 0:
                self.tail = np.zeros(1, np.float64)

    sampler_mode = _abi.DR_SAMPLER_HOST_BUFFER

    def to_abi(self, d):
        d.sampler_mode = self.sampler_mode
        d.spp = self.samplesPerPixel
        d.nsamples = len(self.sample_vec)
        d.pixel_xy = self.pixel_xy.ctypes.data
        d.sample_vec = self.sample_vec.ctypes.data
        d.sample_stride = self.sample_vec.shape[1]
        if self.li_seed is not None:
            d.seed = self.li_seed
        if self.tail is not None:
            d.tail = self.tail.ctypes.data
            if self.tail_offsets is not None:
                d.max_tail = self.max_tail
                d.tail_offsets = self.tail_offsets.ctypes.data
            else:
                d.max_tail = self.tail.shape[1]
        return [self.pixel_xy, self.sample_vec, self.tail, self.tail_offsets]
