"""DESIGN.md 2.9 (DR_SAMPLER_HALTON) restated in plain Python: HaltonSampler.getMoreSamples (samplers/halton_sampler.dart:54-100) with
RadicalInverse / LatinHypercube (core/montecarlo.dart:305-339) and Lerp (core/common.dart:80-81), on Python floats (IEEE f64, no fused
operation) and core.DartRandom.  Written apart from core.HaltonSampler and from the kernels; cited by file.dart:line of the reference.

Two ways to feed it, as tests/stratified_restatement.py has: `keyed` (the device mode: the LatinHypercube draws of index k from the
stream (seed, k, 0, kind 5), the draws inside Li from (seed, k, 0, kind 2)) and `serial` (the reference's own: one RNG(taskNum) through
every accepted sample).
"""
import collections
import math

import numpy as np

from dartray_amd import core

from montecarlo_restatement import ONE_MINUS_EPSILON, LatinHypercube  # noqa: F401  (shared with stratified_restatement.py)
from stratified_restatement import counter_key, sample_extent


def RadicalInverse(n, base):                                      # montecarlo.dart:327-339
    val = 0.0
    invBase = 1.0 / base
    invBi = invBase
    while n > 0:
        d_i = n % base
        val += d_i * invBi
        n = int(n * invBase)                                       # (n * invBase).toInt(): a product, truncated
        invBi *= invBase
    return val


def radical_inverse_int(n, base):
    """The same sum with the textbook integer division as the digit loop's step: what the multiply-and-truncate step must equal."""
    val, invBase = 0.0, 1.0 / base
    invBi = invBase
    while n > 0:
        val += (n % base) * invBi
        n //= base
        invBi *= invBase
    return val


def Lerp(t, v1, v2):                                               # common.dart:80-81
    return v1 * (1.0 - t) + v2 * t


def task_window(film, task_num=0, task_count=1):
    """(left, top, width, height): GetSubWindow's extents of the sampler extent, handed to the sampler as they are (dartray.dart:1009-1023)."""
    e = sample_extent(film)
    x0, x1, y0, y1 = core.GetSubWindow(e[1] - e[0], e[3] - e[2], task_num, max(1, task_count))
    return x0, y0, x1 - x0, y1 - y0


def wanted(window, spp):                                           # halton_sampler.dart:35-36
    delta = max(window[2], window[3])
    return spp * delta * delta


def image_sample(window, k):                                       # :69-74
    left, top, width, height = window
    lerpDelta = float(max(width, height))
    return Lerp(RadicalInverse(k, 3), left, left + lerpDelta), Lerp(RadicalInverse(k, 2), top, top + lerpDelta)


def is_accepted(window, imageX, imageY):                           # :78; right / bottom inclusive (sampler.dart:52-54)
    left, top, width, height = window
    return not (imageX > left + width - 1 or imageY > top + height - 1)


Samples = collections.namedtuple("Samples", "k pixel_xy vec tail imageXY")
Samples.__doc__ = """The accepted samples of a range of indices, in increasing k: k [n] uint64, the anchor pixels [n, 2] int32, the vectors
[n, nFloats] f32 in the C ABI's field order, the first max_tail draws inside Li [n, max(1, max_tail)] f64, and imageXY [n, 2] f64 = anchor +
f32 fraction, the image sample every consumer of the vector forms."""


def _samples(window, spp, n1D, n2D, max_tail, lhs_rng, li_rng, first=0, count=None):
    ks, pix, vecs, tails, xys = [], [], [], [], []
    nf = 5 + sum(n1D) + 2 * sum(n2D)
    last = wanted(window, spp) if count is None else first + count
    for k in range(first, last):
        imageX, imageY = image_sample(window, k)
        if not is_accepted(window, imageX, imageY):
            continue
        px, py = math.floor(imageX), math.floor(imageY)
        v = np.zeros(nf, np.float32)                               # every store rounds the f64 value to f32 once
        v[0], v[1] = imageX - px, imageY - py
        v[2], v[3] = RadicalInverse(k + 1, 5), RadicalInverse(k + 1, 7)   # currentSample was incremented at :76
        v[4] = RadicalInverse(k + 1, 11)                           # (the Lerp over the shutter happens in the consumer)
        rng, o = lhs_rng(k), 5
        for c in n1D:                                              # :91-93
            buf = np.zeros(c, np.float32)
            LatinHypercube(buf, c, 1, rng)
            v[o:o + c] = buf
            o += c
        for c in n2D:                                              # :95-97
            buf = np.zeros(2 * c, np.float32)
            LatinHypercube(buf, c, 2, rng)
            v[o:o + 2 * c] = buf
            o += 2 * c
        r = li_rng(k)
        tails.append([r.randomFloat() for _ in range(max_tail)] if r is not None else [])
        ks.append(k)
        pix.append((px, py))
        vecs.append(v)
        xys.append((px + float(v[0]), py + float(v[1])))
    n = len(ks)
    tail = np.zeros((n, max(1, max_tail)), np.float64)
    for i, t in enumerate(tails):
        tail[i, :len(t)] = t
    return Samples(np.array(ks, np.uint64), np.array(pix, np.int32).reshape(-1, 2), np.array(vecs, np.float32).reshape(-1, nf), tail,
                   np.array(xys, np.float64).reshape(-1, 2))


def keyed(window, spp, seed, n1D, n2D, max_tail=0, first=0, count=None):
    """The device mode for the indices [first, first + count) of the window's sequence (count None: to its end)."""
    return _samples(window, spp, n1D, n2D, max_tail, lambda k: core.DartRandom(counter_key(seed, k, 0, 5)),
                    lambda k: core.DartRandom(counter_key(seed, k, 0, 2)) if max_tail else None, first, count)


def serial(window, spp, n1D, n2D, rng):
    """The reference's mode: ONE rng through every accepted sample in order (no draws inside Li: DirectLighting, or a path of depth <= 2)."""
    return _samples(window, spp, n1D, n2D, 0, lambda k: rng, lambda k: None)


# ---- the draws inside Li for many samples at once (numpy uint64 arithmetic wraps like the generator's) -------------------------------
def _mix64_np(n):
    u = np.uint64
    n = (~n) + (n << u(21))
    n = n ^ (n >> u(24))
    n = n * u(265)
    n = n ^ (n >> u(14))
    n = n * u(21)
    n = n ^ (n >> u(28))
    return n + (n << u(31))


def li_tail(seed, ks, max_tail):
    """[len(ks), max(1, max_tail)] f64: the first max_tail randomFloat() of the stream (seed, k, 0, kind 2) of every k -- what `keyed`
    returns as `tail`, vectorised over the samples (tests/test_halton_sampler.py compares the two)."""
    u = np.uint64
    ks = np.asarray(ks, np.uint64)
    out = np.zeros((len(ks), max(1, max_tail)), np.float64)
    if len(ks) == 0 or max_tail == 0:
        return out
    h = _mix64_np(np.full(len(ks), (seed & ((1 << 64) - 1)) ^ 0x9E3779B97F4A7C15, np.uint64))          # dr_counter_key(seed, k, 0, 2)
    h = _mix64_np(h ^ (ks * u(0xD1B54A32D192ED03) + u(2)))
    h = _mix64_np(h ^ np.full(len(ks), 0x5851F42D4C957F2D, np.uint64))
    key = h & u(0x7fffffffffffffff)
    state = _mix64_np(key)                                                                              # Random(seed)
    state[state == 0] = u(0x5A17)
    lo, hi = state & u(0xffffffff), state >> u(32)

    def step(lo, hi):
        s = u(0xffffda61) * lo + hi
        return s & u(0xffffffff), s >> u(32)

    for _ in range(4):
        lo, hi = step(lo, hi)
    for t in range(max_tail):                                                                           # nextDouble: 26 + 27 bits
        lo, hi = step(lo, hi)
        a = (lo & u((1 << 26) - 1)).astype(np.float64)
        lo, hi = step(lo, hi)
        b = (lo & u((1 << 27) - 1)).astype(np.float64)
        out[:, t] = (a * 134217728.0 + b) / 9007199254740992.0
    return out
