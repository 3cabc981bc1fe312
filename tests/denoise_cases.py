"""Inputs and callers shared by tests/test_denoise.py and tests/test_gpu_denoise.py (inputs only; the checker is tests/denoise_restatement.py)."""
import ctypes as C
import itertools

import numpy as np

from dartray_amd import _abi

SIZES = [(1, 1), (1, 7), (7, 1), (3, 2), (17, 33), (64, 64)]             # (w, h)
ITERATIONS = [1, 2, 5, 8]                                                # step 128 at the last level: larger than every image
# each k zero or not
K_COMBOS = [tuple(k if on else 0.0 for k, on in zip((1.5, 40.0, 0.3), bits)) for bits in itertools.product((False, True), repeat=3)]


def images(w, h, seed=7):
    """Seeded rgb [h, w, 3], normal [h, w, 3], depth [h, w]: colours in [0, 4) with a few huge ones of either sign (their squared distance to every
    other colour is infinite), 0.5 * (n + 1) normals, depths around 30, a block of "misses" (normal and depth 0, as the feature
    integrator writes them) and NaN / +inf / -inf sprinkled over about one pixel in twelve, in colour, in a guide or in both."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * w + h))
    rgb = (4.0 * rng.random((h, w, 3))).astype(np.float32)
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    normal = (0.5 * (n + 1.0)).astype(np.float32)
    depth = (25.0 + 10.0 * rng.random((h, w))).astype(np.float32)
    if w * h >= 6:
        y0, x0 = h // 3, w // 4
        normal[y0:y0 + max(1, h // 4), x0:x0 + max(1, w // 3)] = 0.0
        depth[y0:y0 + max(1, h // 4), x0:x0 + max(1, w // 3)] = 0.0
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    where = rng.random((h, w))
    pick = rng.integers(0, 3, (h, w))
    chan = rng.integers(0, 3, (h, w))
    for y, x in zip(*np.nonzero(where < 0.08)):
        kind = where[y, x]
        if kind < 0.03 or kind >= 0.06:
            rgb[y, x, chan[y, x]] = bad[pick[y, x]]
        if 0.03 <= kind < 0.05 or kind >= 0.06:
            normal[y, x, (chan[y, x] + 1) % 3] = bad[(pick[y, x] + 1) % 3]
        if 0.05 <= kind < 0.06:
            depth[y, x] = bad[(pick[y, x] + 2) % 3]
    if w * h >= 64:
        for i, v in enumerate((3.0e38, -3.0e38, 2.5e38, 3.3e38)):
            y, x = (5 * i + 2) % h, (7 * i + 3) % w
            if np.isfinite(rgb[y, x]).all():
                rgb[y, x, i % 3] = v
    return rgb, normal, depth


def params(iterations, kc, kn, kz):
    return _abi.DrDenoiseParams(int(iterations), float(kc), float(kn), float(kz))


def call(fn, rgb, normal, depth, iterations, kc, kn, kz):
    """One of the two host-buffer entry points on [h, w, .] arrays -> (return code, out)."""
    rgb, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb, normal, depth))
    h, w = depth.shape
    out = np.full_like(rgb, -7.0)
    p = params(iterations, kc, kn, kz)
    return fn(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data), out


def host(rgb, normal, depth, iterations, kc, kn, kz):
    rc, out = call(_abi.lib().dr_denoise_atrous_host, rgb, normal, depth, iterations, kc, kn, kz)
    _abi.check(rc)
    return out
