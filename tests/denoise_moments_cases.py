"""Inputs and callers shared by tests/test_denoise_moments.py and tests/test_gpu_denoise_moments.py (inputs only; the checker is
tests/denoise_moments_restatement.py)."""
import ctypes as C

import numpy as np

from dartray_amd import _abi

F = np.float32
# (w, h): one pixel; smaller than the 7 x 7 window either way; exactly one 64 x 4 tile; one pixel more either way; ragged in both; two tiles
# and a ragged third in x
SIZES = [(1, 1), (3, 5), (64, 4), (65, 5), (67, 9), (130, 7)]
BIG = (70, 300)                                                          # 2 x 75 tiles, ragged in x: the tile walk beyond one workgroup row
VAR_FLOOR = 1.0e-4
# (iterations, k_color, k_normal, k_depth, var_floor, min_history, radius): 1, 3 and 8 levels (step 2^7 exceeds every image); radius 0, 1
# and 3; each guide term off, and both; the smallest and the largest min_history
PARAMS = [
    (1, 0.0625, 40.0, 0.3, VAR_FLOOR, 4, 3),
    (3, 0.0625, 40.0, 0.3, VAR_FLOOR, 4, 3),
    (8, 0.0625, 40.0, 0.3, VAR_FLOOR, 4, 3),
    (3, 0.0625, 0.0, 0.3, VAR_FLOOR, 4, 1),
    (3, 0.0625, 40.0, 0.0, VAR_FLOOR, 4, 0),
    (1, 0.0, 0.0, 0.0, 0.5, 4, 3),
    (3, 0.0625, 40.0, 0.3, VAR_FLOOR, 2, 3),
    (1, 0.0625, 40.0, 0.3, VAR_FLOOR, 4096, 1),
]
POISON = [None, "rgb", "m2", "len", "normal", "depth"]                  # the image that gets NaN, +inf and -inf


def lengths(min_history):
    """The history lengths one 64-pixel row mixes: none, one frame, fractions just below and just above min_history, and the longest."""
    m = F(min_history)
    return np.array([0, 1, 2, 3, np.nextafter(m, F(0)), m, np.nextafter(m, F(1e9)), 1.5, float(m) - 0.5, float(m) + 0.5, 7, 32, 4096],
                    np.float32)


def images(w, h, min_history=4, poison=None, seed=11):
    """Seeded rgb [h, w, 3], m2 [h, w], len [h, w], normal [h, w, 3], depth [h, w], as a temporal history leaves them: colours around a
    gradient with noise that grows to the right, 0.5 * (n + 1) normals in two flat regions, depths around 30 with a step, m2 = lum^2 plus a
    positive spread except where it is below lum^2 (one pixel in eight: the clamp) and the 13 values of lengths() at stride 5 through
    every row, so that len = 0 (not valid) falls on the border, in the interior and in the centre row of its neighbours' windows.  A few huge
    colours (lum^2 overflows).  `poison` names the image that gets NaN, +inf and -inf: in a corner, on the last row and in the middle."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * w + h))
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    base = 0.25 + 1.5 * (x / max(w - 1, 1))[..., None] * np.array([1.0, 0.7, 0.4]) + 0.3 * (y / max(h - 1, 1))[..., None]
    sigma = (0.01 + 0.4 * (x / max(w - 1, 1)) ** 2)[..., None]
    rgb = (base + sigma * rng.normal(size=(h, w, 3))).astype(np.float32)
    n = np.where((x + 2 * y < (w + 2 * h) // 2)[..., None], np.array([0.0, 0.6, 0.8]), np.array([0.8, 0.0, -0.6]))
    n = n + 0.02 * rng.normal(size=(h, w, 3))
    normal = (0.5 * (n / np.linalg.norm(n, axis=2, keepdims=True) + 1.0)).astype(np.float32)
    depth = (28.0 + 0.05 * x + np.where(x > (2 * w) // 3, 4.0, 0.0) + 0.1 * rng.random((h, w))).astype(np.float32)
    lum = (F(0.212671) * rgb[..., 0] + F(0.715160) * rgb[..., 1]) + F(0.072169) * rgb[..., 2]
    spread = (sigma[..., 0] ** 2 * (0.5 + rng.random((h, w)))).astype(np.float32)
    m2 = (lum * lum + spread).astype(np.float32)
    below = (3 * x + 5 * y) % 8 == 3
    m2[below] = (lum * lum)[below] * F(0.75) - F(0.125)                # m2 < lum^2, some of them negative
    ls = lengths(min_history)
    length = ls[(5 * x + 3 * y) % len(ls)].astype(np.float32)
    if w * h >= 64:
        for i, v in enumerate((3.0e38, -3.0e38, 2.5e38)):
            rgb[(2 * i + 1) % h, (23 * i + 9) % w, i] = v
        m2[h - 1, 5], length[h - 1, 5] = 3.0e38, 4096.0                  # a huge temporal variance that stays finite
    if poison is not None:
        img = {"rgb": rgb, "m2": m2, "len": length, "normal": normal, "depth": depth}[poison]
        for (py, px), v in zip(((0, min(1, w - 1)), (h - 1, w // 2), (h // 2, w - 1 - w // 3)), (np.nan, np.inf, -np.inf)):
            if img.ndim == 3:
                img[py, px, (px + py) % 3] = v
            else:
                img[py, px] = v
        if poison == "len" and w * h >= 6:
            length[h // 2, 1] = -3.0                                     # finite and not positive
    return rgb, m2, length, normal, depth


def params(iterations, kc, kn, kz, var_floor=VAR_FLOOR, min_history=4, radius=3):
    return _abi.DrDenoiseMomentsParams(int(iterations), float(kc), float(kn), float(kz), float(var_floor), int(min_history), int(radius))


def call(fn, rgb, m2, length, normal, depth, prm, variance=True, estimate=True):
    """One of the two host-buffer entry points on [h, w, .] arrays -> (return code, out, out_var or None, out_var0 or None)."""
    rgb, m2, length, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb, m2, length, normal, depth))
    h, w = depth.shape
    out = np.full_like(rgb, -7.0)
    var = np.full_like(depth, -7.0) if variance else None
    var0 = np.full_like(depth, -7.0) if estimate else None
    p = params(*prm)
    rc = fn(rgb.ctypes.data, m2.ctypes.data, length.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data,
            var.ctypes.data if variance else None, var0.ctypes.data if estimate else None)
    return rc, out, var, var0


def host(rgb, m2, length, normal, depth, prm, variance=True, estimate=True):
    rc, out, var, var0 = call(_abi.lib().dr_denoise_moments_host, rgb, m2, length, normal, depth, prm, variance, estimate)
    _abi.check(rc)
    return out, var, var0


def grid(sizes=SIZES):
    """Every (size, poison, parameters) of the CPU suite: (key, the five images, the parameters)."""
    for size in sizes:
        for poison in POISON:
            for prm in PARAMS:
                yield (size, poison, prm), images(*size, min_history=prm[5], poison=poison), prm
