"""Inputs and callers shared by tests/test_firefly.py and tests/test_gpu_firefly.py (inputs only; the checker is
tests/firefly_restatement.py).

Sizes: one pixel; a column and a row of seven; 5 x 7; and four that are no multiple of the 64 x 4 tile or hold several tiles, so that the
device's tiles are partial on both axes and their halos cross tile edges.  Kinds of content:

    smooth     one surface, a smooth field, outliers 50 times as bright at the image's corners, its centre and the tile corners (63, 3) and
               (64, 4), which are diagonal neighbours: rank 1 lets them shield each other, rank 2 does not
    surfaces   two depths either side of a slanted line and two normals above and below the middle row, with outliers along both steps
    extremes   colours over five decades sprinkled with NaN and infinities in every plane, negative and subnormal channels, and huge ones
               up to the largest f32.  The luminance weights sum to one, so the luminance of finite channels cannot overflow; what
               overflows is threshold * m, which these members reach
    ties       grey levels 0.25, 1 and 8 only: every list of member luminances has ties, and a pixel of 1 among 0.25s sits exactly on the
               limit at threshold 4, floor 0, where `>` must leave it alone
    zeros      a black image of both zeros with a few lit pixels: m is a zero of either sign

Every kind also carries one +0 and one -0 black pixel, so that a valid pixel is left alone even at threshold 0, floor 0.

What a case must do to test anything (tests/test_firefly.py holds every case to it with the host loop): clamp at least one pixel and
leave at least one valid pixel alone.  One exception is forced by the rule itself: where no pixel of the image has `rank` members -- the
window holds too few pixels, min(w, 2 radius + 1) * min(h, 2 radius + 1) - 1 < rank, which covers 1 x 1 and, at radius 1, ranks 3 and 4
of the column and the row; or a guide step cuts the column's or the row's runs shorter than that -- nothing may be clamped, and that is
what the case is held to.  The member counts are the restatement's, not the library's."""
import ctypes as C
import itertools

import numpy as np

from dartray_amd import _abi

SIZES = [(1, 1), (1, 7), (7, 1), (5, 7), (65, 5), (130, 9), (64, 48)]    # (w, h)
KINDS = ["smooth", "surfaces", "extremes", "ties", "zeros"]
RADII = [1, 2]
RANKS = [1, 2, 3, 4]
LIMITS = [(4.0, 0.0), (0.0, 0.0), (1.5, 0.25)]                           # (threshold, floor)
DEPTH_TOL, NORMAL_TOL = 0.02, 0.05
# (radius, rank, threshold, floor, depth_tol, normal_tol): every radius x rank x limit at the default tolerances, and the defaults at
# tolerances of zero, where only a pixel with the very same guide is a member
PARAM_SETS = [(r, k, t, f, DEPTH_TOL, NORMAL_TOL) for r, k, (t, f) in itertools.product(RADII, RANKS, LIMITS)] + [(1, 2, 4.0, 0.0, 0.0, 0.0)]
DEFAULTS = (1, 2, 4.0, 0.0, DEPTH_TOL, NORMAL_TOL)
SENTINEL = -7.0
BIG = float(np.finfo(np.float32).max)


def spots(w, h):
    """The planted outliers' (x, y): the corners, the centre and the tile corners, those that lie inside."""
    want = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (63, 3), (64, 4), (127, 7), (128, 8)]
    return sorted({(x, y) for x, y in want if 0 <= x < w and 0 <= y < h})


def _encode(n):
    n = np.asarray(n, np.float64)
    return 0.5 * (n / np.linalg.norm(n, axis=-1, keepdims=True) + 1.0)


def image(w, h, kind, seed=11):
    """(rgb [h, w, 3], normal [h, w, 3], depth [h, w]) float32 of the named kind."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * w + 10 * h + KINDS.index(kind)))
    yy, xx = np.mgrid[0:h, 0:w]
    normal = np.broadcast_to(_encode([0.2, -0.1, -1.0]), (h, w, 3)).copy()
    depth = 3.0 + 0.01 * rng.integers(0, 2, (h, w))                      # two values: about half a pixel's neighbours share its depth exactly
    tint = np.array([1.0, 0.9, 0.8])
    field = 0.6 + 0.3 * xx / max(w - 1, 1) + 0.2 * yy / max(h - 1, 1)
    rgb = field[..., None] * tint * (1.0 + 0.05 * rng.random((h, w, 1)))
    boost = 50.0
    if kind == "surfaces":
        depth = depth + 4.0 * (2 * xx + yy >= w + h // 2)
        normal[yy >= (h + 1) // 2] = _encode([0.7, 0.1, -0.7])
        rgb[rng.random((h, w)) < 0.04] *= 30.0
        rgb[h // 3, w // 3] *= 30.0
    elif kind == "extremes":
        rgb = 10.0 ** rng.uniform(-3.0, 2.0, (h, w, 3))
        boost = 1.0e5
    elif kind == "ties":
        rgb = np.repeat(rng.choice([0.25, 1.0, 8.0], size=(h, w, 1), p=[0.7, 0.2, 0.1]), 3, axis=2)
        boost = 64.0
    elif kind == "zeros":
        rgb = np.where(rng.random((h, w, 3)) < 0.5, 0.0, -0.0)
        rgb[rng.random((h, w)) < 0.1] = 0.5
    rgb, normal, depth = rgb.astype(np.float32), normal.astype(np.float32), depth.astype(np.float32)
    if kind == "extremes":
        where, pick = rng.random((h, w)), rng.integers(0, 3, (h, w))
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        for k, (plane, value) in enumerate([(rgb, bad), (normal, bad), (depth, bad), (rgb, np.float32([-1.0, -0.25, -100.0])),
                                            (rgb, np.float32([1e-40, 1e-45, -1e-40])), (rgb, np.float32([3e38, BIG, -3e38]))]):
            hit = (where >= 0.03 * k) & (where < 0.03 * (k + 1))
            if plane.ndim == 2:
                plane[hit] = value[pick[hit]]
            elif k == 5:
                plane[hit] = value[pick[hit]][:, None]                   # all three channels huge
            else:
                plane[hit, 1] = value[pick[hit]]
    planted = spots(w, h)
    for x, y in planted:                                                 # a planted outlier is valid and lit, whatever lay there
        lit = rgb[y, x] if kind not in ("extremes", "zeros") else np.float32([1.0, 0.9, 0.8])
        rgb[y, x] = np.float32(boost) * lit
        normal[y, x] = normal[y, x - 1] if x > 0 and np.isfinite(normal[y, x - 1]).all() else np.float32(_encode([0.2, -0.1, -1.0]))
        if not np.isfinite(depth[y, x]):
            depth[y, x] = 3.0
    if kind != "surfaces":                                               # the centre outlier's neighbours share its depth to the bit, so that
        x, y = w // 2, h // 2                                            # it has members at a depth_tol of 0 even in the column and the row
        near = depth[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
        near[np.isfinite(near)] = depth[y, x]
    black = [(x, y) for x, y in ((w // 4, h // 4), (3 * w // 4, 3 * h // 4)) if (x, y) not in planted]
    for k, (x, y) in enumerate(black):
        rgb[y, x] = np.float32(0.0 if k == 0 else -0.0)
        if not (np.isfinite(normal[y, x]).all() and np.isfinite(depth[y, x])):
            normal[y, x], depth[y, x] = np.float32(_encode([0.2, -0.1, -1.0])), 3.0
    return rgb, normal, depth


def halo_image(w, h, seed=29):
    """The GPU suite's radius-2 case: the smooth kind with outliers in the two columns either side of every tile edge in x and over a
    twelfth of all pixels -- every row is within two of a tile edge in y -- so that a pixel's window holds outliers that the workgroup
    staged as halo, from a neighbouring tile."""
    rgb, normal, depth = image(w, h, "smooth", seed)
    rng = np.random.Generator(np.random.PCG64(seed + w + 100 * h))
    yy, xx = np.mgrid[0:h, 0:w]
    edge = np.isin(xx % 64, (0, 1, 62, 63)) & (rng.random((h, w)) < 0.3)
    rgb[edge | (rng.random((h, w)) < 1.0 / 12.0)] *= np.float32(40.0)
    return rgb, normal, depth


def grid():
    """Every case of the byte-for-byte comparison: (key, (rgb, normal, depth), parameter set)."""
    for size in SIZES:
        for kind in KINDS:
            imgs = image(*size, kind)
            for ps in PARAM_SETS:
                yield (size, kind, ps), imgs, ps


def params(radius, rank, threshold, floor, depth_tol, normal_tol):
    return _abi.DrFireflyParams(int(radius), int(rank), float(threshold), float(floor), float(depth_tol), float(normal_tol))


def call(fn, rgb, normal, depth, ps, with_removed=True):
    """One of the two host-buffer entry points -> (return code, out, removed or None); the outputs start as a sentinel."""
    rgb, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb, normal, depth))
    h, w = depth.shape
    out = np.full_like(rgb, SENTINEL)
    removed = np.full_like(depth, SENTINEL) if with_removed else None
    p = params(*ps)
    rc = fn(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data, removed.ctypes.data if with_removed else None)
    return rc, out, removed


def host(rgb, normal, depth, ps, with_removed=True):
    rc, out, removed = call(_abi.lib().dr_firefly_host, rgb, normal, depth, ps, with_removed)
    _abi.check(rc)
    return out, removed
