"""Inputs and callers shared by tests/test_upsample.py and tests/test_gpu_upsample.py (inputs only; the checker is tests/upsample_restatement.py)."""
import ctypes as C
import itertools

import numpy as np

from dartray_amd import _abi

LOW_SIZES = [(1, 1), (2, 1), (1, 3), (3, 2), (5, 7)]                     # (wl, hl): one tap inside; one axis; borders on every side + an interior
FACTORS = [2, 4]
TAPS = [2, 4]
K_COMBOS = [tuple(k if on else 0.0 for k, on in zip((40.0, 0.3), bits)) for bits in itertools.product((False, True), repeat=2)]   # (k_normal, k_depth)
INVALID = ["colour", "normal", "depth", "full", "all"]

# a scene file of two quads, an emitter over a floor, for the PBRT front end
TINY_PBRT = ('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\nSampler "lowdiscrepancy" "integer pixelsamples" [4]\n'
             'Film "image" "integer xresolution" [24] "integer yresolution" [16]\nSurfaceIntegrator "directlighting"\nWorldBegin\n'
             'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [8 8 8]\nTranslate 0 3 0\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
             '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nAttributeEnd\n'
             'Material "matte" "rgb Kd" [0.6 0.4 0.2]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
             '"point P" [-2 -1 -2  2 -1 -2  2 -1 2  -2 -1 2]\nWorldEnd\n')


def images(wl, hl, f, seed=3, invalid=None):
    """Seeded (rgb_lo [hl, wl, 3], normal_lo [hl, wl, 3], depth_lo [hl, wl], normal [h, w, 3], depth [h, w]): colours over five decades,
    10^-3 .. 10^2, 0.5 * (n + 1) guides of random unit normals, depths around 3 with a step of 4 along a slanted line.  The low-resolution
    guides are the f x f block means of the full-resolution ones.  `invalid`: "colour" / "normal" / "depth" put NaN, +inf and -inf into
    that low-resolution image (one pixel each, where there are that many); "full" into the full-resolution guides; "all" makes every
    low-resolution pixel invalid, one way or another, with a NaN colour among them."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * wl + 10 * hl + f))
    h, w = f * hl, f * wl
    rgb_lo = (10.0 ** rng.uniform(-3.0, 2.0, (hl, wl, 3))).astype(np.float32)
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    normal = (0.5 * (n + 1.0)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (3.0 + 0.25 * rng.random((h, w)) + 4.0 * (2 * xx + yy >= w + h // 2)).astype(np.float32)
    normal_lo = normal.astype(np.float64).reshape(hl, f, wl, f, 3).mean(axis=(1, 3)).astype(np.float32)
    depth_lo = depth.astype(np.float64).reshape(hl, f, wl, f).mean(axis=(1, 3)).astype(np.float32)
    bad = [np.nan, np.inf, -np.inf]
    if invalid in ("colour", "normal", "depth"):
        target = {"colour": rgb_lo, "normal": normal_lo, "depth": depth_lo}[invalid]
        for k, q in enumerate(rng.permutation(wl * hl)[:3]):
            if invalid == "depth":
                target[q // wl, q % wl] = bad[k]
            else:
                target[q // wl, q % wl, (q + k) % 3] = bad[k]
    elif invalid == "full":
        for k, p in enumerate(rng.permutation(w * h)[:6]):
            if k % 2:
                depth[p // w, p % w] = bad[k % 3]
            else:
                normal[p // w, p % w, k % 3] = bad[k % 3]
    elif invalid == "all":
        for q in range(wl * hl):
            y, x = q // wl, q % wl
            if q % 3 == 0:
                rgb_lo[y, x, q % 2] = bad[(q // 3) % 3]                  # q = 0: a NaN colour
            elif q % 3 == 1:
                normal_lo[y, x, 2] = bad[q % 2 + 1]
            else:
                depth_lo[y, x] = bad[q % 3]
    elif invalid is not None:
        raise ValueError(invalid)
    return rgb_lo, normal_lo, depth_lo, normal, depth


def random_image(wl, hl, f, seed=11):
    """The larger GPU cases: images() with NaN / +inf / -inf sprinkled over about one low-resolution pixel in sixteen (colour, normal or
    depth) and one full-resolution guide pixel in sixty-four."""
    rgb_lo, normal_lo, depth_lo, normal, depth = images(wl, hl, f, seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    where, pick = rng.random((hl, wl)), rng.integers(0, 3, (hl, wl))
    rgb_lo[where < 0.02, 1] = bad[pick[where < 0.02]]
    normal_lo[(where >= 0.02) & (where < 0.04), 0] = bad[pick[(where >= 0.02) & (where < 0.04)]]
    depth_lo[(where >= 0.04) & (where < 0.06)] = bad[pick[(where >= 0.04) & (where < 0.06)]]
    where = rng.random(depth.shape)
    depth[where < 0.008] = np.inf
    normal[(where >= 0.008) & (where < 0.016), 2] = np.nan
    return rgb_lo, normal_lo, depth_lo, normal, depth


def params(factor, taps, kn, kz):
    return _abi.DrUpsampleParams(int(factor), int(taps), float(kn), float(kz))


def call(fn, rgb_lo, normal_lo, depth_lo, normal, depth, factor, taps, kn, kz):
    """One of the two host-buffer entry points on [., ., .] arrays -> (return code, out)."""
    rgb_lo, normal_lo, depth_lo, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb_lo, normal_lo, depth_lo, normal, depth))
    hl, wl = depth_lo.shape
    out = np.full_like(normal, -7.0)
    p = params(factor, taps, kn, kz)
    return fn(rgb_lo.ctypes.data, normal_lo.ctypes.data, depth_lo.ctypes.data, wl, hl, normal.ctypes.data, depth.ctypes.data, C.byref(p),
              out.ctypes.data), out


def host(rgb_lo, normal_lo, depth_lo, normal, depth, factor, taps, kn, kz):
    rc, out = call(_abi.lib().dr_upsample_host, rgb_lo, normal_lo, depth_lo, normal, depth, factor, taps, kn, kz)
    _abi.check(rc)
    return out


def grid():
    """Every (low size, factor, taps, invalid) of the byte-for-byte comparison; each runs all four k combinations."""
    for size in LOW_SIZES:
        for f in FACTORS:
            for taps in TAPS:
                for invalid in [None] + INVALID:
                    yield size, f, taps, invalid


def overflow_case():
    """A k_depth * dz that overflows for every tap: the low depths are 1e10, the full ones about 3, dz about 1e20 and k_depth 3e38, so every
    weight is wt / inf = 0 and sumw stays 0.  All values are finite and every low-resolution pixel is valid."""
    rgb_lo, normal_lo, depth_lo, normal, depth = images(3, 2, 2)
    depth_lo[:] = 1.0e10
    return (rgb_lo, normal_lo, depth_lo, normal, depth), (2, 4, 0.0, 3.0e38)


def step_case(taps, kz):
    """Edge keeping: low 8 x 8, two half-planes at depths 1 and 5 with colours 0 and 1 that meet between low columns 3 and 4; the
    full-resolution guides (16 x 16) put the step at column 7, an odd one, so that full column 7 lies on the far side of its own low pixel.
    Returns (the five images, factor, taps, k_normal, k_depth) and the mask of the full-resolution pixels on the depth-5 side."""
    rgb_lo = np.zeros((8, 8, 3), np.float32)
    rgb_lo[:, 4:] = 1.0
    depth_lo = np.where(np.arange(8) >= 4, 5.0, 1.0).astype(np.float32)[None, :].repeat(8, axis=0)
    far = (np.arange(16) >= 7)[None, :].repeat(16, axis=0)
    depth = np.where(far, 5.0, 1.0).astype(np.float32)
    normal_lo, normal = np.full((8, 8, 3), 0.5, np.float32), np.full((16, 16, 3), 0.5, np.float32)
    return (rgb_lo, normal_lo, np.ascontiguousarray(depth_lo), normal, depth, 2, taps, 0.0, kz), far
