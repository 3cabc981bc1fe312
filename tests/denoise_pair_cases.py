"""Inputs and callers shared by tests/test_denoise_pair.py and tests/test_gpu_denoise_pair.py (inputs only; the checker is
tests/denoise_pair_restatement.py)."""
import ctypes as C
import itertools

import numpy as np

from dartray_amd import _abi

import denoise_cases as dc

SIZES, ITERATIONS = dc.SIZES, dc.ITERATIONS
# each k zero or not; k_color is in units of the local variance here, 1/16 is sigma = 4
K_COMBOS = [tuple(k if on else 0.0 for k, on in zip((0.0625, 40.0, 0.3), bits)) for bits in itertools.product((False, True), repeat=3)]
VAR_FLOOR = 1.0e-4

# (which half, channel, value): what a sprinkled pixel gets.  3e38 in one half alone keeps the mean finite (1.5e38) while
# v0 = 0.25 * lum(3e38)^2 overflows; 9e18 in one half alone leaves both finite and huge (v0 of the order 1e36 .. 1e37)
_ONE_HALF_NON_FINITE = [("a", 0, np.nan), ("b", 1, np.inf), ("a", 2, -np.inf), ("b", 0, np.nan), ("ab", 1, np.nan), ("ab", 2, np.inf)]
_ONE_HALF_HUGE = [("a", 1, 3.0e38), ("b", 2, -3.0e38), ("a", 0, -9.0e18), ("b", 1, 9.0e18), ("a", 2, 9.0e18), ("b", 0, 3.0e38)]


def images(w, h, seed=7, variance_only=True):
    """Seeded a [h, w, 3], b [h, w, 3], normal [h, w, 3], depth [h, w]: two noisy copies of denoise_cases.images' picture, whose own NaN / inf
    pixels are in both halves and whose huge colours (3e38, -3e38, 2.5e38, 3.3e38) are in both too, so that their mean overflows (3e38 + 3e38).
    The noise level grows from 0.01 at the left edge to about 0.5 at the right one; in a block near the lower right corner a == b exactly.
    Sprinkled over them: non-finite values in a only, in b only and in both; and, unless `variance_only` is False, huge values of either sign in
    one half only -- the pixels whose variance alone decides their validity (a v0 that overflows beside a finite mean) or is huge."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * w + h + 500000))
    rgb, normal, depth = dc.images(w, h, seed)
    sigma = (0.01 + 0.5 * (np.arange(w, dtype=np.float64) / max(w - 1, 1)) ** 2)[None, :, None]
    with np.errstate(invalid="ignore"):
        a = (rgb + sigma * rng.normal(size=(h, w, 3))).astype(np.float32)
        b = (rgb + sigma * rng.normal(size=(h, w, 3))).astype(np.float32)
    if w * h >= 6:
        b[h - max(1, h // 4):, w - max(1, w // 3):] = a[h - max(1, h // 4):, w - max(1, w // 3):]
    kinds = _ONE_HALF_NON_FINITE + (_ONE_HALF_HUGE if variance_only else [])
    n = w * h
    for rep in range(2 if n >= 1024 else 1):
        for i, (half, chan, value) in enumerate(kinds[:n // 3]):
            p = (3 + 7 * i + 1301 * rep) % n if n >= 64 else (1 + 3 * i) % n
            if "a" in half:
                a[p // w, p % w, chan] = value
            if "b" in half:
                b[p // w, p % w, chan] = value
    return a, b, normal, depth


def params(iterations, kc, kn, kz, var_floor=VAR_FLOOR):
    return _abi.DrDenoisePairParams(int(iterations), float(kc), float(kn), float(kz), float(var_floor))


def call(fn, a, b, normal, depth, iterations, kc, kn, kz, var_floor=VAR_FLOOR, variance=True):
    """One of the two host-buffer entry points on [h, w, .] arrays -> (return code, out, out_var or None)."""
    a, b, normal, depth = (np.ascontiguousarray(x, np.float32) for x in (a, b, normal, depth))
    h, w = depth.shape
    out = np.full_like(a, -7.0)
    var = np.full_like(depth, -7.0) if variance else None
    p = params(iterations, kc, kn, kz, var_floor)
    rc = fn(a.ctypes.data, b.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, C.byref(p), out.ctypes.data,
            var.ctypes.data if variance else None)
    return rc, out, var


def host(a, b, normal, depth, iterations, kc, kn, kz, var_floor=VAR_FLOOR, variance=True):
    rc, out, var = call(_abi.lib().dr_denoise_pair_host, a, b, normal, depth, iterations, kc, kn, kz, var_floor, variance)
    _abi.check(rc)
    return out, var
