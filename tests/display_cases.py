"""Inputs and callers shared by tests/test_display.py and tests/test_gpu_display.py (inputs only; the checker is
tests/display_restatement.py)."""
import ctypes as C
import itertools

import numpy as np

from dartray_amd import _abi

CURVES = (0, 1, 2)        # DR_TONE_CLAMP, _REINHARD, _FILMIC
ENCODES = (0, 1, 2)       # DR_ENCODE_SRGB, _GAMMA22, _REFERENCE
# (auto_exposure, permille, exposure, inv_white2): auto at the median and at another rank, and two manual scales
EXPOSURES = ((1, 500, 1.0, 0.0), (1, 900, 1.0, 0.25), (0, 500, 1.0, 0.0), (0, 500, 0.37, 0.0625))
COMBOS = list(itertools.product(CURVES, ENCODES, EXPOSURES))
INVALID_RGBA = 0x80FF10C0  # r = 0xC0, g = 0x10, b = 0xFF, a = 0x80: four different bytes, so a byte-order slip shows
SIZES = [(1, 1), (1, 7), (7, 1), (3, 2), (17, 33), (64, 64)]

_SPECIAL = [np.nan, np.inf, -np.inf, -1.0, -1e30, 0.0, -0.0, 1e-45, 1e-39, 1.1754942e-38, 1.17549435e-38, 1e30, 3e38, 1e20, 1.0, 1e-20]


def images(w, h, seed=11):
    """Seeded [h, w, 3] f32: magnitudes log-uniform over 1e-6 .. 1e3 with some hue, and, sprinkled over about a quarter of the pixels (all
    of them in a tiny image), one or more channels from NaN, +-inf, negatives, +-0, subnormals, the smallest normal number and its
    predecessor, and values up to 3e38."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * w + h))
    mag = 10.0 ** rng.uniform(-6.0, 3.0, size=(h, w, 1))
    rgb = (mag * rng.uniform(0.2, 1.0, size=(h, w, 3))).astype(np.float32)
    n = w * h
    flat = rgb.reshape(n, 3)
    count = n if n < 64 else n // 4
    where = rng.choice(n, size=count, replace=False)
    special = np.array(_SPECIAL, np.float32)
    i = np.arange(count)
    flat[where, i % 3] = special[i % len(special)]
    five = i % 5 == 0
    flat[where[five], (i[five] + 1) % 3] = special[(i[five] * 7 + 3) % len(special)]
    eleven = i % 11 == 0
    flat[where[eleven], :] = special[(i[eleven] // 11) % len(special)][:, None]
    return rgb


def flat(w, h, value=0.42):
    """Every pixel one luminance: a single bin takes every atomic."""
    return np.full((h, w, 3), value, np.float32)


def all_invalid(w, h):
    img = np.full((h, w, 3), 0.5, np.float32)
    img.reshape(-1, 3)[np.arange(w * h), np.arange(w * h) % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(w * h) % 3]
    return img


def one_valid(w, h):
    img = all_invalid(w, h)
    img.reshape(-1, 3)[(w * h) // 2] = (0.25, 0.5, 0.125)
    return img


def ramp(w, h):
    """Grey pixels whose luminance sits at the centre of bin 8 + (i mod 2032): with 2032 pixels or more every normal bin, 8 .. 2039, is
    occupied (lum(v, v, v) is v to a rounding or two, and the centre is half a bin away from either edge)."""
    i = np.arange(w * h, dtype=np.uint32)
    v = (((8 + i % 2032) << 20) | (1 << 19)).astype(np.uint32).view(np.float32)
    return np.repeat(v, 3).reshape(h, w, 3).copy()


WORST = {"flat": flat, "all_invalid": all_invalid, "one_valid": one_valid, "ramp": ramp}


def params(curve, encode, auto, permille=500, exposure=1.0, inv_white2=0.0, key=0.18, invalid_rgba=INVALID_RGBA):
    return _abi.DrDisplayParams(int(curve), int(encode), int(auto), int(permille), float(exposure), float(key), float(inv_white2), int(invalid_rgba))


def call(fn, rgb, p):
    """One of the two host-buffer entry points on an [h, w, 3] array -> (return code, [h, w, 4] uint8)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    out = np.full((h, w, 4), 7, np.uint8)
    return fn(rgb.ctypes.data, w, h, C.byref(p), out.ctypes.data), out


def host(rgb, p):
    rc, out = call(_abi.lib().dr_display_host, rgb, p)
    _abi.check(rc)
    return out


def exposure(fn, rgb, p, want_hist=True):
    """dr_display_exposure or _host -> (return code, the scale's f32 bits, the 2048 counts or None)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    scale = C.c_float(-3.0)
    hist = np.full(2048, 7, np.uint32) if want_hist else None
    rc = fn(rgb.ctypes.data, w, h, C.byref(p), C.byref(scale), hist.ctypes.data if want_hist else None)
    return rc, int(np.array([scale.value], np.float32).view(np.uint32)[0]), hist


def table_words(encode):
    words = np.zeros(256, np.uint32)
    _abi.check(_abi.lib().dr_display_table(int(encode), words.ctypes.data, 256))
    return words


def table(encode):
    """The library's table in the form the restatement takes: f32 [256] thresholds, or uint8 [256] for the reference encode."""
    words = table_words(encode)
    return words.astype(np.uint8) if encode == 2 else words.view(np.float32)
