"""The display transform (dr_display*): a linear f32 image becomes an 8-bit RGBA one -- exposure (given, or the percentile of a
luminance histogram found on the device), a tone curve, an 8-bit encode -- and the two image files a viewer opens without further tools.

    tonemap(rgb, ...)             [h, w, 3] f32 -> [h, w, 4] uint8
    exposure_of(rgb, ...)         the scale auto-exposure picks, and the 2048 counts it picked from
    tables(encode)                the thresholds (f32) or the reference's gamma table (uint8) every path reads
    to_image(output_image, ...)   tonemap of an OutputImage's rgb
    write_png / write_ppm         zlib and struct from the standard library only

The library takes inv_white2 = 1 / white^2 (0: the plain Reinhard curve); this module takes `white`, as denoise.sharpness takes sigmas.
"""
import ctypes as C
import math
import struct
import zlib

import numpy as np

from . import _abi
from ._image import _entry, _images

CURVES = {"clamp": _abi.DR_TONE_CLAMP, "reinhard": _abi.DR_TONE_REINHARD, "filmic": _abi.DR_TONE_FILMIC}
ENCODES = {"srgb": _abi.DR_ENCODE_SRGB, "gamma22": _abi.DR_ENCODE_GAMMA22, "reference": _abi.DR_ENCODE_REFERENCE}
# The defaults: the median luminance goes to middle grey, 0.18; plain Reinhard; sRGB; an invalid pixel is opaque black
KEY = 0.18
PERCENTILE = 0.5
CURVE = "reinhard"
ENCODE = "srgb"
INVALID = (0, 0, 0, 255)


def inv_white2(white):
    """1 / white^2 as the f32 the library takes; an infinite white gives 0, the plain Y / (1 + Y)."""
    white = float(white)
    if math.isnan(white) or white <= 0.0:
        raise ValueError("display: white must be positive (inf is the plain Reinhard curve), got %r" % (white,))
    return 0.0 if math.isinf(white) else float(np.float32(1.0 / (white * white)))


def _named(table, what, name):
    if name not in table:
        raise ValueError("display: %s must be one of %s (got %r)" % (what, ", ".join(sorted(table)), name))
    return table[name]


def params(exposure=None, key=KEY, percentile=PERCENTILE, curve=CURVE, white=float("inf"), encode=ENCODE, invalid=INVALID):
    """The DrDisplayParams of tonemap()'s keywords; exposure=None is auto-exposure."""
    percentile = float(percentile)
    if not 0.0 <= percentile <= 1.0:
        raise ValueError("display: percentile must be in 0..1 (got %r)" % (percentile,))
    invalid = tuple(int(v) for v in invalid)
    if len(invalid) != 4 or any(v < 0 or v > 255 for v in invalid):
        raise ValueError("display: invalid must be four bytes (r, g, b, a), got %r" % (invalid,))
    rgba = invalid[0] | invalid[1] << 8 | invalid[2] << 16 | invalid[3] << 24
    return _abi.DrDisplayParams(_named(CURVES, "curve", curve), _named(ENCODES, "encode", encode), 1 if exposure is None else 0,
                                int(round(percentile * 1000.0)), 1.0 if exposure is None else float(exposure), float(key), inv_white2(white),
                                rgba)


def _image(rgb):
    return _images("display", "rgb must be [h, w, 3]", (rgb,))[0]


def tonemap(rgb, exposure=None, key=KEY, percentile=PERCENTILE, curve=CURVE, white=float("inf"), encode=ENCODE, invalid=INVALID, device=True):
    """rgb [h, w, 3] linear f32 -> [h, w, 4] uint8, alpha 255.  exposure=None: the scale is key over the luminance at `percentile` of the
    image's histogram; else the scale is `exposure`.  device=True: dr_display, on the GPU; device=False: dr_display_host, which needs none
    and writes the same bytes."""
    rgb = _image(rgb)
    h, w = rgb.shape[:2]
    p = params(exposure, key, percentile, curve, white, encode, invalid)
    out = np.zeros((h, w, 4), np.uint8)
    _abi.check(_entry("dr_display", device)(rgb.ctypes.data, w, h, C.byref(p), out.ctypes.data))
    return out


def exposure_of(rgb, key=KEY, percentile=PERCENTILE, device=True):
    """(scale, hist): the f32 scale auto-exposure picks for this image, as a float, and the 2048 uint32 counts of its luminance histogram."""
    rgb = _image(rgb)
    h, w = rgb.shape[:2]
    p = params(None, key, percentile)
    scale = C.c_float(0.0)
    hist = np.zeros(_abi.DR_DISPLAY_BINS, np.uint32)
    _abi.check(_entry("dr_display_exposure", device)(rgb.ctypes.data, w, h, C.byref(p), C.byref(scale), hist.ctypes.data))
    return float(scale.value), hist


def tables(encode):
    """The table every path reads.  "srgb", "gamma22": float32 [256], T[0] = 0 and T[k] the linear value at which code k begins;
    "reference": uint8 [256], ImageFilm's gamma table G."""
    code = _named(ENCODES, "encode", encode)
    words = np.zeros(256, np.uint32)
    _abi.check(_abi.lib().dr_display_table(code, words.ctypes.data, 256))
    return words.astype(np.uint8) if code == _abi.DR_ENCODE_REFERENCE else words.view(np.float32)


def to_image(output_image, **kw):
    """tonemap() of an OutputImage's rgb; kw: tonemap()'s keywords."""
    return tonemap(output_image.rgb, **kw)


def _rgba8(rgba8):
    a = np.ascontiguousarray(rgba8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("display: an image to write must be uint8 [h, w, 4] (got %s %r)" % (a.dtype, a.shape))
    return a


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, rgba8):
    """8-bit RGBA, no interlace, every scanline with filter type 0."""
    a = _rgba8(rgba8)
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 4 * w), np.uint8)
    rows[:, 1:] = a.reshape(h, 4 * w)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)))
        f.write(_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(_chunk(b"IEND", b""))


def write_ppm(path, rgba8):
    """Binary PPM (P6), top row first; the alpha channel is dropped."""
    a = _rgba8(rgba8)
    h, w = a.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(a[..., :3]).tobytes())
