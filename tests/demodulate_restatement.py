"""Demodulation restated in numpy, from the section's arithmetic: per pixel and colour channel, in f32 with one rounding
per operator,

    demodulate:  d = max(0, rgb - e) / (a + eps)        remodulate:  out = f * (a + eps) + e

e = 0 where the emission image is absent, the divisor 1 where the albedo image is; a pixel with a value of rgb, e or a that is not finite
keeps its rgb bits.  numpy's f32 operators round once each and never fuse, so these arrays are what the host loop and the kernels must
write, byte for byte."""
import numpy as np

F = np.float32


def _parts(rgb, emission, albedo, eps):
    rgb = np.ascontiguousarray(rgb, F)
    e = np.zeros_like(rgb) if emission is None else np.ascontiguousarray(emission, F)
    a = np.zeros_like(rgb) if albedo is None else np.ascontiguousarray(albedo, F)
    with np.errstate(all="ignore"):
        d = np.ones_like(rgb) if albedo is None else a + F(eps)
    ok = (np.isfinite(rgb) & np.isfinite(e) & np.isfinite(a)).all(axis=2, keepdims=True)
    return rgb, e, d, ok


def demodulate(rgb, emission, albedo, eps):
    rgb, e, d, ok = _parts(rgb, emission, albedo, eps)
    with np.errstate(all="ignore"):
        s = rgb - e
        out = np.where(s > F(0), s, F(0)) / d
    return np.where(ok, out, rgb).astype(F)


def remodulate(rgb, emission, albedo, eps):
    rgb, e, d, ok = _parts(rgb, emission, albedo, eps)
    with np.errstate(all="ignore"):
        out = rgb * d + e
    return np.where(ok, out, rgb).astype(F)
