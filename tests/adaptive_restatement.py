"""The adaptive sampler restated in plain Python from the Dart text (samplers/adaptive_sampler.dart), for the tests: the
constructor's normalisation (:40-83), needsSupersampling with method "contrast" (:170-183), and the composition of the
expected film from counter-mode renders of the frozen oracle.  Nothing here imports the product."""
import numpy as np


def round_up_pow2(v):  # common.dart:113-123
    v = int(v) - 1
    for s in (1, 2, 4, 8, 16):
        v |= v >> s
    return v + 1


def is_power_of_2(v):
    return v != 0 and (v & (v - 1)) == 0


def normalise(mins, maxs):
    """AdaptiveSampler's constructor -> (samplesPerPixel, minSamples, maxSamples)."""
    samples_per_pixel = round_up_pow2(max(mins, maxs))  # the super call, :42-43: from the arguments as given
    if mins > maxs:                                     # :53-57
        mins, maxs = maxs, mins
    min_samples = mins if is_power_of_2(mins) else round_up_pow2(mins)  # :59-64
    max_samples = maxs if is_power_of_2(maxs) else round_up_pow2(maxs)  # :66-71
    if min_samples < 2:                                 # :73-77
        min_samples = 2
    if min_samples == max_samples:                      # :79-83
        max_samples *= 2
    return samples_per_pixel, min_samples, max_samples


def luminance(rgb):  # Spectrum.luminance (RGBColor.y): f64 products of the f32 components, summed left to right
    r, g, b = (np.float64(np.float32(c)) for c in rgb)
    return np.float64(0.212671) * r + np.float64(0.715160) * g + np.float64(0.072169) * b


def needs_supersampling(Ls):
    """adaptive_sampler.dart:170-183 for the `count` radiances Ls ([count, 3]) of one pixel."""
    count = len(Ls)
    with np.errstate(divide="ignore", invalid="ignore"):
        Lavg = np.float64(0.0)
        for i in range(count):
            Lavg += luminance(Ls[i])
        Lavg /= count
        max_contrast = 0.5
        for i in range(count):
            if abs(luminance(Ls[i]) - Lavg) / Lavg > max_contrast:
                return True
    return False


def flagged_pixels(pixel_xy, Ls, count):
    """The recorded samples of a render at `count` samples per pixel (pixel-major, a pixel's samples adjacent) ->
    (pixels [n, 2] in trace order, flags [n] bool, black [n] bool)."""
    pixel_xy = np.asarray(pixel_xy, np.int32).reshape(-1, 2)
    Ls = np.asarray(Ls, np.float32).reshape(-1, 3)
    assert len(pixel_xy) == len(Ls) and len(Ls) % count == 0
    px = pixel_xy[::count]
    assert np.array_equal(np.repeat(px, count, axis=0), pixel_xy)
    flags = np.array([needs_supersampling(Ls[k * count:(k + 1) * count]) for k in range(len(px))], bool)
    black = np.array([not Ls[k * count:(k + 1) * count].any() for k in range(len(px))], bool)
    return px, flags, black


def oracle_adaptive(ob, osc, renderer, min_samples, max_samples, pixels=None):
    """The expected result of an adaptive render of `renderer`'s window (or of the raster pixels `pixels`), composed from the
    oracle's counter-mode renders: record Ls at min_samples, decide, then film = (unflagged pixels at min) + (flagged at max).
    Returns dict(pixels, flags, black, flagged (a set of (x, y)), film, rgb)."""
    def desc(spp, px=None):
        rd = ob.render_desc(renderer, sampler_mode=1, pixels=px)
        rd.spp = spp
        return rd

    if pixels is None:
        film = renderer.camera.film
        e = film.getSampleExtent()
        npix = (e[1] - e[0]) * (e[3] - e[2])  # an upper bound of any task's window
    else:
        pixels = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
        npix = len(pixels)
    first = osc.render(desc(min_samples, pixels), record=npix * min_samples)
    assert first["count"] % min_samples == 0 and first["count"] > 0
    px, flags, black = flagged_pixels(first["pixel_xy"], first["Ls"], min_samples)
    if pixels is not None:
        assert np.array_equal(px, pixels)
    # the two conditions every case needs: the flagged set is neither empty nor everything
    assert 0 < flags.sum() < len(px), (int(flags.sum()), len(px))
    low = osc.render(desc(min_samples, px[~flags]))
    high = osc.render(desc(max_samples, px[flags]))
    want = low["film"] + high["film"]
    rgb = np.zeros(want.shape[:2] + (3,), np.float32)
    want = np.ascontiguousarray(want, np.float32)
    ob.lib().orc_film_resolve(want.ctypes.data, want.shape[0] * want.shape[1], rgb.ctypes.data)
    return {"pixels": px, "flags": flags, "black": black, "flagged": set(map(tuple, px[flags].tolist())), "film": want, "rgb": rgb,
            "low": low["film"], "high": high["film"]}
