"""k_film and k_film_resolve against tests/film_reference.py (which tests/test_film_reference.py proves against the oracle), on
every accumulation path: the serial and the unrolled chain (spp < 64), the tiled passes (spp >= 64), own pixel (ordered LDS
chain) and neighbours (f32 atomics), crop windows, several batches, image samples on exactly 0.0 and 0.5, the three radiance
guards, and resolve on films no render produces.

Two comparisons.  EXACT: under a filter table of 256 distinct integers every weight and every partial sum of the weight channel
is an integer below 2^24, so film[..., 3] must equal the f64 reference bit for bit whatever the order of the atomics: one lost,
doubled, misplaced or mis-indexed contribution shows.  BOUNDED: |device - f64 sum| <= (2 n + 4) 2^-24 S per (pixel, channel), n
contributions of magnitude sum S (film_reference.bound: derived, not fitted); exactly 0 where n == 0."""
import numpy as np
import pytest

import film_reference as fr
from dartray_amd import _abi, scenes

pytestmark = pytest.mark.gpu


def _check(out, ref, exact_weight):
    film = out.film
    assert film.shape == ref.sum.shape
    assert (film[ref.n == 0] == 0).all()
    err, bound = np.abs(film.astype(np.float64) - ref.sum), fr.bound(ref.S, ref.n)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("max |device - f64| / bound = %.4f (oracle's own film: %.4f), contributions per pixel <= %d"
          % (ratio, float((np.abs(ref.oracle_film - ref.sum) / np.maximum(bound, 1e-300)).max()), int(ref.n.max())))
    if exact_weight:
        assert ref.sum[..., 3].max() < 2 ** 24   # the precondition, from the reference
        assert film[..., 3].tobytes() == ref.sum[..., 3].astype(np.float32).tobytes()
    assert np.isfinite(film).all()
    assert (err <= bound).all(), ratio
    assert out.rgb.tobytes() == fr.resolve(film).tobytes()


def _exact(filt):
    return fr.FILTERS[filt][2] or filt.startswith("box")  # integer table, or the box filter's table of ones


@pytest.mark.parametrize("c", fr.WIDE_CASES + fr.CROP_CASES, ids=fr.case_id)
def test_wide_filters_on_every_accumulation_path(ob, gpu, c):
    """spp 1 / 4 (serial chain), 8 / 32 (unrolled chain), 64 (one tiled pass), 128 / 1024 (2 / 16 passes over the same LDS rows);
    full and cropped windows (sampled pixels left of and above the window)."""
    prims, r = fr.make_case(c)
    ref = fr.reference(ob, c)
    out = r.render(scenes.make_scene(prims))
    _check(out, ref, _exact(c.filt))


def test_wide_filter_over_several_batches(ob, gpu):
    """A pixel's contributions then come from blocks of different launches; the exact weight channel is the single-batch one."""
    c = fr.BATCH_CASE
    prims, r = fr.make_case(c)
    ref = fr.reference(ob, c)
    scene = scenes.make_scene(prims)
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(b"BATCH_BITS", b""))  # ("" hides the environment's value)
        whole = r.render(scene)
        assert r.last_stats["batches"] == 1
        _abi.check(lib.dr_set_option(b"BATCH_BITS", b"16"))
        out = r.render(scene)
        assert r.last_stats["batches"] >= 3
    finally:
        _abi.check(lib.dr_set_option(b"BATCH_BITS", None))
    _check(whole, ref, True)
    _check(out, ref, True)
    assert out.film[..., 3].tobytes() == whole.film[..., 3].tobytes()


@pytest.mark.parametrize("c", fr.PLACED_CASES, ids=fr.placed_id)
def test_hand_placed_image_samples(ob, gpu, c):
    """Image samples on 0.0, 2^-24, 0.25, 0.5 and the last f32 below 1, in the window's corners, edges, interior and the ring of
    pixels around it.  sx == 0.0 is half a pixel from two centres (the 0.5 box then counts the sample for both); under integer
    widths sx == 0.5 puts pixels at exactly one filter width: table index 16 before the clamp, column / row 15 after it (the
    integer table tells the cells apart)."""
    prims, r, sx, sy, Ls = fr.make_placed(ob, c)
    ref = fr.placed_reference(ob, c)
    out = r.render(scenes.make_scene(prims))
    _check(out, ref, True)
    if not c.zeros:
        # every sample stays in its own pixel: the ordered chain alone, the whole film bit-equal to the reference's serial sum
        assert out.film.tobytes() == ref.serial.tobytes()
    elif c.filt == "box0.5":
        assert out.film[..., 3].max() > c.spp   # the two-pixel spread


@pytest.mark.parametrize("c", fr.GUARD_CASES, ids=fr.case_id)
def test_radiance_guards(ob, gpu, c):
    """Emitters of negative and of +-infinite radiance: samples whose radiance is NaN (inf - inf), of luminance < -1e-5 or of
    infinite luminance add their filter weight and no XYZ (sampler_renderer.dart:181-193), beside ordinary samples in the same
    pixels.  dr_scene_create takes non-finite colours as they are."""
    prims, r = fr.make_case(c)
    ref = fr.reference(ob, c, serial=c.filt == "box0.5")
    out = r.render(scenes.make_scene(prims))
    _check(out, ref, True)
    if c.filt == "box0.5":
        assert out.film.tobytes() == ref.serial.tobytes()
        assert (out.film[..., 3] == c.spp).all()


@pytest.mark.parametrize("n", fr.RESOLVE_SIZES)
def test_resolve_of_hand_made_films(gpu, n):
    """dr_film_resolve_device on zero, negative, denormal, huge and non-finite weight sums and on XYZ that make each rgb channel
    negative, -0.0, NaN, +-inf: bit-equal to writeImage's restatement, the signs of zeros included."""
    import torch
    host = fr.resolve_film(n)
    film = torch.from_numpy(host).cuda()
    rgb = torch.full((n + 1, 3), 7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _abi.check(_abi.lib().dr_film_resolve_device(film.data_ptr(), n, rgb.data_ptr(), stream))
    torch.cuda.synchronize()
    got = rgb.cpu().numpy()
    assert got[:n].tobytes() == fr.resolve(host).tobytes()
    assert (got[n] == 7.0).all()   # nothing past the last pixel
