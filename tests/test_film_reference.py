"""tests/film_reference.py against the oracle, on every case that tests/test_gpu_film.py runs on the device: the restated
film is bit-equal to the oracle's, the derived rounding bound holds for the oracle's own f32 film, and every case holds what it
claims to hold (counted from the recorded samples).  No GPU."""
import numpy as np
import pytest

import film_reference as fr


def _check_reference(ref, integer_table):
    assert ref.oracle_film.tobytes() == ref.serial.tobytes()                 # film_f32_serial == the oracle's film, bit for bit
    assert fr.resolve(ref.oracle_film).tobytes() == ref.oracle_rgb.tobytes()  # resolve == the oracle's writeImage
    assert np.isfinite(ref.oracle_film).all()
    # the bound is a statement about f32 summation: the reference's own serial sum satisfies it
    err, bound = np.abs(ref.oracle_film.astype(np.float64) - ref.sum), fr.bound(ref.S, ref.n)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (ref.oracle_film[ref.n == 0] == 0).all()
    if integer_table:
        # every weight an integer, every partial sum below 2^24: the weight channel is exact in any order
        assert ref.census["max_weight_sum"] < 2 ** 24
        assert np.array_equal(ref.oracle_film[..., 3].astype(np.float64), ref.sum[..., 3])
        assert np.array_equal(ref.sum[..., 3], ref.S[..., 3]) and (ref.sum[..., 3] == np.floor(ref.sum[..., 3])).all()


def _integer(filt):
    return fr.FILTERS[filt][2] or filt.startswith("box")  # a box table is all ones


@pytest.mark.parametrize("c", fr.WIDE_CASES + fr.CROP_CASES + [fr.BATCH_CASE], ids=fr.case_id)
def test_rendered_cases(ob, c):
    ref = fr.reference(ob, c, serial=True)
    _check_reference(ref, _integer(c.filt))
    cs = ref.census
    # blocks: 16 pixels from 64 spp on, 1024 / spp pixels below; more than one, the last one partial.  (The 9 x 7 film of the
    # 1024 spp cases is fixed; under the 1.5 x 2 table its 144 sampled pixels are nine whole blocks.)
    blk = 16 if c.spp >= 64 else 1024 // c.spp
    assert cs["npix"] > blk
    if c.res != (9, 7):
        assert cs["npix"] % 16 != 0 and cs["npix"] % blk != 0
    assert cs["foreign"] > cs["nsamples"]          # the atomic path carries most contributions
    assert cs["pixels_outside"] > 0                # samples of pixels outside the window reach into it
    assert cs["classes"][fr.ORDINARY] == cs["nsamples"]
    if c.crop != fr.FULL:
        film = fr.make_film(c)
        assert film.left > 0 and film.top > 0 and cs["pixels_outside"] > film.width + film.height  # left of and above it too
    if c is fr.BATCH_CASE:
        assert cs["nsamples"] > 3 * 2 ** 16        # at least four batches of 2^16 slots


def test_the_1024_spp_films_keep_a_partial_block(ob):
    assert sorted(fr.reference(ob, c).census["npix"] % 16 for c in fr.WIDE_CASES if c.spp == 1024) == [0, 8, 8, 12]


@pytest.mark.parametrize("c", fr.GUARD_CASES, ids=fr.case_id)
def test_guard_cases(ob, c):
    ref = fr.reference(ob, c, serial=True)
    _check_reference(ref, True)
    cs = ref.census
    want = (fr.G_NEGATIVE,) if c.scene == "negative" else (fr.G_NAN, fr.G_NEGATIVE, fr.G_INFINITE)
    for g in want:
        assert cs["classes"][g] > cs["nsamples"] // 20, (g, cs["classes"])
        assert cs["mixed"][g] > 20, (g, cs["mixed"])   # window pixels with a guarded sample of the class beside lit ordinary ones
    assert cs["classes"][fr.ORDINARY] > cs["nsamples"] // 5
    # guarded samples add their weight and no XYZ: under the 0.5 box every window pixel's weight sum is spp
    if c.filt == "box0.5":
        assert (ref.sum[..., 3] == c.spp).all()


def test_guard_classes_by_hand():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    Ls = np.array([[1, 2, 3], [nan, 1, 1], [1, 1, nan], [-1, 0, 0], [-1e-4, 0, 0], [-1e-6, 0, 0], [inf, 0, 0], [0, inf, 1],
                   [-inf, 1, 1], [inf, -inf, 0], [inf, 1, nan], [3.3e38, 3.3e38, 3.3e38]], np.float32)
    assert list(fr.guard_class(Ls)) == [0, 1, 1, 2, 2, 0, 3, 3, 2, 0, 1, 0]   # (inf, -inf, 0): the luminance is NaN, no channel is
    v = fr.sample_values(Ls)
    assert (v[[1, 2, 3, 4, 6, 7, 8, 10], :3] == 0).all() and (v[:, 3] == 1).all()
    assert np.isnan(v[9, :3]).all()                   # no guard catches it: NaN < -1e-5 and NaN.isInfinite are both false
    assert np.isinf(v[11, 2]) and np.isfinite(v[11, 1])  # finite luminance, Z overflows its f32 store: kept
    assert v[0, 1] == np.float32(0.212671 * 1 + 0.715160 * 2 + 0.072169 * 3)


@pytest.mark.parametrize("c", fr.PLACED_CASES, ids=fr.placed_id)
def test_hand_placed_cases(ob, c):
    ref = fr.placed_reference(ob, c)
    _check_reference(ref, True)
    cs = ref.census
    assert cs["npix"] == 19 * 14 and cs["npix"] > (16 if c.spp >= 64 else 1024 // c.spp) and cs["npix"] % 16 != 0
    assert cs["pixels_outside"] == 2 * 19 + 2 * 12
    if not c.zeros:
        # no coordinate on 0.0: every sample stays in its own pixel, nothing reaches the atomics, index 16 cannot occur
        assert cs["sx_zero"] == cs["sy_zero"] == cs["foreign"] == cs["index16"] == 0
        assert cs["contributions"] == 17 * 12 * c.spp
        return
    assert cs["sx_zero"] > cs["nsamples"] // 10 and cs["sy_zero"] > cs["nsamples"] // 10
    assert cs["foreign"] > 0
    if c.filt == "box0.5":
        # a coordinate of exactly 0.0 is half a pixel from two pixel centres: the sample counts for both (width 0.5: index 16)
        assert cs["contributions"] > 17 * 12 * c.spp and cs["col15_from16"] > 0 and cs["row15_from16"] > 0
        assert ref.sum[..., 3].max() > c.spp
    else:
        # integer x width 1 (and y width 2): sx = 0.5 puts pixels at exactly one filter width, index 16 before the clamp
        assert cs["col15_from16"] > cs["nsamples"] // 10 and cs["row15_from16"] > cs["nsamples"] // 10
    if c.filt == "int1.5x2":
        assert cs["negative_coords"] == 19 + 14 - 1   # the uncropped window's ring has the coordinate -1


def test_resolve_by_hand():
    f = np.array([[1, 1, 1, 2], [1, 1, 1, 0], [0, 1, 0, 1], [np.nan, 1, 1, 1], [1, 1, 1, -2], [-0.0, -0.0, -0.0, 1], [1, 1, 1, 1e-45],
                  [np.inf, 0, 0, 1]], np.float32)
    rgb = fr.resolve(f)
    assert rgb[0, 0] == np.float32((3.240479 - 1.537150 - 0.498535) * 0.5)
    assert rgb[1].tobytes() == np.zeros(3, np.float32).tobytes()
    assert rgb[2, 0] == 0 and rgb[2, 1] == np.float32(1.875991) and rgb[2, 2] == 0
    assert rgb[3].tobytes() == np.zeros(3, np.float32).tobytes()           # max(0.0, NaN) answers 0.0
    assert rgb[4].tobytes() == np.zeros(3, np.float32).tobytes()           # positive XYZ over a negative weight sum
    assert rgb[5].tobytes() == np.zeros(3, np.float32).tobytes()           # +0.0, whatever the sign of the sums
    assert np.isinf(rgb[6]).all() and (rgb[6] > 0).all()                   # 1 / denormal overflows f32
    assert np.isinf(rgb[7, 0]) and rgb[7, 1] == 0 and np.isinf(rgb[7, 2])


def test_resolve_equals_the_oracle_on_hand_made_films(ob):
    for n in fr.RESOLVE_SIZES:
        f = fr.resolve_film(n)
        out = np.zeros((n, 3), np.float32)
        ob.lib().orc_film_resolve(f.ctypes.data, n, out.ctypes.data)
        assert fr.resolve(f).tobytes() == out.tobytes()
    # what the largest film holds
    w, xyz = f[:, 3], f[:, :3]
    rgb = fr.resolve(f)
    assert (w == 0).any() and (w < 0).any() and ((w != 0) & (np.abs(w) < 1.1754944e-38)).any() and (np.abs(w) > 1e30).any()
    assert np.isnan(w).any() and np.isinf(w).any() and np.isnan(xyz).any() and np.isposinf(xyz).any() and np.isneginf(xyz).any()
    assert (np.signbit(xyz) & (xyz == 0)).any()
    ordinary = np.isfinite(f).all(axis=1) & (w > 1e-3) & (w < 1e3)
    x = np.where(ordinary[:, None], xyz, 0).astype(np.float64)
    c = np.stack([3.240479 * x[:, 0] - 1.537150 * x[:, 1] - 0.498535 * x[:, 2],
                  -0.969256 * x[:, 0] + 1.875991 * x[:, 1] + 0.041556 * x[:, 2],
                  0.055648 * x[:, 0] - 0.204043 * x[:, 1] + 1.057311 * x[:, 2]], axis=1)
    for ch in range(3):
        assert (ordinary & (c[:, ch] < 0)).any() and (ordinary & (c[:, ch] > 0)).any()   # each channel clamped somewhere
    assert not np.signbit(rgb[rgb == 0]).any() and (rgb > 0).any() and np.isinf(rgb).any()
