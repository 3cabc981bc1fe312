"""The display transform without a GPU: answers derived by hand, checked against both the numpy restatement
(tests/display_restatement.py, written from the text) and dr_display_host after those two agree byte for byte; the tables; the two against
each other on seeded images full of non-finite, negative, subnormal and huge values; every refusal by code and text; the exposure pick's
corner counts; the PNG writer, decoded with zlib and struct alone; the host code under the address and undefined-behaviour sanitizers as a
stand-alone program (tests/display_host_check.cpp); and the Python module above them (dartray_amd/display.py).  The command line's PNG leg
needs a render, and a render needs a GPU: it is in tests/test_gpu_display.py."""
import ctypes as C
import math
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, display

import display_cases as dc
import display_restatement as dr

F = np.float32
same = dr.same_bytes
CLAMP, REINHARD, FILMIC = dc.CURVES
SRGB, GAMMA22, REFERENCE = dc.ENCODES


def _both(rgb, curve, encode, auto, permille=500, exposure=1.0, inv_white2=0.0, key=0.18):
    """The restatement's and the host entry's bytes, which must agree before either is compared with a derived answer."""
    rgb = np.asarray(rgb, np.float32)
    want, _ = dr.display(rgb, curve, encode, dc.table(encode), auto, permille, exposure, key, inv_white2, dc.INVALID_RGBA)
    got = dc.host(rgb, dc.params(curve, encode, auto, permille, exposure, inv_white2, key))
    assert same(got, want)
    return got


def _grey(v):
    return np.full((1, 1, 3), v, np.float32)


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


# ---- 1. answers derived by hand ----
def test_known_codes_of_the_three_encodes(hip):
    """Curve clamp, scale 1, grey pixels.  0 is below every threshold: code 0.  1 and 5 are above the last one (the linear value of
    254.5 / 255, about 0.996): code 255.  The code is round(255 * encoded), so with e = 1.055 * x^(1 / 2.4) - 0.055 (x > 0.0031308) or 12.92 * x:
      sRGB:      0.25 -> 255 * 0.53710 = 136.96 -> 137;  0.05 -> 255 * 0.24780 = 63.19 -> 63;  0.002 -> 255 * 0.02584 = 6.59 -> 7
      gamma 2.2: 0.25^(1 / 2.2) = 0.53253, * 255 = 135.80 -> 136;  0.05^(1 / 2.2) = 0.25623, * 255 = 65.34 -> 65
    Every one is 0.09 of a code or more from the next threshold, while 1e-3 relative in x moves 255 * e by at most 0.06 at these values.
    The reference encode quantises first: 1.0 -> q = 255 -> G[255] = floor(1 * 255) = 255;  0.5 -> q = floor(127.5) = 127 ->
    G[127] = floor((127 / 255)^(1 / 2.2) * 255) = floor(0.72844 * 255) = floor(185.75) = 185."""
    for encode in dc.ENCODES:
        assert _both(_grey(0.0), CLAMP, encode, 0)[0, 0].tolist() == [0, 0, 0, 255]
        for v in (1.0, 5.0, 1e30):
            assert _both(_grey(v), CLAMP, encode, 0)[0, 0].tolist() == [255, 255, 255, 255]
    for v, code in ((0.25, 137), (0.05, 63), (0.002, 7)):
        assert _both(_grey(v), CLAMP, SRGB, 0)[0, 0].tolist() == [code] * 3 + [255]
    for v, code in ((0.25, 136), (0.05, 65)):
        assert _both(_grey(v), CLAMP, GAMMA22, 0)[0, 0].tolist() == [code] * 3 + [255]
    assert _both(_grey(0.5), CLAMP, REFERENCE, 0)[0, 0].tolist() == [185, 185, 185, 255]
    # a manual exposure is a plain factor: 0.5 at scale 0.5 is 0.25 at scale 1, exactly
    assert _both(_grey(0.5), CLAMP, SRGB, 0, exposure=0.5)[0, 0].tolist() == [137, 137, 137, 255]
    # the channels are encoded one by one, in the order r, g, b
    assert _both(np.array([[[0.25, 0.05, 0.002]]], np.float32), CLAMP, SRGB, 0)[0, 0].tolist() == [137, 63, 7, 255]


def test_plain_reinhard_maps_luminance_one_to_one_half(hip):
    """The three luminance weights sum to 1.0f in f32 in the order they are added, so lum(1, 1, 1) = 1 exactly.  Yd = (1 * (1 + 1 * 0)) /
    (1 + 1) = 0.5, m = 0.5 / 1, and every channel is 1 * 0.5 = 0.5 exactly: the codes are those of 0.5 under the clamp curve.  With
    white = 1 (inv_white2 = 1) Yd = (1 * (1 + 1)) / 2 = 1: white itself maps to 1, code 255.  Y' = 0 gives 0."""
    assert dr.lum(_grey(1.0))[0, 0] == F(1.0)
    with np.errstate(all="ignore"):
        assert (dr.curve_of(_grey(1.0), REINHARD, 0.0) == F(0.5)).all()
    for encode in dc.ENCODES:
        assert same(_both(_grey(1.0), REINHARD, encode, 0), _both(_grey(0.5), CLAMP, encode, 0))
        assert _both(_grey(1.0), REINHARD, encode, 0, inv_white2=1.0)[0, 0].tolist() == [255, 255, 255, 255]
        assert _both(_grey(0.0), REINHARD, encode, 0)[0, 0].tolist() == [0, 0, 0, 255]
    assert _both(_grey(1.0), REINHARD, SRGB, 0)[0, 0, 0] == 188     # 255 * 0.73536 = 187.52: close to a threshold, so only as a cross-check


def test_filmic_at_zero_is_zero_and_saturates(hip):
    """x = 0: (0 * 0.03) / (0 * 0.59 + 0.14) = 0 / 0.14 = 0.  x = 10: 10 * 25.13 / (10 * 24.89 + 0.14) = 251.3 / 249.04 > 1: code 255."""
    for encode in dc.ENCODES:
        assert _both(_grey(0.0), FILMIC, encode, 0)[0, 0].tolist() == [0, 0, 0, 255]
        assert _both(_grey(10.0), FILMIC, encode, 0)[0, 0].tolist() == [255, 255, 255, 255]


def test_powers_of_two_land_in_the_predicted_bins_and_the_median_follows(hip):
    """Grey pixels 2^e have luminance 2^e exactly (the weights sum to 1.0f; a power of two only shifts the exponent), whose bits are
    (e + 127) << 23: bin (e + 127) * 8.  Nine pixels, e = -4 .. 4: n = 9, permille 500 gives rank = 8 * 500 / 1000 = 4, the fifth pixel,
    e = 0, bin 1016.  Its centre has the bits 1016 << 20 | 1 << 19 = 0x3f880000 = 1.0625, and scale = 0.18f / 1.0625f.  permille 0 picks
    e = -4 (bin 984, centre 0.0625 * 1.0625), permille 1000 rank 8, e = 4 (bin 1048, centre 17)."""
    e = np.arange(-4, 5)
    img = np.repeat((2.0 ** e).astype(np.float32), 3).reshape(3, 3, 3)
    lib = hip.lib()
    want = np.zeros(2048, np.uint32)
    want[(e + 127) * 8] = 1
    for permille, centre in ((500, 1.0625), (0, 0.0625 * 1.0625), (1000, 17.0), (499, 0.5 * 1.0625), (625, 2.0 * 1.0625)):
        rc, bits, hist = dc.exposure(lib.dr_display_exposure_host, img, dc.params(CLAMP, SRGB, 1, permille))
        assert rc == 0 and same(hist, want) and same(dr.histogram(img), want)
        assert bits == _bits(F(0.18) / F(centre)) == _bits(dr.pick(want, permille, 0.18)), (permille, bits)
    # the picked scale is the one the transform uses: auto-exposure equals the manual exposure of that value
    p_auto, p_manual = dc.params(FILMIC, SRGB, 1, 500), dc.params(FILMIC, SRGB, 0, 500, exposure=float(F(0.18) / F(1.0625)))
    assert same(dc.host(img, p_auto), dc.host(img, p_manual))
    _both(img, FILMIC, SRGB, 1)


# ---- 2. the tables ----
def test_tables(hip):
    for encode in (SRGB, GAMMA22):
        t = dc.table(encode)
        assert t.dtype == np.float32 and t[0] == 0 and (np.diff(t[1:]) > 0).all() and t[1] > 0
        t64 = dr.thresholds(encode)
        assert (np.abs(t.astype(np.float64) - t64) <= np.spacing(t)).all()     # within one f32 ulp of numpy's f64 value
        assert 0.99 < t[255] < 1.0
    assert abs(dc.table(SRGB)[1] - 0.5 / 255 / 12.92) < 1e-9 and abs(dc.table(GAMMA22)[128] - 0.5 ** 2.2) < 1e-7
    g = dc.table(REFERENCE)
    assert g.dtype == np.uint8 and g[0] == 0 and g[255] == 255 and (np.diff(g.astype(int)) >= 0).all()
    assert g.tolist() == [min(max(math.floor(math.pow(i / 255.0, 1.0 / 2.2) * 255.0), 0), 255) for i in range(256)]
    for name, encode in (("srgb", SRGB), ("gamma22", GAMMA22), ("reference", REFERENCE)):
        assert same(display.tables(name), dc.table(encode))
    lib = hip.lib()
    words = np.zeros(256, np.uint32)
    for args, needle in (((3, words.ctypes.data, 256), "encode must be"), ((0, None, 256), "a null pointer"), ((0, words.ctypes.data, 255), "n must be 256")):
        assert lib.dr_display_table(*args) == -1 and needle in lib.dr_last_error().decode()


# ---- 3. host == restatement, byte for byte, no pixel exempted ----
@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_byte_for_byte(hip, size):
    img = dc.images(*size)
    outs = [_both(img, curve, encode, auto, permille, exposure, iw) for curve, encode, (auto, permille, exposure, iw) in dc.COMBOS]
    if size == (64, 64):
        bad = ~np.isfinite(img).all(axis=2)
        assert 100 < bad.sum() < 2000
        for out in outs:                                                # invalid pixels are invalid_rgba, valid ones opaque
            assert (out[bad] == [0xC0, 0x10, 0xFF, 0x80]).all() and (out[~bad][:, 3] == 255).all()
        distinct = {o.tobytes() for o in outs}
        assert len(distinct) == len(outs)                               # no parameter is ignored on both sides


def test_the_cases_hold_what_they_promise():
    img = dc.images(64, 64)
    fin = np.isfinite(img)
    assert np.isnan(img).any() and (img == np.inf).any() and (img == -np.inf).any() and (img[fin] < 0).any() and (img == 0).any()
    tiny = fin & (img != 0) & (np.abs(img) < 1.17549435e-38)
    assert tiny.any() and (img[fin] >= 1e30).any() and np.signbit(img[img == 0]).any()
    hist = dr.histogram(img)
    assert hist.sum() < 64 * 64 - (~fin.all(axis=2)).sum()              # some valid pixels are not counted: zero or subnormal luminance
    with np.errstate(all="ignore"):
        assert np.isnan(dr.curve_of(dr.floored(img) * F(1e8), FILMIC, 0.0)[fin.all(axis=2)]).any()    # an overflow on the way makes a NaN
    assert (dr.histogram(dc.ramp(67, 31))[8:2040] >= 1).all() and dr.histogram(dc.ramp(67, 31)).sum() == 67 * 31
    assert dr.histogram(dc.all_invalid(17, 5)).sum() == 0 and dr.histogram(dc.one_valid(17, 5)).sum() == 1
    assert np.count_nonzero(dr.histogram(dc.flat(17, 5))) == 1


@pytest.mark.parametrize("name", sorted(dc.WORST))
def test_worst_case_images_on_the_host(hip, name):
    img = dc.WORST[name](67, 31)
    for curve, encode, (auto, permille, exposure, iw) in dc.COMBOS[::5]:
        _both(img, curve, encode, auto, permille, exposure, iw)


def test_a_nan_made_on_the_way_is_white(hip):
    """A finite channel times the scale may overflow, and the curves then form inf / inf: the result is taken as +inf, the largest code."""
    img = np.array([[[3e38, 1.0, 0.0]]], np.float32)
    assert _both(img, FILMIC, SRGB, 0, exposure=10.0)[0, 0].tolist()[0] == 255
    assert _both(img, REINHARD, REFERENCE, 0, exposure=10.0)[0, 0].tolist() == [255, 255, 255, 255]   # Y' = inf: m is a NaN, and 0 * NaN too


# ---- 4. the exposure pick's corners ----
def test_exposure_counts_and_corners(hip):
    lib = hip.lib()
    p = dc.params(CLAMP, SRGB, 1, 500)
    rc, bits, hist = dc.exposure(lib.dr_display_exposure_host, dc.all_invalid(5, 3), p)
    assert rc == 0 and bits == _bits(1.0) and hist.sum() == 0           # n == 0: scale 1
    zeros = np.zeros((2, 2, 3), np.float32)
    zeros[0, 0] = 1e-39                                                 # zero and subnormal luminances are not counted
    rc, bits, hist = dc.exposure(lib.dr_display_exposure_host, zeros, p)
    assert rc == 0 and bits == _bits(1.0) and hist.sum() == 0
    big = np.full((1, 2, 3), np.finfo(np.float32).max, np.float32)     # the weights sum to 1 + 7e-9: the largest grey keeps a finite luminance
    rc, bits, hist = dc.exposure(lib.dr_display_exposure_host, big, p)
    assert rc == 0 and hist[2039] == 2 and hist.sum() == 2 and same(hist, dr.histogram(big))
    assert bits == _bits(F(0.18) / np.array([(2039 << 20) | (1 << 19)], np.uint32).view(np.float32)[0])
    img = dc.images(17, 33)
    want = dr.histogram(img)
    occupied = np.nonzero(want)[0]
    for permille, b in ((0, occupied[0]), (1000, occupied[-1])):        # the first and the last occupied bin
        rc, bits, hist = dc.exposure(lib.dr_display_exposure_host, img, dc.params(CLAMP, SRGB, 1, permille, key=0.5))
        centre = np.array([(int(b) << 20) | (1 << 19)], np.uint32).view(np.float32)[0]
        assert rc == 0 and same(hist, want) and bits == _bits(F(0.5) / centre)
    rc, bits, none = dc.exposure(lib.dr_display_exposure_host, img, dc.params(CLAMP, SRGB, 1, 1000, key=0.5), want_hist=False)
    assert rc == 0 and none is None and bits == _bits(F(0.5) / centre)
    # auto_exposure itself is not read by the exposure entry
    assert dc.exposure(lib.dr_display_exposure_host, img, dc.params(CLAMP, SRGB, 0, 1000, key=0.5))[1] == bits


# ---- 5. the refusals, by code and text ----
def test_every_refusal_by_code_and_text(hip):
    lib = hip.lib()
    nan, inf = float("nan"), float("inf")

    def refused(needle, w=3, h=2, **kw):
        base = dict(curve=REINHARD, encode=SRGB, auto=1, permille=500, exposure=1.0, inv_white2=0.0, key=0.18)
        base.update(kw)
        p = dc.params(**base)
        assert lib.dr_display_check(C.byref(p), w, h) == -1, needle
        text = lib.dr_last_error().decode()
        assert needle in text and text.startswith("dr_display_check: "), (needle, text)
        img, out = np.zeros((2, 3, 3), np.float32), np.zeros((2, 3, 4), np.uint8)
        for fn in (lib.dr_display_host, lib.dr_display):              # the same checks, ahead of any device call
            assert fn(img.ctypes.data, w, h, C.byref(p), out.ctypes.data) == -1 and needle in lib.dr_last_error().decode(), needle

    assert lib.dr_display_check(C.byref(dc.params(REINHARD, SRGB, 1)), 3, 2) == 0
    assert lib.dr_display_check(C.byref(dc.params(FILMIC, REFERENCE, 0, 1000, 1e-30, 3e38, 1e-30)), 2 ** 31 - 1, 1) == 0
    assert lib.dr_display_check(None, 3, 2) == -1 and "a null pointer" in lib.dr_last_error().decode()
    refused("curve must be DR_TONE_CLAMP, DR_TONE_REINHARD or DR_TONE_FILMIC", curve=3)
    refused("encode must be DR_ENCODE_SRGB, DR_ENCODE_GAMMA22 or DR_ENCODE_REFERENCE", encode=3)
    refused("encode must be", encode=2 ** 32 - 1)
    refused("permille must be in 0..1000", permille=1001)
    for bad in (0.0, -0.0, -1.0, inf, nan):
        refused("exposure must be finite and positive", exposure=bad)
        refused("key must be finite and positive", key=bad)
    for bad in (-1e-6, -inf, inf, nan):
        refused("inv_white2 must be finite and not negative", inv_white2=bad)
    refused("w and h must be at least 1", w=0)
    refused("w and h must be at least 1", h=0)
    refused("w and h must be at least 1", w=-3)
    refused("the image has 2^31 or more pixels", w=65536, h=32768)
    refused("the image has 2^31 or more pixels", w=2 ** 31 - 1, h=2)
    img, out, ok = np.zeros((2, 3, 3), np.float32), np.zeros((2, 3, 4), np.uint8), dc.params(REINHARD, SRGB, 1)
    scale, hist = C.c_float(0), np.zeros(2048, np.uint32)
    for fn in (lib.dr_display_host, lib.dr_display):
        for args in ((None, 3, 2, C.byref(ok), out.ctypes.data), (img.ctypes.data, 3, 2, None, out.ctypes.data), (img.ctypes.data, 3, 2, C.byref(ok), None)):
            assert fn(*args) == -1 and "a null pointer" in lib.dr_last_error().decode()
        assert fn(img.ctypes.data, 3, 2, C.byref(ok), img.ctypes.data + 71) == -1 and "out overlaps an input" in lib.dr_last_error().decode()
        assert fn(img.ctypes.data + 23, 3, 2, C.byref(ok), img.ctypes.data) == -1 and "out overlaps an input" in lib.dr_last_error().decode()
    for fn in (lib.dr_display_exposure_host, lib.dr_display_exposure):
        for args in ((None, 3, 2, C.byref(ok), C.byref(scale), hist.ctypes.data), (img.ctypes.data, 3, 2, None, C.byref(scale), None),
                     (img.ctypes.data, 3, 2, C.byref(ok), None, hist.ctypes.data)):
            assert fn(*args) == -1 and "a null pointer" in lib.dr_last_error().decode()
        assert fn(img.ctypes.data, 3, 0, C.byref(ok), C.byref(scale), None) == -1 and "w and h must be at least 1" in lib.dr_last_error().decode()
    # the device entry: the same checks and its own, all ahead of any device call; the size query needs no device
    dev, n = lib.dr_display_device, C.c_uint64(0)
    assert dev(None, 129, 65, C.byref(ok), None, None, C.byref(n), None) == 0 and n.value == 2048 * 4 + 16
    assert dev(None, 129, 65, C.byref(ok), None, None, None, None) == -1 and "a null pointer" in lib.dr_last_error().decode()
    assert dev(None, 129, 65, None, None, None, C.byref(n), None) == -1 and "a null pointer" in lib.dr_last_error().decode()
    assert dev(None, 0, 65, C.byref(ok), None, None, C.byref(n), None) == -1 and "w and h must be at least 1" in lib.dr_last_error().decode()
    assert dev(None, 3, 2, C.byref(dc.params(REINHARD, SRGB, 1, 1001)), None, None, C.byref(n), None) == -1
    assert "permille must be in 0..1000" in lib.dr_last_error().decode()
    fake, need = 1 << 20, 2048 * 4 + 16                                 # addresses that are only compared, never read
    for args, needle in (((None, 3, 2, C.byref(ok), 2 * fake, 3 * fake, C.c_uint64(need)), "a null pointer"),
                         ((fake, 3, 2, C.byref(ok), None, 3 * fake, C.c_uint64(need)), "a null pointer"),
                         ((fake, 3, 2, C.byref(ok), 2 * fake, 3 * fake, C.c_uint64(need - 1)), "the scratch buffer is too small"),
                         ((fake, 3, 2, C.byref(ok), 2 * fake, 3 * fake + 4, C.c_uint64(need)), "not 16-byte aligned"),
                         ((fake, 3, 2, C.byref(ok), 2 * fake + 2, 3 * fake, C.c_uint64(need)), "out is not 4-byte aligned"),
                         ((fake, 3, 2, C.byref(ok), 3 * fake + need - 4, 3 * fake, C.c_uint64(need)), "out overlaps the scratch buffer"),
                         ((3 * fake - 4, 3, 2, C.byref(ok), 2 * fake, 3 * fake, C.c_uint64(need)), "rgb overlaps the scratch buffer"),
                         ((fake, 3, 2, C.byref(ok), fake + 68, 3 * fake, C.c_uint64(need)), "out overlaps an input")):
        a = list(args)
        a[6] = C.byref(a[6])
        assert dev(*a, None) == -1 and needle in lib.dr_last_error().decode(), (needle, lib.dr_last_error())


# ---- 6. the image files ----
def _png_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        (n,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xffffffff, kind
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data)
    return chunks


def decode_png(path):
    """An 8-bit RGBA, non-interlaced PNG whose scanlines all have filter type 0 -> [h, w, 4] uint8, with zlib and struct alone."""
    chunks = _png_chunks(open(path, "rb").read())
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"") and len(chunks[0][1]) == 13
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 6, 0, 0, 0)
    raw = zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT"))
    assert len(raw) == h * (1 + 4 * w)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 4 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 4).copy()


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (67, 31)], ids=lambda s: "%dx%d" % s)
def test_png_and_ppm_round_trip(tmp_path, size):
    w, h = size
    rgba = np.random.Generator(np.random.PCG64(w)).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    display.write_png(path, rgba)
    assert same(decode_png(path), rgba)
    assert [kind for kind, _ in _png_chunks(open(path, "rb").read())] == [b"IHDR", b"IDAT", b"IEND"]
    ppm = str(tmp_path / "a.ppm")
    display.write_ppm(ppm, rgba)
    data = open(ppm, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data[:len(head)] == head and data[len(head):] == rgba[..., :3].tobytes()
    for bad in (rgba.astype(np.float32), rgba[..., :3], rgba[0]):
        with pytest.raises(ValueError, match=r"must be uint8 \[h, w, 4\]"):
            display.write_png(path, bad)


# ---- 7. the host code under the sanitizers, as a program of its own ----
def test_host_transform_runs_clean_under_the_sanitizers(tmp_path):
    """tests/display_host_check.cpp + dr_display_host.cpp, built with -fsanitize=address,undefined and run as a child process; the
    sanitizer runtimes are linked into the program, which then depends on nothing else the process loads."""
    exe = str(tmp_path / "display_host_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "display_host_check.cpp"),
                           os.path.join(ROOT, "dartray_amd", "csrc", "dr_display_host.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "display_host_check: OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ---- 8. the Python module ----
def test_the_defaults_are_the_documented_ones():
    p = display.params()
    assert (p.curve, p.encode, p.auto_exposure, p.permille, p.exposure, p.key, p.inv_white2, p.invalid_rgba) == \
        (REINHARD, SRGB, 1, 500, 1.0, float(F(0.18)), 0.0, 0xff000000)
    assert C.sizeof(_abi.DrDisplayParams) == 32
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "exposure = None, key = 0.18, percentile = 0.5, curve = \"reinhard\", white = inf, encode = \"srgb\", invalid = (0, 0, 0, 255)" in design
    assert display.inv_white2(float("inf")) == 0.0 and display.inv_white2(2.0) == 0.25 and display.inv_white2(0.3) == float(F(1.0 / 0.09))
    p = display.params(exposure=2.5, percentile=0.25, curve="filmic", white=4.0, encode="reference", invalid=(1, 2, 3, 4))
    assert (p.curve, p.encode, p.auto_exposure, p.permille, p.exposure, p.inv_white2, p.invalid_rgba) == (FILMIC, REFERENCE, 0, 250, 2.5, 0.0625, 0x04030201)
    for kw, needle in ((dict(white=0.0), "white must be positive"), (dict(curve="aces"), "curve must be one of"), (dict(encode="rec709"), "encode must be one of"),
                       (dict(percentile=1.5), "percentile must be in 0..1"), (dict(invalid=(0, 0, 256, 0)), "invalid must be four bytes")):
        with pytest.raises(ValueError, match=needle):
            display.params(**kw)


def test_the_module_on_the_host_equals_the_restatement(hip):
    img = dc.images(17, 33)
    got = display.tonemap(img, device=False)
    assert got.dtype == np.uint8 and got.shape == (33, 17, 4)
    assert same(got, dr.display(img, REINHARD, SRGB, dc.table(SRGB), True, 500, 1.0, 0.18, 0.0, 0xff000000)[0])
    got = display.tonemap(img, exposure=0.5, curve="filmic", encode="reference", invalid=(9, 8, 7, 6), device=False)
    assert same(got, dr.display(img, FILMIC, REFERENCE, dc.table(REFERENCE), False, 500, 0.5, 0.18, 0.0, 0x06070809)[0])
    got = display.tonemap(img, percentile=0.9, key=0.3, white=2.0, encode="gamma22", device=False)
    assert same(got, dr.display(img, REINHARD, GAMMA22, dc.table(GAMMA22), True, 900, 1.0, 0.3, 0.25, 0xff000000)[0])
    scale, hist = display.exposure_of(img, key=0.3, percentile=0.9, device=False)
    assert same(hist, dr.histogram(img)) and _bits(scale) == _bits(dr.pick(hist, 900, 0.3))

    class Image:
        rgb = img
    assert same(display.to_image(Image(), exposure=0.5, curve="clamp", device=False), display.tonemap(img, exposure=0.5, curve="clamp", device=False))
    with pytest.raises(ValueError, match=r"rgb must be \[h, w, 3\]"):
        display.tonemap(img[..., :2], device=False)
    with pytest.raises(_abi.DartRayHipError, match="exposure must be finite and positive"):
        display.tonemap(img, exposure=-1.0, device=False)


def test_the_bindings_keep_step_with_the_header(hip):
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    for name, value in (("DR_TONE_CLAMP", 0), ("DR_TONE_REINHARD", 1), ("DR_TONE_FILMIC", 2), ("DR_ENCODE_SRGB", 0), ("DR_ENCODE_GAMMA22", 1),
                        ("DR_ENCODE_REFERENCE", 2), ("DR_DISPLAY_BINS", 2048)):
        assert "#define %s %du" % (name, value) in header and getattr(_abi, name) == value
        assert ("%s = %d" % (name, value)) in dart
    assert "const int SIZEOF_DrDisplayParams = 32;" in dart and "lookupFunction<_DisplayC, _DisplayD>('dr_display')" in dart
    for i, (field, _) in enumerate(_abi.DrDisplayParams._fields_):
        assert "const int OFF_DrDisplayParams_%s = %d;" % (field, 4 * i) in dart
