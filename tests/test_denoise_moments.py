"""The variance-guided a-trous denoiser over a temporal history without a GPU: dr_denoise_moments_host against the numpy
restatement (tests/denoise_moments_restatement.py, written from the text) bit for bit on seeded histories; answers derived by hand for both
variance estimates; its tie to the pair rule's level (tests/denoise_pair_level_check.cpp, dnp_pixel built into a program of its own); what
becomes of pixels that are not valid; every refusal by code and text; and the Python module above it (dartray_amd/denoise.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, denoise

import denoise_moments_cases as mc
import denoise_moments_restatement as mr

F = np.float32
same = mr.same_bits


def _want(images, prm):
    it, kc, kn, kz, floor, mh, radius = prm
    return mr.denoise_moments(*images, it, kc, kn, kz, floor, mh, radius)


# ---- 1. host == restatement, bit for bit ----
@pytest.mark.parametrize("size", mc.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_bit_for_bit(hip, size):
    n = 0
    for key, images, prm in mc.grid([size]):
        want = _want(images, prm)
        got = mc.host(*images, prm)
        assert all(same(a, b) for a, b in zip(got, want)), key
        out, var, var0 = got
        assert np.array_equal(var0 < 0, var0 == -1) and np.array_equal(var < 0, var == -1) and not (var0 == -7).any()
        assert (var[var0 < 0] == -1).all() and np.isfinite(out[var >= 0]).all()
        n += 1
    assert n == len(mc.POISON) * len(mc.PARAMS)
    images, prm = mc.images(*size), mc.PARAMS[1]
    want = _want(images, prm)
    for variance, estimate in ((False, False), (True, False), (False, True)):     # the optional outputs change no byte of the others
        out, var, var0 = mc.host(*images, prm, variance=variance, estimate=estimate)
        assert same(out, want[0]) and (var is None) == (not variance) and (var0 is None) == (not estimate)
        assert (var is None or same(var, want[1])) and (var0 is None or same(var0, want[2]))


def test_the_cases_hold_what_they_promise():
    for mh in (2, 4, 4096):
        rgb, m2, length, normal, depth = mc.images(130, 7, min_history=mh)
        for row in length:                                               # every 64-pixel run of a row mixes all of them
            for x0 in (0, 66):
                run = row[x0:x0 + 64]
                assert (run == 0).any() and (run == 1).any() and (run == 4096).any()
                assert (run == np.nextafter(F(mh), F(0))).any() and (run == np.nextafter(F(mh), F(1e9))).any() and (run == mh).any()
        n = mr.pack(rgb, m2, length, normal, depth)
        bad = n < 0
        assert bad[0].any() and bad[-1].any() and bad[:, 0].any() and bad[:, -1].any() and bad[3, 3:-3].any()     # border and interior
        lum = mr.lum(rgb)
        with np.errstate(over="ignore"):
            assert ((m2 < lum * lum) & ~bad & (n >= mh)).any() and ((m2 < 0) & ~bad).any() and (np.isinf(lum * lum) & ~bad).any()
        v0 = mr.estimate(rgb, m2, n, normal, depth, mh, 3, 40.0, 0.3)
        assert ((v0 == 0) & (n >= mh)).any() and ((v0 > 0) & (n >= mh)).any() and ((v0 > 0) & (n < mh) & ~bad).any()
        assert ((v0 < 0) & ~bad).any() and (v0 > 1e30).any()             # an estimate that is not finite, and a huge one that is
    for poison in mc.POISON[1:]:
        clean, dirty = mc.images(67, 9), mc.images(67, 9, poison=poison)
        k = mc.POISON.index(poison) - 1
        assert (~np.isfinite(dirty[k])).sum() == 3 + (~np.isfinite(clean[k])).sum()
        assert np.isnan(dirty[k]).any() and (dirty[k] == np.inf).any() and (dirty[k] == -np.inf).any()
        assert (mr.pack(*dirty) < 0).sum() >= (mr.pack(*clean) < 0).sum() + 2
        assert not same(mc.host(*clean, mc.PARAMS[1])[0], mc.host(*dirty, mc.PARAMS[1])[0])


def test_every_parameter_matters(hip):
    """The cases above would agree trivially if a parameter were ignored on both sides."""
    images = mc.images(67, 9)
    base = (2, 0.0625, 40.0, 0.3, mc.VAR_FLOOR, 4, 3)
    variants = [base] + [base[:i] + (v,) + base[i + 1:] for i, v in ((0, 3), (1, 0.5), (2, 0.0), (3, 0.0), (4, 0.5), (5, 8), (6, 1), (6, 0))]
    outs = [mc.host(*images, prm) for prm in variants]
    for i in range(len(outs)):
        for j in range(i):
            assert not same(outs[i][0], outs[j][0]), (i, j)
    est = [o[2] for o in outs]
    assert same(est[0], est[1]) and same(est[0], est[2]) and same(est[0], est[5])                 # levels, k_color and floor: not the estimate's
    assert all(not same(est[0], est[i]) for i in (3, 4, 6, 7, 8))


# ---- 2. answers derived by hand ----
def _flat(w, h, rgb=(0.0, 0.0, 0.0), m2=0.75, length=4.0):
    return (np.broadcast_to(np.array(rgb, np.float32), (h, w, 3)).copy(), np.full((h, w), m2, np.float32), np.full((h, w), length, np.float32),
            np.full((h, w, 3), 0.25, np.float32), np.full((h, w), 3.0, np.float32))


def test_known_answers_for_the_temporal_estimate(hip):
    """Black rgb, m2 = 0.75, len = 4 = min_history: v = max(0, 0.75 - 0) / (4 - 1) = 0.25, all dyadic."""
    prm = (1, 0.0625, 40.0, 0.3, mc.VAR_FLOOR, 4, 3)
    out, var, var0 = mc.host(*_flat(9, 7), prm)
    assert (var0 == 0.25).all() and (out == 0).all()
    # grey 0.5: lum = 0.5 up to the three weights' rounding; m2 = 0.25 + 1.5 and len = 7 give 1.5 / 6 = 0.25 to a few ulp
    images = _flat(9, 7, rgb=(0.5, 0.5, 0.5), m2=1.75, length=7.0)
    var0 = mc.host(*images, prm)[2]
    assert (np.abs(var0.astype(np.float64) - 0.25) <= 4 * 2.0 ** -24).all()
    # m2 below lum^2 is clamped: exactly 0
    var0 = mc.host(*_flat(9, 7, rgb=(0.5, 0.5, 0.5), m2=0.125, length=7.0), prm)[2]
    assert (var0 == 0).all()
    # the longest history: len - 1 is the divisor
    var0 = mc.host(*_flat(9, 7, m2=0.75, length=4096.0), prm)[2]
    assert (var0 == F(0.75) / F(4095)).all()


def test_known_answers_for_the_spatial_estimate(hip):
    """len = 3 < min_history goes to the window: 0 over an all-black one whatever m2 says; and over a window of two exact luminances the
    plain variance of its valid pixels -- green 0 and 1 / 0.715160 make lum 0 and (the f32 nearest) 1, every guide term off."""
    prm = (1, 0.0625, 0.0, 0.0, mc.VAR_FLOOR, 4, 3)
    out, var, var0 = mc.host(*_flat(9, 7, length=3.0), prm)
    assert (var0 == 0).all() and (var == 0).all() and (out == 0).all()
    rgb, m2, length, normal, depth = _flat(7, 7, length=1.0)
    g = F(1.0) / F(0.715160)
    lum1 = F(0.715160) * g
    rgb[:, :3, 1] = g                                                    # 21 of the 49 pixels
    length[3, 0] = 0.0                                                   # ... of which one is not valid: 20 of 48
    var0 = mc.host(rgb, m2, length, normal, depth, prm)[2]
    mean = 20.0 * float(lum1) / 48.0
    want = 20.0 * float(lum1) ** 2 / 48.0 - mean * mean
    assert abs(float(var0[3, 3]) - want) <= 64 * 2.0 ** -24 and var0[3, 0] == -1
    # radius 0: the centre alone, whose variance is 0 exactly
    var0 = mc.host(rgb, m2, length, normal, depth, prm[:6] + (0,))[2]
    assert (var0[length > 0] == 0).all()
    # a neighbour across a depth step counts for 1 / (1 + k_depth * dz): with dz = 1 and k = 1, a half
    rgb, m2, length, normal, depth = _flat(2, 1, length=1.0)
    rgb[0, 1, 1], depth[0, 1] = g, 4.0
    var0 = mc.host(rgb, m2, length, normal, depth, (1, 0.0, 0.0, 1.0, mc.VAR_FLOOR, 4, 1))[2]
    l = float(lum1)
    want = (0.5 * l * l) / 1.5 - ((0.5 * l) / 1.5) ** 2
    assert np.abs(var0.astype(np.float64) - want).max() <= 8 * 2.0 ** -24


def test_a_pixel_without_history_comes_out_bit_for_bit(hip):
    rgb, m2, length, normal, depth = mc.images(67, 9)
    rgb.view(np.uint32)[4, 30] = [0x3fa00000, 0x7fc01234, 0xc0000000]       # 1.25, a NaN with a payload, -2
    length[4, 30] = 0.0
    length[4, 31] = 0.0
    for prm in (mc.PARAMS[0], mc.PARAMS[2]):
        out, var, var0 = mc.host(rgb, m2, length, normal, depth, prm)
        for x in (30, 31):
            assert same(out[4, x], rgb[4, x]) and var[4, x] == -1 and var0[4, x] == -1
    bad = mr.pack(rgb, m2, length, normal, depth) < 0
    assert bad.sum() > 40
    out, var, var0 = mc.host(rgb, m2, length, normal, depth, mc.PARAMS[2])
    assert same(out[bad], rgb[bad]) and (var[bad] == -1).all() and (var0[bad] == -1).all()
    # ... and is no tap of any other pixel: new finite colours and moments under the same validity change nothing else
    rng = np.random.Generator(np.random.PCG64(5))
    rgb2, m22 = rgb.copy(), m2.copy()
    sel = bad[..., None] & np.isfinite(rgb2) & (np.abs(rgb2) < 1e10)
    rgb2[sel] = (10.0 * rng.random(int(sel.sum()))).astype(np.float32)
    m22[bad & np.isfinite(m22)] = 5.0
    assert np.array_equal(mr.pack(rgb2, m22, length, normal, depth) < 0, bad) and not same(rgb2[bad], rgb[bad])
    out2, var2, var02 = mc.host(rgb2, m22, length, normal, depth, mc.PARAMS[2])
    assert same(out2[~bad], out[~bad]) and same(var2, var) and same(var02, var0) and same(out2[bad], rgb2[bad])


# ---- 3. the tie to the pair rule ----
def _run_level(exe, tmp_path, colour, v, normal, depth, s, kc, kn, kz, var_floor):
    h, w = v.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([w, h, s], np.int32).tobytes() + np.array([kc, kn, kz, var_floor], np.float32).tobytes())
        f.write(np.concatenate([colour, v[..., None]], axis=2).astype(np.float32).tobytes())
        f.write(np.concatenate([normal, depth[..., None]], axis=2).astype(np.float32).tobytes())
    res = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "denoise_pair_level_check: OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    out = np.fromfile(dst, np.float32).reshape(h, w, 4)
    return np.ascontiguousarray(out[..., :3]), np.ascontiguousarray(out[..., 3])


def test_one_level_is_the_pair_rules_level_on_the_estimate(hip, tmp_path):
    """iterations = 1: `out` and `out_var` are one level of dnp_pixel, built into a program of its own, on the planes (rgb, out_var0) and
    dn_pack_guide -- the levels are dnp_pixel and nothing else."""
    exe = str(tmp_path / "denoise_pair_level_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "denoise_pair_level_check.cpp"), "-o", exe])
    for size, poison in (((67, 9), None), ((3, 5), "len"), ((65, 5), "normal")):
        rgb, m2, length, normal, depth = mc.images(*size, poison=poison)
        for prm in (mc.PARAMS[0], mc.PARAMS[5], mc.PARAMS[7]):
            out, var, var0 = mc.host(rgb, m2, length, normal, depth, prm)
            got = _run_level(exe, tmp_path, rgb, var0, normal, depth, 1, *prm[1:5])
            assert same(got[0], out) and same(got[1], var), (size, poison, prm)


# ---- 4. the refusals, by code and text ----
def test_every_refusal_by_code_and_text(hip):
    lib = hip.lib()
    rgb, m2, length, normal, depth = (np.ascontiguousarray(x[:2, :3]) for x in mc.images(67, 9))
    out, var, var0 = np.zeros_like(rgb), np.zeros_like(depth), np.zeros_like(depth)
    ok = mc.params(2, 1.0, 1.0, 1.0)

    def refused(needle, rgb=rgb.ctypes.data, m2=m2.ctypes.data, length=length.ctypes.data, normal=normal.ctypes.data, depth=depth.ctypes.data,
                w=3, h=2, p=ok, out=out.ctypes.data, var=var.ctypes.data, var0=var0.ctypes.data):
        for fn in (lib.dr_denoise_moments_host, lib.dr_denoise_moments):     # the same checks, ahead of any device call
            rc = fn(rgb, m2, length, normal, depth, w, h, C.byref(p) if p is not None else None, out, var, var0)
            assert rc == -1, (needle, rc)
            assert needle in lib.dr_last_error().decode(), (needle, lib.dr_last_error())

    def check_refused(needle, p, w=3, h=2):
        assert lib.dr_denoise_moments_check(C.byref(p) if p is not None else None, w, h) == -1
        assert needle in lib.dr_last_error().decode() and "dr_denoise_moments_check: " in lib.dr_last_error().decode()

    for name in ("rgb", "m2", "length", "normal", "depth", "p", "out"):
        refused("a null pointer", **{name: None})
    check_refused("a null pointer", None)
    for kw in (dict(w=0), dict(h=-2)):
        refused("w and h must be at least 1", **kw)
        check_refused("w and h must be at least 1", ok, **kw)
    for kw in (dict(w=65536, h=32768), dict(w=2 ** 31 - 1, h=2)):
        refused("the image has 2^31 or more pixels", **kw)
        check_refused("the image has 2^31 or more pixels", ok, **kw)

    def both(needle, p):
        refused(needle, p=p)
        check_refused(needle, p)

    for it in (0, 9, -1):
        both("iterations must be in 1..8", mc.params(it, 1.0, 1.0, 1.0))
    for bad in (-1.0, float("inf"), float("nan"), -0.5):
        for which in range(3):
            k = [1.0, 1.0, 1.0]
            k[which] = bad
            both("must be finite and not negative", mc.params(2, *k))
    for bad in (0.0, -0.0, -1e-4, float("inf"), float("nan")):
        both("var_floor must be finite and positive", mc.params(2, 1.0, 1.0, 1.0, var_floor=bad))
    for bad in (1, 0, -4, 4097):
        both("min_history must be in 2..4096", mc.params(2, 1.0, 1.0, 1.0, min_history=bad))
    for bad in (-1, 4, 49):
        both("radius must be in 0..3", mc.params(2, 1.0, 1.0, 1.0, radius=bad))
    for good in (mc.params(8, 3.0e38, 0.0, 1.0, 1e-45, 2, 0), mc.params(1, 0.0, 1.0, 0.0, 3e38, 4096, 3)):
        assert lib.dr_denoise_moments_check(C.byref(good), 3, 2) == 0
        _abi.check(lib.dr_denoise_moments_host(rgb.ctypes.data, m2.ctypes.data, length.ctypes.data, normal.ctypes.data, depth.ctypes.data, 3, 2,
                                               C.byref(good), out.ctypes.data, var.ctypes.data, var0.ctypes.data))
    refused("out overlaps an input", out=rgb.ctypes.data)
    refused("out overlaps an input", out=m2.ctypes.data + 4 * 5)          # its first float is m2's last
    refused("out overlaps an input", out=length.ctypes.data)
    refused("out overlaps an input", out=normal.ctypes.data + 4 * 17)
    refused("out overlaps an input", depth=out.ctypes.data + 4 * 17)
    refused("out_var overlaps an input", var=rgb.ctypes.data + 4 * 12)
    refused("out_var overlaps an input", var=m2.ctypes.data)
    refused("out_var overlaps an input", var=length.ctypes.data + 4 * 5)
    refused("out_var overlaps an input", var=normal.ctypes.data)
    refused("out_var overlaps an input", var=depth.ctypes.data)
    refused("out_var0 overlaps an input", var0=rgb.ctypes.data)
    refused("out_var0 overlaps an input", var0=m2.ctypes.data + 4 * 5)
    refused("out_var0 overlaps an input", var0=length.ctypes.data)
    refused("out_var0 overlaps an input", var0=normal.ctypes.data + 4 * 17)
    refused("out_var0 overlaps an input", var0=depth.ctypes.data)
    refused("out overlaps out_var", var=out.ctypes.data + 4 * 17)
    refused("out overlaps out_var0", var0=out.ctypes.data)
    refused("out_var overlaps out_var0", var0=var.ctypes.data + 4 * 5)
    # inputs are only read and may share a buffer; the optional outputs may be NULL
    _abi.check(lib.dr_denoise_moments_host(rgb.ctypes.data, m2.ctypes.data, m2.ctypes.data, rgb.ctypes.data, m2.ctypes.data, 3, 2, C.byref(ok),
                                           out.ctypes.data, None, None))
    # the device entry: the same checks and its own, all ahead of any device call; the size query needs no device
    n = C.c_uint64(0)
    dev = lib.dr_denoise_moments_device
    none5 = (None,) * 5
    assert dev(*none5, 129, 65, C.byref(ok), None, None, None, None, C.byref(n), None) == 0
    assert n.value == 48 * 129 * 65
    pair = C.c_uint64(0)
    assert lib.dr_denoise_pair_device(None, None, None, None, 129, 65, C.byref(_abi.DrDenoisePairParams(2, 1.0, 1.0, 1.0, 1e-4)), None, None, None,
                                      C.byref(pair), None) == 0 and pair.value == n.value
    assert dev(*none5, 129, 65, C.byref(ok), None, None, None, None, None, None) == -1
    assert "a null pointer" in lib.dr_last_error().decode()
    assert dev(*none5, 0, 65, C.byref(ok), None, None, None, None, C.byref(n), None) == -1
    assert "w and h must be at least 1" in lib.dr_last_error().decode()
    assert dev(*none5, 3, 2, C.byref(mc.params(2, 1.0, 1.0, 1.0, radius=4)), None, None, None, None, C.byref(n), None) == -1
    assert "radius must be in 0..3" in lib.dr_last_error().decode()
    assert dev(*none5, 3, 2, C.byref(mc.params(2, 1.0, 1.0, 1.0, min_history=1)), None, None, None, None, C.byref(n), None) == -1
    assert "min_history must be in 2..4096" in lib.dr_last_error().decode()
    fake = 1 << 20                                                       # addresses that are only compared, never read
    args = (fake, 2 * fake, 3 * fake, 4 * fake, 5 * fake, 3, 2, C.byref(ok))
    o, v, v0, sc = 6 * fake, 7 * fake, 8 * fake, 9 * fake
    n = C.c_uint64(48 * 6 - 1)
    assert dev(*args, o, v, v0, sc, C.byref(n), None) == -1
    assert "the scratch buffer is too small" in lib.dr_last_error().decode()
    n = C.c_uint64(48 * 6)
    assert dev(*args, o, v, v0, sc + 4, C.byref(n), None) == -1
    assert "not 16-byte aligned" in lib.dr_last_error().decode()
    assert dev(*args, sc + 16, v, v0, sc, C.byref(n), None) == -1
    assert "out overlaps the scratch buffer" in lib.dr_last_error().decode()
    assert dev(*args, o, sc + 48 * 6 - 4, v0, sc, C.byref(n), None) == -1
    assert "out_var overlaps the scratch buffer" in lib.dr_last_error().decode()
    assert dev(*args, o, v, sc - 20, sc, C.byref(n), None) == -1
    assert "out_var0 overlaps the scratch buffer" in lib.dr_last_error().decode()
    assert dev(*args, 2 * fake + 8, v, v0, sc, C.byref(n), None) == -1
    assert "out overlaps an input" in lib.dr_last_error().decode()
    assert dev(*args, o, 5 * fake + 20, v0, sc, C.byref(n), None) == -1
    assert "out_var overlaps an input" in lib.dr_last_error().decode()
    assert dev(*args, o, v, 3 * fake, sc, C.byref(n), None) == -1
    assert "out_var0 overlaps an input" in lib.dr_last_error().decode()
    assert dev(*args, o, o + 68, v0, sc, C.byref(n), None) == -1
    assert "out overlaps out_var" in lib.dr_last_error().decode()
    assert dev(*args, o, v, v + 20, sc, C.byref(n), None) == -1
    assert "out_var overlaps out_var0" in lib.dr_last_error().decode()
    assert dev(*args[:7], None, o, v, v0, sc, C.byref(n), None) == -1
    assert "a null pointer" in lib.dr_last_error().decode()


# ---- 5. the Python module ----
def test_the_defaults_are_the_documented_ones():
    p = denoise.moments_params()
    assert (p.iterations, p.k_color, p.k_normal, p.k_depth, p.var_floor, p.min_history, p.radius) == \
        (5, 0.0625, float(F(1.0 / (0.1 * 0.1))), 1.0, float(F(1e-4)), 4, 3)
    assert C.sizeof(_abi.DrDenoiseMomentsParams) == 28
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "iterations = 5, sigma_color = 4.0, sigma_normal = 0.1, sigma_depth = 1.0, var_floor = 1e-4, min_history = 4, radius = 3" in design
    assert "### 2.24" in design


def test_the_module_on_the_host_equals_the_restatement(hip):
    images = mc.images(67, 9)
    frame = denoise.TemporalFrame(*images)
    p = denoise.moments_params()
    want = mr.denoise_moments(*images, p.iterations, p.k_color, p.k_normal, p.k_depth, p.var_floor, p.min_history, p.radius)
    got = denoise.atrous_moments(frame, device=False)
    assert isinstance(got, np.ndarray) and same(got, want[0])
    got = denoise.atrous_moments(frame, device=False, return_variance=True)
    assert len(got) == 2 and same(got[0], want[0]) and same(got[1], want[1])
    got = denoise.atrous_moments(frame, device=False, return_estimate=True)
    assert len(got) == 2 and same(got[0], want[0]) and same(got[1], want[2])
    got = denoise.atrous_moments(frame, device=False, return_variance=True, return_estimate=True)
    assert len(got) == 3 and all(same(a, b) for a, b in zip(got, want))

    class Bag:
        pass
    bag = Bag()
    bag.rgb, bag.m2, bag.len, bag.normal, bag.depth = (a.astype(np.float64) for a in images)      # anything with the five; converted to f32
    got = denoise.atrous_moments(bag, iterations=2, sigma_color=float("inf"), sigma_normal=0.5, sigma_depth=float("inf"), var_floor=0.25,
                                 min_history=8, radius=1, device=False)
    assert same(got, mr.denoise_moments(*images, 2, 0.0, 4.0, 0.0, 0.25, 8, 1)[0])
    del bag.m2
    with pytest.raises(ValueError, match="frame has no m2"):
        denoise.atrous_moments(bag, device=False)
    with pytest.raises(ValueError, match=r"m2 and len must be \[h, w\]"):
        denoise.atrous_moments(denoise.TemporalFrame(images[0], images[1][:5], *images[2:]), device=False)
    with pytest.raises(_abi.DartRayHipError, match="min_history must be in 2..4096"):
        denoise.atrous_moments(frame, min_history=1, device=False)
    with pytest.raises(_abi.DartRayHipError, match="radius must be in 0..3"):
        denoise.atrous_moments(frame, radius=4, device=False)


def test_render_sequence_refuses_by_name():
    with pytest.raises(ValueError, match="render_sequence: denoise must be False, True or \"moments\", got 'nonsense'"):
        denoise.render_sequence([], None, denoise="nonsense")
    with pytest.raises(ValueError, match="render_sequence: denoise must be False, True or \"moments\", got 2"):
        denoise.render_sequence([], None, denoise=2)
    with pytest.raises(ValueError, match="render_sequence: min_history given without denoise=True"):
        denoise.render_sequence([], None, min_history=4)
    with pytest.raises(ValueError, match="render_sequence: iterations, radius given without denoise=True"):
        denoise.render_sequence([], None, denoise=False, radius=1, iterations=2)
    assert denoise.render_sequence([], None, denoise="moments", radius=1) == []
