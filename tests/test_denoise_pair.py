"""The variance-guided a-trous denoiser over two half renders without a GPU: dr_denoise_pair_host against the numpy restatement
(tests/denoise_pair_restatement.py, written from the text) bit for bit on seeded pairs; its tie to the plain filter of 2.15; the symmetry in
the two halves; answers derived by hand for the variance it carries and for the estimator; what becomes of pixels that are not valid; every
refusal by code and text; and the Python module above it (dartray_amd/denoise.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, denoise, scenes

import denoise_cases as dc
import denoise_pair_cases as pc
import denoise_pair_restatement as pr

F = np.float32
same = pr.same_bits
LUM = np.array([0.212671, 0.715160, 0.072169])


def _both(a, b, normal, depth, iterations, kc, kn, kz, var_floor=pc.VAR_FLOOR):
    """The restatement's and the host entry's (colour, variance), which must agree before either is compared with a derived answer."""
    want = pr.denoise_pair(a, b, normal, depth, iterations, kc, kn, kz, var_floor)
    got = pc.host(a, b, normal, depth, iterations, kc, kn, kz, var_floor)
    assert same(got[0], want[0]) and same(got[1], want[1])
    return want


def _finite_guides(normal, depth):
    return np.isfinite(normal).all(axis=2) & np.isfinite(depth)


# ---- 1. host == restatement, bit for bit ----
@pytest.mark.parametrize("iterations", pc.ITERATIONS)
@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_bit_for_bit(hip, size, iterations):
    a, b, normal, depth = pc.images(*size)
    m, v0 = pr.pack(a, b, normal, depth)
    if size[0] * size[1] >= 64:
        assert 0 < (v0 < 0).sum() < v0.size // 3 and (a == b).all(axis=2).sum() > 4
    for k in pc.K_COMBOS:
        out, var = _both(a, b, normal, depth, iterations, *k)
        assert np.isfinite(out[var >= 0]).all() and np.isfinite(var).all() and ((var >= 0) | (var == -1)).all()
        colours_only, none = pc.host(a, b, normal, depth, iterations, *k, variance=False)     # out_var == NULL: the same colours
        assert none is None and same(colours_only, out)


def test_the_cases_hold_what_they_promise():
    a, b, normal, depth = pc.images(64, 64)
    m, v = pr.pack(a, b, normal, depth)
    fin_a, fin_b, guides = np.isfinite(a).all(axis=2), np.isfinite(b).all(axis=2), _finite_guides(normal, depth)
    assert (~fin_a & fin_b).any() and (fin_a & ~fin_b).any() and (~fin_a & ~fin_b).any()          # non-finite in a only, b only, both
    huge_a, huge_b = np.abs(np.where(fin_a[..., None], a, 0)).max(axis=2) > 1e18, np.abs(np.where(fin_b[..., None], b, 0)).max(axis=2) > 1e18
    assert (huge_a & ~huge_b).any() and (~huge_a & huge_b).any() and (huge_a & huge_b).any()
    assert (a[huge_a] < -1e18).any() and (a[huge_a] > 1e18).any() and (b[huge_b] < -1e18).any() and (b[huge_b] > 1e18).any()
    assert (fin_a & fin_b & guides & np.isinf(m).any(axis=2)).any()                                # a mean that overflows
    assert (np.isfinite(m).all(axis=2) & guides & (v < 0)).any()                                   # v0 alone overflows
    assert (v > 1e30).any()                                                                        # ... and a huge one that does not
    with np.errstate(invalid="ignore"):
        noise = np.abs(a - b)[..., 1]
    ok = np.isfinite(noise) & (noise < 10)
    assert np.median(noise[:, :8][ok[:, :8]]) * 5 < np.median(noise[:, -8:][ok[:, -8:] & (noise[:, -8:] > 0)])   # the noise level varies


def test_the_term_switches_levels_and_floor_matter(hip):
    """The cases above would agree trivially if k, the level count or the floor were ignored on both sides."""
    a, b, normal, depth = pc.images(17, 33)
    outs = [pc.host(a, b, normal, depth, 2, *k) for k in pc.K_COMBOS] + [pc.host(a, b, normal, depth, 3, *pc.K_COMBOS[-1]),
                                                                          pc.host(a, b, normal, depth, 2, *pc.K_COMBOS[-1], var_floor=0.5)]
    for i in range(len(outs)):
        for j in range(i):
            assert not same(outs[i][0], outs[j][0]), (i, j)


# ---- 2. the tie to the filter of 2.15 ----
@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("size", [(17, 33), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_without_the_colour_term_the_colours_are_the_plain_filters(hip, size, iterations):
    a, b, normal, depth = pc.images(*size, variance_only=False)
    guides = _finite_guides(normal, depth)
    for kn, kz in [(0.0, 0.0), (40.0, 0.0), (0.0, 0.3), (40.0, 0.3)]:
        levels = pr.planes(a, b, normal, depth, iterations, 0.0, kn, kz, pc.VAR_FLOOR)
        for m, v in levels:                                             # no pixel loses validity through its variance alone
            assert np.array_equal(v < 0, ~(np.isfinite(m).all(axis=2) & guides))
        assert (levels[0][1] < 0).any()
        out, _ = pc.host(a, b, normal, depth, iterations, 0.0, kn, kz)
        assert same(out, levels[-1][0])
        assert same(out, dc.host(levels[0][0], normal, depth, iterations, 0.0, kn, kz))


# ---- 3. symmetry ----
@pytest.mark.parametrize("size", [(7, 1), (17, 33), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_swapping_the_halves_changes_no_byte(hip, size):
    a, b, normal, depth = pc.images(*size)
    for k in (pc.K_COMBOS[0], pc.K_COMBOS[4], pc.K_COMBOS[-1]):
        ab, ba = pc.host(a, b, normal, depth, 5, *k), pc.host(b, a, normal, depth, 5, *k)
        assert same(ab[0], ba[0]) and same(ab[1], ba[1])


# ---- 4. answers derived by hand ----
def test_known_answer_for_the_propagated_variance(hip):
    """a = c + e, b = c - e, exact in f32: m = c and v0 = lum(e)^2 at every pixel.  One level with every k = 0 leaves an interior pixel (all 25
    taps inside) with sumw = 1 and sumv = v0 * sum of H^2 = v0 * (70 / 256)^2 -- h's sum of squares is 70 / 256.  The bound is a handful of f32
    roundings over 25 taps."""
    w, h = 17, 33
    c, e = np.array([0.5, 0.25, 0.75], np.float32), np.array([0.125, 0.0625, 0.03125], np.float32)
    a, b = np.broadcast_to(c + e, (h, w, 3)).copy(), np.broadcast_to(c - e, (h, w, 3)).copy()
    assert ((a + b) * F(0.5) == c).all() and ((a - b) == 2 * e).all()
    normal, depth = np.full((h, w, 3), 0.25, np.float32), np.full((h, w), 3.0, np.float32)
    out, var = _both(a, b, normal, depth, 1, 0.0, 0.0, 0.0)
    want = float(LUM @ e.astype(np.float64)) ** 2 * (70.0 / 256.0) ** 2
    inner = var[2:-2, 2:-2].astype(np.float64)
    assert inner.size == 13 * 29 and (np.abs(inner - want) <= 1e-5 * want).all()
    assert (np.abs(out.astype(np.float64) - c) <= 1e-5 * c).all()
    assert (var[0].astype(np.float64) > want * 1.2).all()              # a border pixel renormalises over fewer taps: less averaging


def test_known_answer_for_the_estimator():
    """A constant image plus independent Gaussian noise of standard deviation sigma per channel in each half: lum(a - b) has variance
    2 sigma^2 * sum of the squared luminance weights, so v0 = lum(a - b)^2 / 4 has the mean 0.5 sigma^2 * that sum.  v0 is a scaled
    chi-square with one degree of freedom: over 4096 pixels its mean deviates by sqrt(2 / 4096) relative, and five of those are allowed."""
    rng = np.random.Generator(np.random.PCG64(2017))
    sigma = 0.3
    a = (1.0 + sigma * rng.normal(size=(64, 64, 3))).astype(np.float32)
    b = (1.0 + sigma * rng.normal(size=(64, 64, 3))).astype(np.float32)
    m, v0 = pr.pack(a, b, np.zeros((64, 64, 3), np.float32), np.ones((64, 64), np.float32))
    want = 0.5 * sigma ** 2 * float((LUM ** 2).sum())
    got = float(v0.astype(np.float64).mean())
    assert (v0 >= 0).all() and abs(got - want) <= 5.0 * np.sqrt(2.0 / 4096.0) * want, (got, want)
    assert np.abs(m.astype(np.float64).mean() - 1.0) < 5 * sigma / np.sqrt(2 * 3 * 4096)


# ---- 5. pixels that are not valid ----
@pytest.mark.parametrize("size", [(17, 33), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_invalid_pixels_pass_through_as_the_mean_and_are_no_tap(hip, size):
    a, b, normal, depth = pc.images(*size)
    m, v0 = pr.pack(a, b, normal, depth)
    bad = v0 < 0
    assert bad.sum() > 8
    nan = np.isnan(m)
    assert nan.any() and (m.view(np.uint32)[nan] == 0x7fc00000).all()  # a NaN mean is the one quiet NaN, whatever NaN went in
    rng = np.random.Generator(np.random.PCG64(5))
    a2, b2, normal2, depth2 = a.copy(), b.copy(), normal.copy(), depth.copy()
    for img in (a2, b2, normal2):                                       # new values in the finite channels of moderate size: the huge ones are
        sel = bad[..., None] & np.isfinite(img) & (np.abs(img) < 1e10)  # what makes some of these pixels invalid
        img[sel] = (10.0 * rng.random(int(sel.sum()))).astype(np.float32)
    sel = bad & np.isfinite(depth2)
    depth2[sel] = (40.0 * rng.random(int(sel.sum()))).astype(np.float32)
    m2, v2 = pr.pack(a2, b2, normal2, depth2)
    assert np.array_equal(v2 < 0, bad) and not same(m2[bad], m[bad])
    for k in (pc.K_COMBOS[0], pc.K_COMBOS[-1]):
        out, var = _both(a, b, normal, depth, 5, *k)
        assert same(out[bad], m[bad]) and (var[bad] == -1).all() and (var[~bad] >= 0).all()
        out2, var2 = pc.host(a2, b2, normal2, depth2, 5, *k)
        assert same(out2[~bad], out[~bad]) and same(var2, var) and same(out2[bad], m2[bad])


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


def test_a_pixel_that_loses_validity_at_a_level_keeps_that_levels_colour(tmp_path):
    """No plane that the pack writes lets a level do this (a mean is at most FLT_MAX / 2 and v0 at most FLT_MAX / 4, and a
    level's colour and variance are bounded by the largest among its taps), so the rule -- dnp_pixel itself, built into a program of its
    own -- is handed a plane with an infinite variance.  Every pixel that has that one as a tap gets an infinite variance out: it comes out
    as (its filtered colour, -1), and the next level passes it through bit for bit."""
    exe = str(tmp_path / "denoise_pair_level_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "denoise_pair_level_check.cpp"), "-o", exe])
    w, h = 9, 7
    rng = np.random.Generator(np.random.PCG64(3))
    colour = rng.random((h, w, 3)).astype(np.float32)
    v = (0.01 * rng.random((h, w))).astype(np.float32)
    normal, depth = rng.random((h, w, 3)).astype(np.float32), (3.0 + rng.random((h, w))).astype(np.float32)
    v[1, 1] = np.inf
    v[6, 8] = -1.0
    k = (0.0625, 2.0, 0.3, 1e-4)
    want1 = pr.one_level(colour, v, normal, depth, 1, *k)
    got1 = _run_level(exe, tmp_path, colour, v, normal, depth, 1, *k)
    assert same(got1[0], want1[0]) and same(got1[1], want1[1])
    lost = (v >= 0) & (got1[1] < 0)
    near = np.zeros((h, w), bool)
    near[:4, :4] = True                                                 # the pixels that have (1, 1) as a tap at step 1
    assert np.array_equal(lost, near) and (got1[1][lost] == -1).all()
    assert np.isfinite(got1[0][lost]).all() and (got1[0][lost] != colour[lost]).any(axis=1).all()     # this level's colour, not its input's
    assert same(got1[0][6, 8], colour[6, 8])
    want2 = pr.one_level(*want1, normal, depth, 2, *k)
    got2 = _run_level(exe, tmp_path, *got1, normal, depth, 2, *k)
    assert same(got2[0], want2[0]) and same(got2[1], want2[1])
    assert same(got2[0][lost], got1[0][lost]) and (got2[1][lost] == -1).all() and (got2[1][~lost & (v >= 0)] >= 0).all()


# ---- 6. the refusals, by code and text ----
def test_every_refusal_by_code_and_text(hip):
    lib = hip.lib()
    a, b, normal, depth = (np.ascontiguousarray(x[:2, :3]) for x in pc.images(17, 33))
    out, var = np.zeros_like(a), np.zeros_like(depth)
    ok = pc.params(2, 1.0, 1.0, 1.0)

    def refused(needle, a=a.ctypes.data, b=b.ctypes.data, normal=normal.ctypes.data, depth=depth.ctypes.data, w=3, h=2, p=ok,
                out=out.ctypes.data, var=var.ctypes.data):
        for fn in (lib.dr_denoise_pair_host, lib.dr_denoise_pair):     # the same checks, ahead of any device call
            rc = fn(a, b, normal, depth, w, h, C.byref(p) if p is not None else None, out, var)
            assert rc == -1, (needle, rc)
            assert needle in lib.dr_last_error().decode(), (needle, lib.dr_last_error())

    for name in ("a", "b", "normal", "depth", "p", "out"):
        refused("a null pointer", **{name: None})
    refused("w and h must be at least 1", w=0)
    refused("w and h must be at least 1", h=-2)
    refused("the image has 2^31 or more pixels", w=65536, h=32768)
    refused("the image has 2^31 or more pixels", w=2 ** 31 - 1, h=2)
    for it in (0, 9, -1):
        refused("iterations must be in 1..8", p=pc.params(it, 1.0, 1.0, 1.0))
    for bad in (-1.0, float("inf"), float("nan"), -0.5):
        for which in range(3):
            k = [1.0, 1.0, 1.0]
            k[which] = bad
            refused("must be finite and not negative", p=pc.params(2, *k))
    for bad in (0.0, -0.0, -1e-4, float("inf"), float("nan")):
        refused("var_floor must be finite and positive", p=pc.params(2, 1.0, 1.0, 1.0, var_floor=bad))
    _abi.check(lib.dr_denoise_pair_host(a.ctypes.data, b.ctypes.data, normal.ctypes.data, depth.ctypes.data, 3, 2,
                                        C.byref(pc.params(8, 3.0e38, 1.0, 1.0, var_floor=1e-45)), out.ctypes.data, var.ctypes.data))
    refused("out overlaps an input", out=a.ctypes.data)
    refused("out overlaps an input", out=b.ctypes.data + 4 * 17)       # its first float is b's last
    refused("out overlaps an input", out=normal.ctypes.data)
    refused("out overlaps an input", depth=out.ctypes.data + 4 * 17)
    refused("out_var overlaps an input", var=a.ctypes.data + 4 * 12)
    refused("out_var overlaps an input", var=b.ctypes.data)
    refused("out_var overlaps an input", var=normal.ctypes.data)
    refused("out_var overlaps an input", var=depth.ctypes.data + 4 * 5)
    refused("out overlaps out_var", var=out.ctypes.data + 4 * 17)
    # the two halves may be one buffer: inputs are only read
    _abi.check(lib.dr_denoise_pair_host(a.ctypes.data, a.ctypes.data, normal.ctypes.data, depth.ctypes.data, 3, 2, C.byref(ok), out.ctypes.data, None))
    # the device entry: the same checks and its own, all ahead of any device call; the size query needs no device
    n = C.c_uint64(0)
    dev = lib.dr_denoise_pair_device
    assert dev(None, None, None, None, 129, 65, C.byref(ok), None, None, None, C.byref(n), None) == 0
    assert n.value == 48 * 129 * 65
    assert dev(None, None, None, None, 129, 65, C.byref(ok), None, None, None, None, None) == -1
    assert "a null pointer" in lib.dr_last_error().decode()
    assert dev(None, None, None, None, 0, 65, C.byref(ok), None, None, None, C.byref(n), None) == -1
    assert "w and h must be at least 1" in lib.dr_last_error().decode()
    assert dev(None, None, None, None, 3, 2, C.byref(pc.params(2, 1.0, 1.0, 1.0, var_floor=0.0)), None, None, None, C.byref(n), None) == -1
    assert "var_floor must be finite and positive" in lib.dr_last_error().decode()
    fake = 1 << 20                                                       # addresses that are only compared, never read
    args = (fake, 2 * fake, 3 * fake, 4 * fake, 3, 2, C.byref(ok))
    n = C.c_uint64(48 * 6 - 1)
    assert dev(*args, 5 * fake, 6 * fake, 7 * fake, C.byref(n), None) == -1
    assert "the scratch buffer is too small" in lib.dr_last_error().decode()
    n = C.c_uint64(48 * 6)
    assert dev(*args, 5 * fake, 6 * fake, 7 * fake + 4, C.byref(n), None) == -1
    assert "not 16-byte aligned" in lib.dr_last_error().decode()
    assert dev(*args, 7 * fake + 16, 6 * fake, 7 * fake, C.byref(n), None) == -1
    assert "out overlaps the scratch buffer" in lib.dr_last_error().decode()
    assert dev(*args, 5 * fake, 7 * fake + 48 * 6 - 4, 7 * fake, C.byref(n), None) == -1
    assert "out_var overlaps the scratch buffer" in lib.dr_last_error().decode()
    assert dev(*args, 2 * fake + 8, 6 * fake, 7 * fake, C.byref(n), None) == -1
    assert "out overlaps an input" in lib.dr_last_error().decode()
    assert dev(*args, 5 * fake, 4 * fake + 20, 7 * fake, C.byref(n), None) == -1
    assert "out_var overlaps an input" in lib.dr_last_error().decode()
    assert dev(*args, 5 * fake, 5 * fake + 68, 7 * fake, C.byref(n), None) == -1
    assert "out overlaps out_var" in lib.dr_last_error().decode()


# ---- 7. the Python module ----
def test_the_defaults_are_the_documented_ones():
    p = denoise.pair_params()
    assert (p.iterations, p.k_color, p.k_normal, p.k_depth, p.var_floor) == (5, 0.0625, float(F(1.0 / (0.1 * 0.1))), 1.0, float(F(1e-4)))
    assert C.sizeof(_abi.DrDenoisePairParams) == 20
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "iterations = 5, sigma_color = 4.0, sigma_normal = 0.1, sigma_depth = 1.0, var_floor = 1e-4" in design
    assert denoise.pair_seed(5489) == 5489 ^ 0x2545F491 and all(denoise.pair_seed(s) != s for s in (0, 1, -1, 5489, 2 ** 62))
    assert "0x2545F491" in design


def test_the_module_on_the_host_equals_the_restatement(hip):
    a, b, normal, depth = pc.images(17, 33)
    p = denoise.pair_params()
    want = pr.denoise_pair(a, b, normal, depth, p.iterations, p.k_color, p.k_normal, p.k_depth, p.var_floor)
    got = denoise.atrous_pair(a, b, normal, depth, device=False)
    assert isinstance(got, np.ndarray) and same(got, want[0])
    got = denoise.atrous_pair(a, b, normal, depth, device=False, return_variance=True)
    assert same(got[0], want[0]) and same(got[1], want[1])
    got = denoise.atrous_pair(a, b, normal, depth, iterations=2, sigma_color=float("inf"), sigma_normal=0.5, sigma_depth=float("inf"),
                              var_floor=0.25, device=False)
    assert same(got, pr.denoise_pair(a, b, normal, depth, 2, 0.0, 4.0, 0.0, 0.25)[0])
    with pytest.raises(ValueError, match=r"a, b and normal must be \[h, w, 3\]"):
        denoise.atrous_pair(a, b[:5], normal, depth, device=False)
    with pytest.raises(_abi.DartRayHipError, match="var_floor must be finite and positive"):
        denoise.atrous_pair(a, b, normal, depth, var_floor=0.0, device=False)


def test_render_denoised_pair_refuses_by_name():
    cam = scenes.cornell_camera(16, 16)

    def renderer(sampler):
        return core.SamplerRenderer(sampler, cam, core.PathIntegrator(3), core.EmissionIntegrator())
    with pytest.raises(ValueError, match="render_denoised_pair: the adaptive sampler is not supported"):
        denoise.render_denoised_pair(renderer(core.AdaptiveSampler(cam, 4, 16, "contrast", 5489)), None)
    host_buffer = core.HostBufferSampler(cam, 1, np.zeros((1, 2), np.int32), np.zeros((1, 5), np.float32))
    with pytest.raises(ValueError, match="render_denoised_pair: HostBufferSampler has no seed to vary"):
        denoise.render_denoised_pair(renderer(host_buffer), None)
    with pytest.raises(ValueError, match="render_denoised_pair: seed_b equals the sampler's seed"):
        denoise.render_denoised_pair(renderer(core.LowDiscrepancySampler(cam, 4, 77)), None, seed_b=77)
    with pytest.raises(ValueError, match="normal_channel must be ns or ng"):
        denoise.render_denoised_pair(renderer(core.LowDiscrepancySampler(cam, 4, 77)), None, normal_channel="uv")
