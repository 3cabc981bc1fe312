"""The edge-avoiding a-trous denoiser without a GPU: answers derived by hand, checked against both the numpy restatement
(tests/denoise_restatement.py, written from the text) and dr_denoise_atrous_host; the two against each other bit for bit on seeded images;
every refusal by code and text; the host code under the address and undefined-behaviour sanitizers as a stand-alone program
(tests/denoise_host_check.cpp); and the Python module above them (dartray_amd/denoise.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, denoise, scenes

import denoise_cases as dc
import denoise_restatement as dr

F = np.float32
same = dr.same_bits


def _both(rgb, normal, depth, iterations, kc, kn, kz):
    """The restatement's and the host entry's results, which must agree before either is compared with a derived answer."""
    a = dr.atrous(rgb, normal, depth, iterations, kc, kn, kz)
    b = dc.host(rgb, normal, depth, iterations, kc, kn, kz)
    assert same(a, b)
    return a


def _flat_guides(w, h):
    return np.full((h, w, 3), 0.25, np.float32), np.full((h, w), 3.0, np.float32)


# ---- 1. answers derived by hand ----
@pytest.mark.parametrize("iterations", [1, 3, 8])
def test_a_constant_image_comes_back_bit_identical(hip, iterations):
    """Every weight is H / (1 + k * 0) = H, a multiple of 1/256; sum = 0.5 * sumw with every partial sum exact, and the quotient is 0.5."""
    rgb = np.full((7, 9, 3), 0.5, np.float32)
    normal, depth = _flat_guides(9, 7)
    for k in dc.K_COMBOS:
        assert same(_both(rgb, normal, depth, iterations, *k), rgb)


def test_a_unit_impulse_gives_the_tap_table(hip):
    rgb = np.zeros((9, 9, 3), np.float32)
    rgb[4, 4] = (1.0, 2.0, 0.5)                                          # powers of two: H * c is exact
    normal, depth = _flat_guides(9, 9)
    out = _both(rgb, normal, depth, 1, 0.0, 0.0, 0.0)
    want = np.zeros_like(rgb)
    for dy in range(-2, 3):
        for dx in range(-2, 3):                                          # all 25 taps of these pixels lie inside: sumw = 1
            want[4 + dy, 4 + dx] = dr.H[dy + 2][dx + 2] * np.array((1.0, 2.0, 0.5), np.float32)
    assert same(out, want) and (out[:2] == 0).all() and (out[:, 7:] == 0).all()


def test_an_impulse_in_a_corner_renormalises_over_the_taps_inside(hip):
    rgb = np.zeros((9, 9, 3), np.float32)
    rgb[0, 0] = 1.0
    normal, depth = _flat_guides(9, 9)
    out = _both(rgb, normal, depth, 1, 0.0, 0.0, 0.0)
    want = np.zeros_like(rgb)
    for y in range(3):
        for x in range(3):
            sumw = F(0)
            for dy in range(-2, 3):                                      # the loop's own order: dy outer, dx inner
                for dx in range(-2, 3):
                    if 0 <= x + dx < 9 and 0 <= y + dy < 9:
                        sumw = sumw + dr.H[dy + 2][dx + 2]
            assert (sumw < 1) == (x < 2 or y < 2)                        # (only pixel (2, 2) has all its taps inside)
            want[y, x] = dr.H[2 - y][2 - x] / sumw                       # the impulse is tap (-x, -y) of pixel (x, y)
    assert same(out, want)


def test_a_normal_edge_stops_the_filter_to_the_derived_bound(hip):
    """Colour 0 left of x = 6 and 1 right of it, normals (0, 0, 0) and (1, 0, 0): dn = 1 across the edge, k_normal = 2^60.  A far-side tap weighs
    H / (1 + 2^60) <= H / 2^60 and sumw >= 9/64 (the centre tap), so a pixel moves by at most (sum of H over its far-side taps) / (9/64) / 2^60."""
    w, h = 12, 6
    rgb = np.zeros((h, w, 3), np.float32)
    rgb[:, 6:] = 1.0
    normal = np.zeros((h, w, 3), np.float32)
    normal[:, 6:, 0] = 1.0
    depth = np.full((h, w), 3.0, np.float32)
    out = _both(rgb, normal, depth, 1, 0.0, 2.0 ** 60, 0.0)
    H = dr.H.astype(np.float64)
    touched = 0
    for y in range(h):
        for x in range(w):
            far = sum(H[dy + 2][dx + 2] for dy in range(-2, 3) for dx in range(-2, 3)
                      if 0 <= x + dx < w and 0 <= y + dy < h and (x + dx >= 6) != (x >= 6))
            bound = far / (9.0 / 64.0) / 2.0 ** 60
            err = np.abs(out[y, x].astype(np.float64) - rgb[y, x]).max()
            assert err <= bound, (x, y, err, bound)
            touched += far > 0
    assert touched == 4 * h                                              # the two columns on either side of the edge
    assert (out[:, :6] > 0).any()                                        # ... and the bound is not met by doing nothing: something did cross


def _scalar_filter(rgb, normal, depth, skip, iterations, kc0, kn, kz):
    """The text once more, as scalar loops with an explicit list of pixels that are no tap and are not filtered."""
    h, w = depth.shape
    cur = rgb.astype(np.float32)
    kn, kz, one = F(kn), F(kz), F(1)
    for i in range(iterations):
        s, kc = 1 << i, dr.level_kc(kc0, i)
        nxt = cur.copy()
        for y in range(h):
            for x in range(w):
                if skip[y, x]:
                    continue
                total, sumw = [F(0), F(0), F(0)], F(0)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qx, qy = x + dx * s, y + dy * s
                        if not (0 <= qx < w and 0 <= qy < h) or skip[qy, qx]:
                            continue
                        cq, cp, nq, np_ = cur[qy, qx], cur[y, x], normal[qy, qx], normal[y, x]
                        d = cq - cp
                        dcol = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
                        d = nq - np_
                        dnor = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
                        dz = (depth[qy, qx] - depth[y, x]) * (depth[qy, qx] - depth[y, x])
                        wt = dr.H[dy + 2][dx + 2]
                        if kc != 0:
                            wt = wt / (one + kc * dcol)
                        if kn != 0:
                            wt = wt / (one + kn * dnor)
                        if kz != 0:
                            wt = wt / (one + kz * dz)
                        total = [total[c] + wt * cq[c] for c in range(3)]
                        sumw = sumw + wt
                nxt[y, x] = [total[c] / sumw for c in range(3)]
        cur = nxt
    return cur


@pytest.mark.parametrize("where", ["colour", "guide", "both"])
def test_non_finite_pixels_pass_through_and_are_no_tap(hip, where):
    w, h = 7, 6
    rng = np.random.Generator(np.random.PCG64(11))
    rgb = rng.random((h, w, 3)).astype(np.float32)
    normal = rng.random((h, w, 3)).astype(np.float32)
    depth = (3.0 + rng.random((h, w))).astype(np.float32)
    clean = (rgb.copy(), normal.copy(), depth.copy())                    # finite stand-ins at the pixels that get the bad values
    skip = np.zeros((h, w), bool)
    for (x, y), v in zip([(0, 0), (3, 2), (6, 5), (4, 3)], [np.nan, np.inf, -np.inf, np.nan]):
        skip[y, x] = True
        if where in ("colour", "both"):
            rgb[y, x, (x + y) % 3] = v
        if where == "guide":
            (normal if x % 2 else depth)[(y, x, 1) if x % 2 else (y, x)] = v
        if where == "both":
            depth[y, x] = -v
    for k in [(0.0, 0.0, 0.0), (1.5, 40.0, 0.3)]:
        out = _both(rgb, normal, depth, 2, *k)
        assert same(out[skip], rgb[skip])                                # unchanged, bit for bit
        want = _scalar_filter(*clean, skip, 2, *k)
        assert same(out[~skip], want[~skip]) and np.isfinite(out[~skip]).all()


# ---- 2. host == restatement, bit for bit ----
@pytest.mark.parametrize("iterations", dc.ITERATIONS)
@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_bit_for_bit(hip, size, iterations):
    rgb, normal, depth = dc.images(*size)
    valid = np.isfinite(rgb).all(axis=2) & np.isfinite(normal).all(axis=2) & np.isfinite(depth)
    if size[0] * size[1] >= 64:
        assert 0 < (~valid).sum() < valid.size // 4 and (normal == 0).all(axis=2).sum() > 4
    for k in dc.K_COMBOS:
        out = _both(rgb, normal, depth, iterations, *k)
        assert same(out[~valid], rgb[~valid])
        assert np.isfinite(out[valid]).all()


def test_the_term_switches_and_levels_matter(hip):
    """The cases above would agree trivially if k or the level count were ignored on both sides."""
    rgb, normal, depth = dc.images(17, 33)
    outs = [dc.host(rgb, normal, depth, 2, *k) for k in dc.K_COMBOS] + [dc.host(rgb, normal, depth, 3, *dc.K_COMBOS[-1])]
    for i in range(len(outs)):
        for j in range(i):
            assert not same(outs[i], outs[j]), (i, j)


# ---- 3. the refusals, by code and text ----
def test_every_refusal_by_code_and_text(hip):
    lib = hip.lib()
    rgb, normal, depth = (np.ascontiguousarray(a[:2, :3]) for a in dc.images(17, 33))
    out = np.zeros_like(rgb)
    ok = dc.params(2, 1.0, 1.0, 1.0)

    def refused(needle, rgb=rgb.ctypes.data, normal=normal.ctypes.data, depth=depth.ctypes.data, w=3, h=2, p=ok, out=out.ctypes.data):
        for fn in (lib.dr_denoise_atrous_host, lib.dr_denoise_atrous):   # the same checks, ahead of any device call
            rc = fn(rgb, normal, depth, w, h, C.byref(p) if p is not None else None, out)
            assert rc == -1, (needle, rc)
            assert needle in lib.dr_last_error().decode(), (needle, lib.dr_last_error())

    for name in ("rgb", "normal", "depth", "p", "out"):
        refused("a null pointer", **{name: None})
    refused("w and h must be at least 1", w=0)
    refused("w and h must be at least 1", h=-2)
    refused("the image has 2^31 or more pixels", w=65536, h=32768)
    refused("the image has 2^31 or more pixels", w=2 ** 31 - 1, h=2)
    for it in (0, 9, -1):
        refused("iterations must be in 1..8", p=dc.params(it, 1.0, 1.0, 1.0))
    for bad in (-1.0, float("inf"), float("nan"), -0.5):
        for which in range(3):
            k = [1.0, 1.0, 1.0]
            k[which] = bad
            refused("must be finite and not negative", p=dc.params(2, *k))
    refused("k_color of the last level is not finite in f32", p=dc.params(2, 3.0e38, 1.0, 1.0))
    _abi.check(lib.dr_denoise_atrous_host(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, 3, 2, C.byref(dc.params(1, 3.0e38, 1.0, 1.0)),
                                          out.ctypes.data))           # ... while one level of the same k is served
    refused("out overlaps an input", out=rgb.ctypes.data)
    refused("out overlaps an input", out=normal.ctypes.data + 4 * 17)   # its first float is normal's last
    refused("out overlaps an input", depth=out.ctypes.data + 4 * 17)
    # the device entry: the same checks and its own, all ahead of any device call; the size query needs no device
    n = C.c_uint64(0)
    assert lib.dr_denoise_atrous_device(None, None, None, 129, 65, C.byref(ok), None, None, C.byref(n), None) == 0
    assert n.value == 48 * 129 * 65
    assert lib.dr_denoise_atrous_device(None, None, None, 129, 65, C.byref(ok), None, None, None, None) == -1
    assert "a null pointer" in lib.dr_last_error().decode()
    assert lib.dr_denoise_atrous_device(None, None, None, 0, 65, C.byref(ok), None, None, C.byref(n), None) == -1
    assert "w and h must be at least 1" in lib.dr_last_error().decode()
    fake = 1 << 20                                                       # addresses that are only compared, never read
    n = C.c_uint64(48 * 6 - 1)
    assert lib.dr_denoise_atrous_device(fake, 2 * fake, 3 * fake, 3, 2, C.byref(ok), 4 * fake, 5 * fake, C.byref(n), None) == -1
    assert "the scratch buffer is too small" in lib.dr_last_error().decode()
    n = C.c_uint64(48 * 6)
    assert lib.dr_denoise_atrous_device(fake, 2 * fake, 3 * fake, 3, 2, C.byref(ok), 4 * fake, 5 * fake + 4, C.byref(n), None) == -1
    assert "not 16-byte aligned" in lib.dr_last_error().decode()
    assert lib.dr_denoise_atrous_device(fake, 2 * fake, 3 * fake, 3, 2, C.byref(ok), 5 * fake + 16, 5 * fake, C.byref(n), None) == -1
    assert "out overlaps the scratch buffer" in lib.dr_last_error().decode()
    assert lib.dr_denoise_atrous_device(fake, 2 * fake, 3 * fake, 3, 2, C.byref(ok), 2 * fake + 8, 5 * fake, C.byref(n), None) == -1
    assert "out overlaps an input" in lib.dr_last_error().decode()


# ---- 4. the host code under the sanitizers, as a program of its own ----
def test_host_filter_runs_clean_under_the_sanitizers(tmp_path):
    """tests/denoise_host_check.cpp + dr_denoise_host.cpp, built with -fsanitize=address,undefined and run as a child process; the
    sanitizer runtimes are linked into the program, which then depends on nothing else the process loads."""
    exe = str(tmp_path / "denoise_host_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "denoise_host_check.cpp"),
                           os.path.join(ROOT, "dartray_amd", "csrc", "dr_denoise_host.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "denoise_host_check: OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ---- 5. the Python module ----
def test_sigmas_become_sharpness_values():
    assert denoise.sharpness(float("inf")) == 0.0 and denoise.sharpness(0.5) == 4.0 and denoise.sharpness(0.1) == float(F(1.0 / (0.1 * 0.1)))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="a sigma must be positive"):
            denoise.sharpness(bad)
    p = denoise.params()
    assert (p.iterations, p.k_color, p.k_normal, p.k_depth) == (5, 1.0, float(F(1.0 / (0.1 * 0.1))), 1.0)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "iterations = 5, sigma_color = 1.0, sigma_normal = 0.1, sigma_depth = 1.0" in design     # the stated defaults are the module's


def test_the_module_on_the_host_equals_the_restatement(hip):
    rgb, normal, depth = dc.images(17, 33)
    got = denoise.atrous(rgb, normal, depth, device=False)
    p = denoise.params()
    assert same(got, dr.atrous(rgb, normal, depth, p.iterations, p.k_color, p.k_normal, p.k_depth))
    got = denoise.atrous(rgb, normal, depth, iterations=2, sigma_color=float("inf"), sigma_normal=0.5, sigma_depth=float("inf"), device=False)
    assert same(got, dr.atrous(rgb, normal, depth, 2, 0.0, 4.0, 0.0))
    with pytest.raises(ValueError, match=r"rgb and normal must be \[h, w, 3\]"):
        denoise.atrous(rgb, normal, depth[:5], device=False)
    with pytest.raises(_abi.DartRayHipError, match="iterations must be in 1..8"):
        denoise.atrous(rgb, normal, depth, iterations=9, device=False)


def test_render_denoised_refuses_the_adaptive_sampler_by_name():
    cam = scenes.cornell_camera(16, 16)
    r = core.SamplerRenderer(core.AdaptiveSampler(cam, 4, 16, "contrast", 5489), cam, core.PathIntegrator(3), core.EmissionIntegrator())
    with pytest.raises(ValueError, match="render_denoised: the adaptive sampler is not supported"):
        denoise.render_denoised(r, None)
    with pytest.raises(ValueError, match="normal_channel must be ns or ng"):
        denoise.render_denoised(r, None, normal_channel="uv")
