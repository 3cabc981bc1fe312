"""The joint bilateral upsampler without a GPU: dr_upsample_host against the numpy restatement (tests/upsample_restatement.py,
written from the text) bit for bit on the smallest images where the rule can go wrong, with and without non-finite values; answers derived
by hand, checked against both; an edge that a plain bilinear zoom would smear; every refusal by code and text; and the Python module above
them (dartray_amd/denoise.py)."""
import ctypes as C

import numpy as np
import pytest

from dartray_amd import _abi, core, denoise, scenes

import upsample_cases as uc
import upsample_restatement as ur

F = np.float32
same = ur.same_bits


def _both(imgs, factor, taps, kn, kz):
    """The restatement's and the host entry's results, which must agree before either is compared with a derived answer."""
    a = ur.upsample(*imgs, factor, taps, kn, kz)
    b = uc.host(*imgs, factor, taps, kn, kz)
    assert same(a, b), (factor, taps, kn, kz)
    return a


def _nearest(rgb_lo, f):
    return np.repeat(np.repeat(rgb_lo, f, axis=0), f, axis=1)


# ---- 1. host == restatement, bit for bit ----
@pytest.mark.parametrize("factor", uc.FACTORS)
@pytest.mark.parametrize("size", uc.LOW_SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_bit_for_bit(hip, size, factor):
    for taps in uc.TAPS:
        imgs = uc.images(*size, factor)
        outs = [_both(imgs, factor, taps, *k) for k in uc.K_COMBOS]
        assert all(np.isfinite(o).all() for o in outs)
        if size == (5, 7):                                               # ... and the switches are read: no two of the four agree
            assert not any(same(outs[i], outs[j]) for i in range(4) for j in range(i))


@pytest.mark.parametrize("invalid", uc.INVALID)
@pytest.mark.parametrize("factor", uc.FACTORS)
@pytest.mark.parametrize("size", uc.LOW_SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_on_non_finite_values(hip, size, factor, invalid):
    imgs = uc.images(*size, factor, invalid=invalid)
    for taps in uc.TAPS:
        for k in uc.K_COMBOS:
            _both(imgs, factor, taps, *k)


def test_taps_and_factor_matter(hip):
    """The cases above would agree trivially if taps were ignored on both sides."""
    imgs = uc.images(5, 7, 2)
    assert not same(uc.host(*imgs, 2, 2, 40.0, 0.3), uc.host(*imgs, 2, 4, 40.0, 0.3))


# ---- 2. invalid data: what the rule promises, beyond agreement ----
@pytest.mark.parametrize("which", ["colour", "normal", "depth"])
def test_an_invalid_low_pixel_is_no_tap(hip, which):
    """The finite colour values of an invalid low-resolution pixel show nowhere but (through the fallback) in the f x f pixels that it is
    the nearest of, and every other pixel is finite: all of them have a valid tap."""
    bad = uc.images(5, 7, 2, invalid=which)
    ok = np.isfinite(bad[0]).all(axis=2) & np.isfinite(bad[1]).all(axis=2) & np.isfinite(bad[2])
    assert (~ok).sum() == 3
    other = [a.copy() for a in bad]
    other[0][~ok] = np.where(np.isfinite(bad[0][~ok]), 1.0e6, bad[0][~ok])
    own = np.repeat(np.repeat(ok, 2, axis=0), 2, axis=1)
    for taps in uc.TAPS:
        a, b = _both(bad, 2, taps, 40.0, 0.3), _both(other, 2, taps, 40.0, 0.3)
        assert same(a[own], b[own]) and np.isfinite(a[own]).all() and a[own].max() < 100.0    # (every valid colour is below 100)


def test_a_pixel_whose_own_guide_is_not_finite_drops_the_edge_terms(hip):
    imgs = uc.images(5, 7, 4, invalid="full")
    plain = np.isfinite(imgs[3]).all(axis=2) & np.isfinite(imgs[4])
    assert (~plain).sum() == 6
    for taps in uc.TAPS:
        edge, spatial = _both(imgs, 4, taps, 40.0, 0.3), _both(imgs, 4, taps, 0.0, 0.0)
        assert same(edge[~plain], spatial[~plain]) and np.isfinite(edge).all()
        assert not (edge[plain] == spatial[plain]).all()


@pytest.mark.parametrize("factor", uc.FACTORS)
def test_a_footprint_without_a_valid_tap_gives_the_nearest_low_pixel_bit_for_bit(hip, factor):
    imgs = uc.images(3, 2, factor, invalid="all")
    assert np.isnan(imgs[0][0, 0]).any() and np.isinf(imgs[0]).any()
    imgs[0].view(np.uint32)[0, 0][np.isnan(imgs[0][0, 0])] = 0xFFC12345    # a NaN with a sign and a payload of its own
    for taps in uc.TAPS:
        for k in uc.K_COMBOS:
            assert same(_both(imgs, factor, taps, *k), _nearest(imgs[0], factor))


def test_weights_that_all_underflow_give_the_nearest_low_pixel(hip):
    imgs, (factor, taps, kn, kz) = uc.overflow_case()
    with np.errstate(over="ignore"):
        assert np.isinf(F(kz) * (imgs[2][0, 0] - imgs[4][0, 0]) ** 2)
    assert same(_both(imgs, factor, taps, kn, kz), _nearest(imgs[0], factor))
    assert not same(_both(imgs, factor, taps, kn, 0.0), _nearest(imgs[0], factor))


# ---- 3. a known answer ----
def test_two_by_two_gives_the_bilinear_blends_in_the_rules_order(hip):
    """f = 2, T = 2, both k zero, low 2 x 2 with colours a, b / c, d.  The tent weights of a full-resolution pixel are 3/4 and 1/4 per axis, so
    the four interior pixels blend with 9/16, 3/16, 3/16, 1/16, the edge pixels renormalise two taps over 3/4 and the corners one over 9/16.
    The colours are multiples of 64: every product, sum and quotient is exact, and the answer is the rational one."""
    a, b, c, d = (np.array(v, np.float64) for v in ((64, 128, 192), (256, 64, 1024), (640, 320, 128), (1920, 448, 64)))
    rgb_lo = np.array([[a, b], [c, d]], np.float32)
    flat = (np.full((2, 2, 3), 0.5, np.float32), np.full((2, 2), 3.0, np.float32), np.full((4, 4, 3), 0.5, np.float32), np.full((4, 4), 3.0, np.float32))
    out = _both((rgb_lo,) + flat, 2, 2, 0.0, 0.0)
    q = [9 / 16, 3 / 16, 3 / 16, 1 / 16]
    assert same(out[1, 1], q[0] * a + q[1] * b + q[2] * c + q[3] * d)
    assert same(out[1, 2], q[1] * a + q[0] * b + q[3] * c + q[2] * d)
    assert same(out[2, 1], q[2] * a + q[3] * b + q[0] * c + q[1] * d)
    assert same(out[2, 2], q[3] * a + q[2] * b + q[1] * c + q[0] * d)
    # ... evaluated as the rule does: tap by tap, row by row, from 0
    w = [F(0.75) * F(0.75), F(0.25) * F(0.75), F(0.75) * F(0.25), F(0.25) * F(0.25)]
    s, sumw = np.zeros(3, np.float32), F(0)
    for wt, col in zip(w, (a, b, c, d)):
        s, sumw = s + wt * col.astype(np.float32), sumw + wt
    assert sumw == 1 and same(out[1, 1], s / sumw)
    for (y, x), col in (((0, 0), a), ((0, 3), b), ((3, 0), c), ((3, 3), d)):
        assert same(out[y, x], col)                                      # the single tap: (9/16 * colour) / (9/16)
    assert same(out[0, 1], 0.75 * a + 0.25 * b) and same(out[2, 0], 0.25 * a + 0.75 * c) and same(out[3, 2], 0.25 * c + 0.75 * d)


# ---- 4. edge keeping ----
@pytest.mark.parametrize("taps", uc.TAPS)
def test_a_depth_step_on_an_odd_column_stays_where_the_full_resolution_guide_puts_it(hip, taps):
    args, far = uc.step_case(taps, denoise.sharpness(denoise.SIGMA_DEPTH))
    out = _both(args[:5], *args[5:])
    assert (out[far] > 0.5).all() and (out[~far] < 0.5).all()            # every pixel on its own side
    plain_args, _ = uc.step_case(taps, 0.0)
    plain = _both(plain_args[:5], *plain_args[5:])
    assert (plain[:, 7] < 0.5).all() and far[:, 7].all()                 # ... which a plain zoom does not manage next to the step
    assert (plain[:, :7] < 0.5).all() and (plain[:, 8:] > 0.5).all()


# ---- 5. the refusals, by code and text ----
def test_every_refusal_by_code_and_text(hip):
    lib = hip.lib()
    rgb_lo, normal_lo, depth_lo, normal, depth = uc.images(3, 2, 2)
    out = np.zeros_like(normal)
    ok = uc.params(2, 2, 1.0, 1.0)
    ptr = dict(rgb_lo=rgb_lo.ctypes.data, normal_lo=normal_lo.ctypes.data, depth_lo=depth_lo.ctypes.data, normal=normal.ctypes.data,
               depth=depth.ctypes.data, out=out.ctypes.data)

    def refused(needle, wl=3, hl=2, p=ok, images_only=False, **over):
        a = dict(ptr, **over)
        pp = C.byref(p) if p is not None else None
        for fn in (lib.dr_upsample_host, lib.dr_upsample):               # the same checks, ahead of any device call
            rc = fn(a["rgb_lo"], a["normal_lo"], a["depth_lo"], wl, hl, a["normal"], a["depth"], pp, a["out"])
            assert rc == -1, (needle, rc)
            assert needle in lib.dr_last_error().decode(), (needle, lib.dr_last_error())
        if not images_only:                                              # dr_upsample_check agrees, and so does the device entry's size query
            n = C.c_uint64(0)
            for rc in (lib.dr_upsample_check(pp, wl, hl), lib.dr_upsample_device(None, None, None, wl, hl, None, None, pp, None, None, C.byref(n), None)):
                assert rc == -1 and needle in lib.dr_last_error().decode(), (needle, rc, lib.dr_last_error())

    for name in ptr:
        refused("a null pointer", images_only=True, **{name: None})
    refused("a null pointer", p=None)
    for bad in (0, 1, 3, 8, -2):
        refused("factor must be 2 or 4", p=uc.params(bad, 2, 1.0, 1.0))
        refused("taps must be 2 or 4", p=uc.params(2, bad, 1.0, 1.0))
    refused("wl and hl must be at least 1", wl=0)
    refused("wl and hl must be at least 1", hl=-2)
    refused("the image has 2^31 or more pixels", wl=32768, hl=16384)     # 2^29 * 4
    refused("the image has 2^31 or more pixels", wl=2 ** 31 - 1, hl=2 ** 31 - 1)
    refused("the image has 2^31 or more pixels", wl=16384, hl=8192, p=uc.params(4, 2, 1.0, 1.0))     # 2^27 * 16
    assert lib.dr_upsample_check(C.byref(ok), 32768, 16383) == 0 and lib.dr_upsample_check(C.byref(uc.params(4, 4, 0.0, 0.0)), 16384, 8191) == 0
    for bad in (-1.0, float("inf"), float("nan"), -0.5):
        refused("k_normal and k_depth must be finite and not negative", p=uc.params(2, 2, bad, 1.0))
        refused("k_normal and k_depth must be finite and not negative", p=uc.params(2, 2, 1.0, bad))
    for name, nbytes in (("rgb_lo", 72), ("normal_lo", 72), ("depth_lo", 24), ("normal", 288), ("depth", 96)):
        refused("out overlaps an input", images_only=True, out=ptr[name])
        refused("out overlaps an input", images_only=True, out=ptr[name] + nbytes - 4)               # its first float is the input's last
        refused("out overlaps an input", images_only=True, **{name: ptr["out"] + 288 - 4})
    assert lib.dr_upsample_check(C.byref(ok), 3, 2) == 0
    # the device entry: the same checks and its own, all ahead of any device call; the size query needs no device
    n = C.c_uint64(0)
    assert lib.dr_upsample_device(None, None, None, 129, 65, None, None, C.byref(ok), None, None, C.byref(n), None) == 0
    assert n.value == 32 * 129 * 65
    assert lib.dr_upsample_device(None, None, None, 129, 65, None, None, C.byref(ok), None, None, None, None) == -1
    assert "a null pointer" in lib.dr_last_error().decode()
    fake = 1 << 20                                                       # addresses that are only compared, never read

    def device(out_addr, scratch_addr, nbytes):
        n = C.c_uint64(nbytes)
        return lib.dr_upsample_device(fake, 2 * fake, 3 * fake, 3, 2, 4 * fake, 5 * fake, C.byref(ok), out_addr, scratch_addr, C.byref(n), None)
    assert device(6 * fake, 7 * fake, 32 * 6 - 1) == -1 and "the scratch buffer is too small" in lib.dr_last_error().decode()
    assert device(6 * fake, 7 * fake + 4, 32 * 6) == -1 and "not 16-byte aligned" in lib.dr_last_error().decode()
    assert device(7 * fake + 16, 7 * fake, 32 * 6) == -1 and "out overlaps the scratch buffer" in lib.dr_last_error().decode()
    assert device(4 * fake + 8, 7 * fake, 32 * 6) == -1 and "out overlaps an input" in lib.dr_last_error().decode()


def test_the_struct_is_sixteen_bytes_in_every_binding():
    assert C.sizeof(_abi.DrUpsampleParams) == 16
    assert [(n, getattr(_abi.DrUpsampleParams, n).offset) for n, _ in _abi.DrUpsampleParams._fields_] == [("factor", 0), ("taps", 4), ("k_normal", 8),
                                                                                                         ("k_depth", 12)]


# ---- 6. the Python module ----
def test_the_module_on_the_host_equals_the_restatement(hip):
    imgs = uc.images(5, 7, 4)
    p = denoise.upsample_params(4)
    assert (p.factor, p.taps, p.k_normal, p.k_depth) == (4, 2, denoise.sharpness(denoise.SIGMA_NORMAL), denoise.sharpness(denoise.SIGMA_DEPTH))
    got = denoise.upsample(*imgs, device=False)                          # the factor from the shapes
    assert got.shape == (28, 20, 3) and got.dtype == np.float32
    assert same(got, ur.upsample(*imgs, 4, 2, p.k_normal, p.k_depth))
    got = denoise.upsample(*uc.images(5, 7, 2), factor=2, taps=4, sigma_normal=float("inf"), sigma_depth=0.5, device=False)
    assert same(got, ur.upsample(*uc.images(5, 7, 2), 2, 4, 0.0, 4.0))
    rgb_lo, normal_lo, depth_lo, normal, depth = imgs
    with pytest.raises(ValueError, match=r"rgb_lo and normal_lo must be \[hl, wl, 3\] and depth_lo \[hl, wl\] \(got \(7, 5, 3\), \(7, 5, 3\), \(7, 4\)\)"):
        denoise.upsample(rgb_lo, normal_lo, depth_lo[:, :4], normal, depth, device=False)
    with pytest.raises(ValueError, match=r"normal must be \[h, w, 3\] and depth \[h, w\] \(got \(28, 20, 3\), \(27, 20\)\)"):
        denoise.upsample(rgb_lo, normal_lo, depth_lo, normal, depth[:27], device=False)
    with pytest.raises(ValueError, match=r"must be 2 or 4 times the low-resolution image in both axes \(got \(21, 15\) for \(7, 5\)\)"):
        denoise.upsample(rgb_lo, normal_lo, depth_lo, normal[:21, :15], depth[:21, :15], device=False)
    with pytest.raises(ValueError, match=r"must be 4 times the low-resolution image in both axes \(got \(28, 10\) for \(7, 5\)\)"):
        denoise.upsample(rgb_lo, normal_lo, depth_lo, normal[:, :10], depth[:, :10], device=False)
    with pytest.raises(ValueError, match=r"must be 2 times the low-resolution image in both axes \(got \(28, 20\) for \(7, 5\)\)"):
        denoise.upsample(rgb_lo, normal_lo, depth_lo, normal, depth, factor=2, device=False)
    with pytest.raises(_abi.DartRayHipError, match="taps must be 2 or 4"):
        denoise.upsample(rgb_lo, normal_lo, depth_lo, normal, depth, taps=3, device=False)
    with pytest.raises(ValueError, match="a sigma must be positive"):
        denoise.upsample(rgb_lo, normal_lo, depth_lo, normal, depth, sigma_depth=0.0, device=False)


def test_the_pbrt_loader_builds_the_low_resolution_renderer_from_the_same_file(hip, tmp_path):
    from dartray_amd import pbrt
    assert pbrt.loads(uc.TINY_PBRT).lowRendererObject is None
    for f, res in ((2, (12, 8)), (4, (6, 4))):
        api = pbrt.loads(uc.TINY_PBRT, upsample=f)
        low, full = api.lowRendererObject, api.rendererObject
        assert (low.camera.film.xResolution, low.camera.film.yResolution) == res
        assert (full.camera.film.xResolution, full.camera.film.yResolution) == (24, 16)
        assert low.sampler.camera is low.camera and low.camera is not full.camera
        assert denoise._upsample_refusals("render_upsampled", low, full) == f
    with pytest.raises(ValueError, match=r"upsample 4: the film's resolution, 26 x 16, is not a multiple of 4 in both axes"):
        pbrt.loads(uc.TINY_PBRT, upsample=4, overrides={"xresolution": 26})
    with pytest.raises(ValueError, match="upsample must be 2 or 4"):
        pbrt.loads(uc.TINY_PBRT, upsample=3)
    scene = tmp_path / "tiny.pbrt"
    scene.write_text(uc.TINY_PBRT)
    with pytest.raises(SystemExit):                                      # the command line refuses it before any render
        pbrt.main([str(scene), "--upsample", "4", "--xres", "26"])
    with pytest.raises(SystemExit):
        pbrt.main([str(scene), "--upsample", "3"])


def _renderer(res, sampler=None, **kw):
    cam = scenes.cornell_camera(*res)
    return core.SamplerRenderer(sampler(cam) if sampler else core.LowDiscrepancySampler(cam, 4, 5489), cam, core.PathIntegrator(3),
                                core.EmissionIntegrator(), **kw)


def test_render_upsampled_refuses_by_name_before_it_renders():
    low, full = _renderer((16, 16)), _renderer((32, 32))
    with pytest.raises(ValueError, match="render_upsampled: normal_channel must be ns or ng"):
        denoise.render_upsampled(low, full, None, normal_channel="uv")
    for res in ((48, 48), (32, 64), (16, 16), (8, 8), (128, 128)):
        with pytest.raises(ValueError, match=r"full_renderer's film must be exactly 2 or 4 times low_renderer's in both axes \(got %d x %d for 16 x 16\)" % res):
            denoise.render_upsampled(low, _renderer(res), None)
    adaptive = lambda cam: core.AdaptiveSampler(cam, 4, 16, "contrast", 5489)
    with pytest.raises(ValueError, match=r"render_upsampled: the adaptive sampler is not supported \(low_renderer"):
        denoise.render_upsampled(_renderer((16, 16), adaptive), full, None)
    with pytest.raises(ValueError, match=r"render_upsampled: the adaptive sampler is not supported \(full_renderer"):
        denoise.render_upsampled(low, _renderer((32, 32), adaptive), None)
    with pytest.raises(ValueError, match=r"render_upsampled: tileCount > 1 is not supported \(full_renderer has tileCount 2\)"):
        denoise.render_upsampled(low, _renderer((32, 32), tileCount=2), None)
    with pytest.raises(ValueError, match=r"render_upsampled: taskCount > 1 is not supported \(low_renderer has taskCount 4\)"):
        denoise.render_upsampled(_renderer((16, 16), taskCount=4), full, None)
    cropped = _renderer((32, 32))
    cropped.camera.film = core.ImageFilm(32, 32, core.BoxFilter(0.5, 0.5), (0.0, 0.5, 0.0, 1.0))
    with pytest.raises(ValueError, match=r"render_upsampled: a crop window other than the whole film is not supported \(full_renderer has \(0.0, 0.5, 0.0, 1.0\)\)"):
        denoise.render_upsampled(low, cropped, None)
    with pytest.raises(ValueError, match="render_upsampled: iterations given without denoise=True"):
        denoise.render_upsampled(low, full, None, iterations=3)
    moved = _renderer((32, 32))
    moved.camera.cameraToWorld = np.array(moved.camera.cameraToWorld, copy=True)
    moved.camera.cameraToWorld.reshape(-1)[3] += 1.0
    with pytest.raises(ValueError, match="render_upsampled: low_renderer's and full_renderer's cameras differ in their pose"):
        denoise.render_upsampled(low, moved, None)
