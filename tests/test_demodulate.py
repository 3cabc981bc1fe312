"""Demodulation on the host (no GPU): dr_demodulate_host / dr_remodulate_host against the numpy restatement
(tests/demodulate_restatement.py) bit for bit, the exact round trip, the refusals by name, the Python module, and the `demodulate` keyword
of the render_* functions with the renders replaced by fixed images, so that the whole chain runs through the host loops."""
import ctypes as C
import os

import numpy as np
import pytest

from dartray_amd import _abi, core, denoise, scenes

import demodulate_cases as dc
import demodulate_restatement as dm
import denoise_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
same = dc.same


def _host(entry, rgb, e, a, eps=dc.EPS):
    h, w = rgb.shape[:2]
    out = np.full_like(rgb, 7.0)
    p = _abi.DrDemodulateParams(eps)
    rc = getattr(_abi.lib(), entry)(rgb.ctypes.data, e.ctypes.data if e is not None else None, a.ctypes.data if a is not None else None, w, h,
                                    C.byref(p), out.ctypes.data)
    assert rc == 0, _abi.lib().dr_last_error()
    return out


# ---- 1. the host loops against numpy ----
@pytest.mark.parametrize("absent", sorted(dc.ABSENT))
@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_host_loops_equal_the_restatement_bit_for_bit(hip, size, absent):
    has_e, has_a = dc.ABSENT[absent]
    seen_invalid = seen_clamped = False
    for rgb, e, a in dc.images(*size):
        e, a = e if has_e else None, a if has_a else None
        d = _host("dr_demodulate_host", rgb, e, a)
        want = dm.demodulate(rgb, e, a, dc.EPS)
        assert same(d, want), (size, absent)
        filtered = np.ascontiguousarray(np.where(np.isfinite(want), want * F(0.75), want), F)     # what a filter might hand back
        assert same(_host("dr_remodulate_host", filtered, e, a), dm.remodulate(filtered, e, a, dc.EPS))
        invalid = ~np.isfinite(rgb).all(axis=2) | (~np.isfinite(e).all(axis=2) if has_e else False) | (~np.isfinite(a).all(axis=2) if has_a else False)
        assert same(d[invalid], rgb[invalid]) and np.isfinite(d[~invalid]).all()                  # passed through with its bits; nothing else is
        seen_invalid |= bool(np.any(invalid))
        seen_clamped |= bool(has_e and np.any((rgb < e)[~invalid]) and (d[~invalid][(rgb < e)[~invalid]] == 0.0).all())
    assert seen_invalid and (seen_clamped or not has_e)


def test_the_special_pixels_do_what_the_section_says(hip):
    (rgb, e, a), = dc.images(3, 5)
    d = _host("dr_demodulate_host", rgb, e, a).reshape(-1, 3)
    rgb, e, a = (x.reshape(-1, 3) for x in (rgb, e, a))
    assert (a[3] == 0.0).all() and same(d[3], rgb[3] / F(dc.EPS))                              # zero albedo: divided by eps
    assert (rgb[10] < e[10]).all() and (d[10] == 0.0).all() and not np.signbit(d[10]).any()     # one ulp below: +0
    assert same(rgb[2], e[2]) and (d[2] == 0.0).all()                                           # a pure emitter: nothing left to filter
    back = _host("dr_remodulate_host", np.ascontiguousarray(d.reshape(5, 3, 3)), e.reshape(5, 3, 3), a.reshape(5, 3, 3)).reshape(-1, 3)
    assert same(back[2], e[2]) and same(back[10], e[10])                                        # ... and the emitter comes back exactly


@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_round_trip_is_exact_where_every_operation_is(hip, size):
    rgb, e, a, eps = dc.exact_images(*size)
    d = _host("dr_demodulate_host", rgb, e, a, eps)
    assert same(d, dm.demodulate(rgb, e, a, eps)) and (d >= 0).all()
    assert same(_host("dr_remodulate_host", d, e, a, eps), rgb) and (d != rgb).any()
    # and with the defaults it is the identity up to the two roundings of the divide and the multiply
    rgb, e, a = dc.images(67, 9)[0]
    ok = np.isfinite(rgb).all(axis=2) & np.isfinite(e).all(axis=2) & np.isfinite(a).all(axis=2) & (rgb >= e).all(axis=2)
    back = _host("dr_remodulate_host", _host("dr_demodulate_host", rgb, e, a), e, a)
    assert np.allclose(back[ok], rgb[ok], rtol=4 * 2.0 ** -24, atol=0.0)


# ---- 2. the refusals ----
def test_refusals_by_name(hip):
    lib = _abi.lib()
    why = lambda: lib.dr_last_error().decode()
    P = _abi.DrDemodulateParams
    assert lib.dr_demodulate_check(C.byref(P(1e-3)), 4, 4) == 0
    for eps in (0.0, -1e-3, float("nan"), float("inf")):
        assert lib.dr_demodulate_check(C.byref(P(eps)), 4, 4) == -1 and "dr_demodulate_check: eps must be finite and positive" in why()
    assert lib.dr_demodulate_check(C.byref(P(1e-3)), 0, 4) == -1 and "w and h must be at least 1" in why()
    assert lib.dr_demodulate_check(C.byref(P(1e-3)), 1 << 16, 1 << 15) == -1 and "the image has 2^31 or more pixels" in why()
    assert lib.dr_demodulate_check(None, 4, 4) == -1 and "a null pointer" in why()
    buf = np.zeros((4, 4, 3), F)
    out = np.zeros((4, 4, 3), F)
    p = P(1e-3)
    for name in ("dr_demodulate_host", "dr_remodulate_host"):
        fn = getattr(lib, name)
        assert fn(None, None, None, 4, 4, C.byref(p), out.ctypes.data) == -1 and name + ": a null pointer" in why()
        assert fn(buf.ctypes.data, None, None, 4, 4, C.byref(p), None) == -1 and name + ": a null pointer" in why()
        assert fn(buf.ctypes.data, None, None, 4, 4, None, out.ctypes.data) == -1 and name + ": a null pointer" in why()
        assert fn(buf.ctypes.data, None, None, 4, 4, C.byref(p), buf.ctypes.data) == -1 and name + ": an output overlaps an input" in why()
        assert fn(buf.ctypes.data, out.ctypes.data, None, 4, 4, C.byref(p), out.ctypes.data) == -1 and "an output overlaps an input" in why()
        assert fn(buf.ctypes.data, None, out.ctypes.data + 12, 4, 3, C.byref(p), out.ctypes.data) == -1 and "an output overlaps an input" in why()
        assert fn(buf.ctypes.data, None, None, 4, 4, C.byref(p), out.ctypes.data) == 0


# ---- 3. the Python module ----
def test_the_default_eps_is_the_documented_one():
    assert denoise.DEMODULATE_EPS == 1.0e-3 and denoise.demodulate_params().eps == float(F(1.0e-3))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "eps = 1e-3" in design and "reasoned, not tuned" in design.split("### 2.27")[1].split("\n## ")[0]


def test_the_module_on_the_host_equals_the_restatement(hip):
    rgb, e, a = dc.images(67, 9)[0]
    assert same(denoise.demodulate(rgb, e, a, device=False), dm.demodulate(rgb, e, a, 1e-3))
    assert same(denoise.demodulate(rgb, albedo=a, device=False), dm.demodulate(rgb, None, a, 1e-3))
    assert same(denoise.demodulate(rgb.astype(np.float64), e.tolist(), eps=0.5, device=False), dm.demodulate(rgb, e, None, 0.5))
    assert same(denoise.remodulate(rgb, e, a, device=False), dm.remodulate(rgb, e, a, 1e-3))
    assert same(denoise.remodulate(rgb, device=False), dm.remodulate(rgb, None, None, 1e-3))
    with pytest.raises(ValueError, match=r"demodulate: rgb, emission and albedo must be \[h, w, 3\] \(got \(9, 67, 3\), \(9, 66, 3\)\)"):
        denoise.demodulate(rgb, e[:, :66], device=False)
    with pytest.raises(ValueError, match=r"remodulate: rgb, emission and albedo must be \[h, w, 3\]"):
        denoise.remodulate(rgb[..., 0], e, a, device=False)
    with pytest.raises(_abi.DartRayHipError, match="eps must be finite and positive"):
        denoise.demodulate(rgb, e, a, eps=0.0, device=False)


def _renderer():
    cam = scenes.cornell_camera(16, 16)
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, 4, 5489), cam, core.PathIntegrator(3), core.EmissionIntegrator())


def test_the_demodulate_keyword_refuses_by_name_before_anything_renders():
    r = _renderer()
    calls = {"render_denoised": lambda **kw: denoise.render_denoised(r, None, **kw),
             "render_denoised_pair": lambda **kw: denoise.render_denoised_pair(r, None, **kw),
             "render_sequence": lambda **kw: denoise.render_sequence([r], None, **kw)}
    for who, call in calls.items():
        for bad in (1, "albedo", (), ("albedo", "albedo"), ("emission", "roughness"), {"eps": 1.0}):
            with pytest.raises(ValueError, match=r"%s: demodulate must be False, True or a tuple of \"emission\" and / or \"albedo\", got " % who):
                call(demodulate=bad)
        for good in (True, ("emission",), ("albedo",), ("emission", "albedo"), ["albedo", "emission"]):
            with pytest.raises(ValueError, match="%s: one_pass=True together with demodulate is not supported" % who):
                call(demodulate=good, one_pass=True)
    assert denoise._demodulate_kw("x", False) is None and denoise._demodulate_kw("x", None) is None
    assert denoise._demodulate_kw("x", True) == ("emission", "albedo") == denoise._demodulate_kw("x", ["albedo", "emission"])
    assert denoise._demodulate_kw("x", ("albedo",)) == ("albedo",)


# ---- 4. the keyword through the host loops: the renders are fixed images ----
class _Fixed:
    """Stands in for the module's three sources of rendered images and counts what was asked for."""

    def __init__(self, monkeypatch, w=17, h=33):
        rgb, normal, depth = denoise_cases.images(w, h)
        rng = np.random.default_rng(5)
        self.rgb, self.normal, self.depth = rgb, normal, depth
        self.emission = np.where(rng.random((h, w, 1)) < 0.2, np.minimum(rgb, F(0.5)), F(0)).astype(F)
        self.albedo = rng.choice(np.array([0.0, 0.25, 0.5, 0.75], F), (h, w, 3)).astype(F)
        self.material_renders = []
        beauty = core.OutputImage(0, 0, w, h, rgb, None)
        monkeypatch.setattr(denoise, "_beauty_and_guides", lambda renderer, scene, channel, one_pass: (beauty, normal, depth))

        def rerender(renderer, scene, surface, sampler=None):
            assert isinstance(surface, core.MaterialIntegrator)
            self.material_renders.append(surface.channel)
            return core.OutputImage(0, 0, w, h, getattr(self, surface.channel), None)
        monkeypatch.setattr(denoise, "_rerender", rerender)


def test_render_denoised_without_the_keyword_is_what_it_was(hip, monkeypatch):
    fx = _Fixed(monkeypatch)
    want = denoise.atrous(fx.rgb, fx.normal, fx.depth, device=False)
    for kw in ({}, {"demodulate": False}, {"demodulate": None}):
        out = denoise.render_denoised(_renderer(), None, device=False, **kw)
        assert same(out.rgb, want) and same(out.noisy, fx.rgb) and not hasattr(out, "emission") and not hasattr(out, "demodulated")
    clamped = denoise.firefly(fx.rgb, fx.normal, fx.depth, device=False)
    out = denoise.render_denoised(_renderer(), None, firefly={"device": False}, device=False, iterations=2)
    assert same(out.rgb, denoise.atrous(clamped, fx.normal, fx.depth, iterations=2, device=False))
    assert fx.material_renders == []                                 # no material image was rendered


@pytest.mark.parametrize("channels", [True, ("emission",), ("albedo",)], ids=["both", "emission", "albedo"])
def test_render_denoised_with_the_keyword_is_the_chain_by_hand(hip, monkeypatch, channels):
    fx = _Fixed(monkeypatch)
    names = ("emission", "albedo") if channels is True else channels
    e, a = (fx.emission if "emission" in names else None), (fx.albedo if "albedo" in names else None)
    out = denoise.render_denoised(_renderer(), None, demodulate=channels, firefly={"device": False}, device=False, iterations=3)
    assert fx.material_renders == list(names)
    base = dm.demodulate(fx.rgb, e, a, 1e-3)
    clamped = denoise.firefly(base, fx.normal, fx.depth, device=False)             # demodulation comes before the firefly clamp
    want = dm.remodulate(denoise.atrous(clamped, fx.normal, fx.depth, iterations=3, device=False), e, a, 1e-3)
    assert same(out.rgb, want) and same(out.demodulated, base) and same(out.noisy, fx.rgb)
    assert (hasattr(out, "emission"), hasattr(out, "albedo")) == (e is not None, a is not None)
    assert not same(out.rgb, denoise.atrous(denoise.firefly(fx.rgb, fx.normal, fx.depth, device=False), fx.normal, fx.depth, iterations=3, device=False))


# ---- 5. the end-to-end scene of tests/test_gpu_demodulate.py, unfiltered, on the CPU oracle ----
def test_the_unfiltered_reference_holds_lemit_inside_the_emitter(ob, monkeypatch):
    """The condition the GPU test asks of the filtered image, asked of the oracle's unfiltered one: every pixel wholly inside the emitter --
    ten pixels across at 32 x 32 -- is Lemit to the film's tolerance (the XYZ round trip of the film is not exact), and the ring around it is not."""
    monkeypatch.setenv("DARTRAY_BVH_BUILDER", "host")
    cam = scenes.cornell_camera(32, 32)
    r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 4, 5489), cam, core.PathIntegrator(3), core.EmissionIntegrator())
    rgb = ob.OracleScene(dc.emitter_box_prims()).render(ob.render_desc(r, sampler_mode=1))["rgb"]
    inside = rgb[dc.INSIDE]
    assert inside.shape == (10, 10, 3) and np.allclose(inside, np.array(dc.LEMIT, F), rtol=dc.EMITTER_RTOL, atol=dc.EMITTER_ATOL)
    ring = rgb[9:23, 9:23].copy()
    ring[1:-1, 1:-1] = 0
    assert ring.max() < 1.5 and rgb[16, 8].max() > 0.1          # the pixels around the emitter's partly covered rim: the dim back wall
