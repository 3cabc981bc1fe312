"""The one-pass guide render's host side (dr_render_guides_check, SamplerRenderer.guides_desc, the one_pass keyword): every
refusal by code and text, every accepted integrator, the struct in every binding.  No GPU: the check needs neither a scene nor a device, and
a refused one_pass=True raises before anything is rendered."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, denoise, pbrt

DR_ERR_INVALID, DR_ERR_UNSUPPORTED = -1, -4
SEED = 5489
T = pbrt.Transform


def _camera(w=8, h=6):
    return core.PerspectiveCamera.lookAt((0.0, 3.0, -6.0), (0.0, 1.2, 2.0), (0.0, 1.0, 0.0), 50.0, core.ImageFilm(w, h, core.BoxFilter(0.5, 0.5)))


def _scene():
    quad = core.TriangleMesh(np.array(((0, 1, 2), (0, 2, 3)), np.uint32), np.array([(-4.0, 0.0, -2.0), (-4.0, 0.0, 5.0), (4.0, 0.0, 5.0), (4.0, 0.0, -2.0)], np.float32))
    accel = core.BVHAccel([core.GeometricPrimitive(quad, core.MatteMaterial((0.5, 0.5, 0.5)), None)])
    return core.Scene(accel, [core.PointLight(T.Translate(0.0, 6.0, -3.0).m, (30.0, 30.0, 30.0))])


def _renderer(surface, sampler=None):
    cam = _camera()
    return core.SamplerRenderer(sampler(cam) if sampler else core.LowDiscrepancySampler(cam, 4, SEED), cam, surface, core.EmissionIntegrator())


def _guides(*channels, count=None):
    g = _abi.DrGuidesDesc()
    g.count = len(channels) if count is None else count
    for i, c in enumerate(channels[:_abi.DR_GUIDES_MAX]):
        g.channels[i] = c
    return g


def _answer(d, g, nprims=12):
    lib = _abi.lib()
    rc = lib.dr_render_guides_check(C.byref(d), C.byref(g), nprims)
    return rc, lib.dr_last_error().decode()


ACCEPTED = {"path": lambda: core.PathIntegrator(3), "direct_all": lambda: core.DirectLightingIntegrator(0, 3),
            "direct_one": lambda: core.DirectLightingIntegrator(1, 3), "whitted": lambda: core.WhittedIntegrator(3),
            "ao": lambda: core.AmbientOcclusionIntegrator(4)}
REFUSED = {"feature": (lambda: core.FeatureIntegrator("ns"), "render guides: the feature integrator is not supported"),
           "diffuse_prt": (lambda: core.DiffusePRTIntegrator(2, 8), "render guides: the diffuse PRT integrator is not supported"),
           "glossy_prt": (lambda: core.GlossyPRTIntegrator(lmax=2, nSamples=8), "render guides: the glossy PRT integrator is not supported"),
           "use_probes": (lambda: core.UseProbesIntegrator(None), "render guides: the use probes integrator is not supported")}
BOTH = _guides(_abi.DR_FEATURE_NS, _abi.DR_FEATURE_DEPTH)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_every_accepted_integrator_is_accepted(hip, name):
    d, keep = _renderer(ACCEPTED[name]()).describe()
    assert _answer(d, BOTH)[0] == 0
    assert _answer(d, _guides(*range(5)))[0] == 0
    assert _answer(d, _guides(_abi.DR_FEATURE_ID, _abi.DR_FEATURE_NG))[0] == 0


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_every_other_integrator_is_refused_by_name(hip, name):
    make, needle = REFUSED[name]
    d, keep = _renderer(make()).describe()
    rc, why = _answer(d, BOTH)
    assert rc == DR_ERR_UNSUPPORTED and needle in why, (rc, why)


def test_an_unknown_integrator_and_null_arguments(hip):
    d, keep = _renderer(core.PathIntegrator(3)).describe()
    for value in (6, 8, 10, 12, -1):
        d.integrator = value
        rc, why = _answer(d, BOTH)
        assert rc == DR_ERR_INVALID and "render guides: unknown integrator" in why, (value, rc, why)
    lib = _abi.lib()
    assert lib.dr_render_guides_check(None, C.byref(BOTH), 1) == DR_ERR_INVALID and "null argument" in lib.dr_last_error().decode()
    d.integrator = _abi.DR_INTEGRATOR_PATH
    assert lib.dr_render_guides_check(C.byref(d), None, 1) == DR_ERR_INVALID and "null argument" in lib.dr_last_error().decode()


def test_the_adaptive_sampler_is_refused_by_name(hip):
    d, keep = _renderer(core.PathIntegrator(3), lambda cam: core.AdaptiveSampler(cam, 2, 8, "contrast", SEED)).describe()
    assert d.sampler_mode == _abi.DR_SAMPLER_ADAPTIVE
    rc, why = _answer(d, BOTH)
    assert rc == DR_ERR_UNSUPPORTED and "render guides: the adaptive sampler is not supported" in why, (rc, why)
    # every sampler mode the feature integrator accepts is accepted
    for mk in (lambda cam: core.StratifiedSampler(cam, 2, 2, True, SEED), lambda cam: core.HaltonSampler(cam, 5, SEED),
               lambda cam: core.RandomSampler(cam, 4, SEED)):
        d, keep = _renderer(core.PathIntegrator(3), mk).describe()
        assert _answer(d, BOTH)[0] == 0
    d.sampler_mode = _abi.DR_SAMPLER_HOST_BUFFER
    assert _answer(d, BOTH)[0] == 0


def test_the_channel_list_is_refused_by_name(hip):
    d, keep = _renderer(core.PathIntegrator(3)).describe()
    cases = [(_guides(), "render guides: the channel list is empty"),
             (_guides(count=-3), "render guides: the channel list is empty"),
             (_guides(_abi.DR_FEATURE_NS, _abi.DR_FEATURE_DEPTH, _abi.DR_FEATURE_NS), "render guides: a channel is given twice"),
             (_guides(_abi.DR_FEATURE_DEPTH, _abi.DR_FEATURE_DEPTH), "render guides: a channel is given twice"),
             (_guides(_abi.DR_FEATURE_NS, 5), "render guides: unknown channel"),
             (_guides(-1), "render guides: unknown channel"),
             (_guides(1 << 20, _abi.DR_FEATURE_NS), "render guides: unknown channel"),
             (_guides(0, 1, 2, 3, 4, count=6), "render guides: more than five channels"),
             (_guides(0, 1, 2, 3, 4, count=1 << 30), "render guides: more than five channels")]
    for g, needle in cases:
        rc, why = _answer(d, g)
        assert rc == DR_ERR_INVALID and needle in why, (needle, rc, why)
    # entries behind `count` are not read
    g = _guides(_abi.DR_FEATURE_NS, 99, count=1)
    assert _answer(d, g)[0] == 0


def test_the_id_channel_keeps_the_feature_integrators_primitive_limit(hip):
    d, keep = _renderer(core.PathIntegrator(3)).describe()
    ids = _guides(_abi.DR_FEATURE_DEPTH, _abi.DR_FEATURE_ID)
    assert _answer(d, ids, (1 << 24) - 1)[0] == 0
    for n in (1 << 24, (1 << 24) + 7):
        rc, why = _answer(d, ids, n)
        assert rc == DR_ERR_UNSUPPORTED and "render guides: the id channel needs a scene of fewer than 2^24 primitives" in why, (rc, why)
        assert _answer(d, BOTH, n)[0] == 0
        assert _abi.lib().dr_feature_check(_abi.DR_FEATURE_ID, n) == DR_ERR_UNSUPPORTED      # (the same limit)


def test_guides_desc_raises_value_error_with_the_librarys_text(hip):
    scene = _scene()
    d, keep, g = _renderer(core.PathIntegrator(3)).guides_desc(scene, ("ns", "depth"))
    assert g.count == 2 and list(g.channels)[:2] == [_abi.DR_FEATURE_NS, _abi.DR_FEATURE_DEPTH] and d.integrator == _abi.DR_INTEGRATOR_PATH
    with pytest.raises(ValueError, match="render guides: the feature integrator is not supported .*FeatureIntegrator"):
        _renderer(core.FeatureIntegrator("ns")).guides_desc(scene, ("ns", "depth"))
    with pytest.raises(ValueError, match="channel must be one of ng, ns, depth, uv, id"):
        _renderer(core.PathIntegrator(3)).guides_desc(scene, ("ns", "albedo"))
    with pytest.raises(ValueError, match="a channel is given twice"):
        _renderer(core.PathIntegrator(3)).guides_desc(scene, ("ns", "ns"))
    with pytest.raises(ValueError, match="the channel list is empty"):
        _renderer(core.PathIntegrator(3)).guides_desc(scene, ())
    with pytest.raises(ValueError, match="more than five channels"):
        _renderer(core.PathIntegrator(3)).guides_desc(scene, ("ng", "ns", "depth", "uv", "id", "ng"))


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_render(monkeypatch):
    """Any attempt to reach the device scene -- a render -- raises."""
    def boom(self):
        raise _NoDevice("a render was started")
    monkeypatch.setattr(core.Scene, "_device", boom)


CALLS = {"render_denoised": lambda r, s, **kw: denoise.render_denoised(r, s, **kw),
         "render_denoised_pair": lambda r, s, **kw: denoise.render_denoised_pair(r, s, **kw),
         "render_firefly": lambda r, s, **kw: denoise.render_firefly(r, s, **kw),
         "render_sequence": lambda r, s, **kw: denoise.render_sequence([r, r], s, **kw),
         "render_upsampled": lambda r, s, **kw: denoise.render_upsampled(
             core.SamplerRenderer(core.LowDiscrepancySampler(_camera(4, 3), 4, SEED), _camera(4, 3), r.surfaceIntegrator, core.EmissionIntegrator()), r, s, **kw)}


@pytest.mark.parametrize("fn", sorted(CALLS))
def test_one_pass_refuses_an_integrator_before_anything_is_rendered(hip, no_render, fn):
    scene = _scene()
    for name in ("diffuse_prt", "use_probes"):
        make, needle = REFUSED[name]
        with pytest.raises(ValueError, match="%s: one_pass=True: %s" % (fn, needle)):
            CALLS[fn](_renderer(make()), scene, one_pass=True)
    # an accepted integrator gets as far as the render
    with pytest.raises(_NoDevice):
        CALLS[fn](_renderer(core.PathIntegrator(3)), scene, one_pass=True)


@pytest.mark.parametrize("fn", sorted(CALLS))
def test_one_pass_must_be_a_bool(hip, no_render, fn):
    scene = _scene()
    for bad in (1, 0, "yes", None, ("ns",)):
        with pytest.raises(ValueError, match="%s: one_pass must be False or True" % fn):
            CALLS[fn](_renderer(core.PathIntegrator(3)), scene, one_pass=bad)


def test_the_struct_is_twenty_four_bytes_in_every_binding():
    assert C.sizeof(_abi.DrGuidesDesc) == 24 and _abi.DrGuidesDesc.channels.offset == 4 and _abi.DR_GUIDES_MAX == 5
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    assert "DR_ABI_SIZE(DrGuidesDesc, 24);" in header and "#define DR_ABI_VERSION 9" in header and "#define DR_GUIDES_MAX 5" in header
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    assert "const int SIZEOF_DrGuidesDesc = 24;" in dart and "const int OFF_DrGuidesDesc_channels = 4;" in dart
    for sym in ("dr_render_guides_check", "dr_render_guides", "dr_render_guides_device"):
        assert "('%s')" % sym in dart, sym
    assert "renderWithGuides(Scene scene, List<int> channels)" in dart
