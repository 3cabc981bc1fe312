"""The first-hit material integrator on the host (no GPU): the slot table through the real library, the class, the plugin,
what it marshals and where, its refusals by name, and the Python restatement (tests/material_restatement.py) against answers derived by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt, scenes

import feature_restatement as fe
import material_cases as mc
import material_restatement as me

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def host_builder(monkeypatch):
    monkeypatch.setenv("DARTRAY_BVH_BUILDER", "host")


def _renderer(sampler, cam, channel="albedo"):
    return core.SamplerRenderer(sampler, cam, core.MaterialIntegrator(channel), core.EmissionIntegrator())


# ---- the slot table, the class, the plugin ----
def test_the_c_table_and_the_python_class_count_the_same_slots():
    cam = scenes.cornell_camera(2, 2)
    r = _renderer(core.LowDiscrepancySampler(cam, 2, 5489), cam)
    assert core.MaterialIntegrator.kind == _abi.DR_INTEGRATOR_MATERIAL == 13
    for nlights in (0, 1, 3):
        scene = core.Scene(core.BVHAccel([scenes.floor_quad()]), [core.PointLight(None, (1.0 + i, 1.0, 1.0)) for i in range(nlights)])
        n1D, n2D = r.sampler.slot_counts(r, scene)
        assert _abi.lib().dr_sample_floats(13, nlights) == 5 + sum(n1D) + 2 * sum(n2D) == 7 and (n1D, n2D) == ([1, 1], [])
    # the value before it stays unassigned: counted as DirectLighting "all", like every unknown value
    assert _abi.lib().dr_sample_floats(12, 3) == _abi.lib().dr_sample_floats(14, 3) == 25


def test_plugin_creates_it_and_the_channels_map_to_the_constants():
    make = core.Plugin.get("surfaceIntegrator", "material")
    assert make is not None and isinstance(make(), core.MaterialIntegrator) and make().channel == "albedo"
    want = {"albedo": _abi.DR_MATERIAL_CHANNEL_ALBEDO, "emission": _abi.DR_MATERIAL_CHANNEL_EMISSION}
    assert want == {"albedo": 0, "emission": 1} == me.CHANNELS == core.MaterialIntegrator.CHANNELS
    cam = scenes.cornell_camera(4, 4)
    for name, const in want.items():
        integ = make({"channel": name})
        assert integ.channel == name and integ.li_draws_recorded is False and integ.requestSamples(None, None) == ([], [])
        d, keep = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, integ, core.EmissionIntegrator()).describe()
        assert (d.integrator, d.material_channel, d.max_depth) == (13, const, 0)
    for bad in ("ng", "Albedo", "roughness", ""):
        with pytest.raises(ValueError) as e:
            make({"channel": bad})
        assert str(e.value).startswith("material integrator: channel must be one of albedo, emission")


def test_the_adaptive_sampler_is_refused_and_a_replay_needs_no_seed():
    cam = scenes.cornell_camera(8, 8)
    with pytest.raises(ValueError) as e:
        _renderer(core.AdaptiveSampler(cam, 2, 8, "contrast", 5489), cam).describe()
    assert str(e.value) == "material integrator: the adaptive sampler is not supported"
    d, keep = _renderer(core.HostBufferSampler(cam, 2, [(0, 0)], np.zeros((2, 7), np.float32)), cam, "emission").describe()
    assert (d.integrator, d.material_channel, d.sampler_mode, d.tail) == (13, 1, _abi.DR_SAMPLER_HOST_BUFFER, None)


def test_dr_material_check_answers_without_a_device():
    lib = _abi.lib()
    assert lib.dr_material_check(0) == 0 and lib.dr_material_check(1) == 0
    for ch in (-1, 2, 99):
        assert lib.dr_material_check(ch) == -1
        assert "material integrator: unknown channel (DR_MATERIAL_CHANNEL_ALBEDO or _EMISSION)" in lib.dr_last_error().decode()


def test_a_guide_render_refuses_it_by_name():
    cam = scenes.cornell_camera(4, 4)
    d, keep = _renderer(core.LowDiscrepancySampler(cam, 2, 5489), cam).describe()
    g = _abi.DrGuidesDesc()
    g.count, g.channels[0] = 1, _abi.DR_FEATURE_DEPTH
    assert _abi.lib().dr_render_guides_check(C.byref(d), C.byref(g), 10) == -4
    assert "render guides: the material integrator is not supported" in _abi.lib().dr_last_error().decode()


# ---- the ABI ----
def test_the_channel_shares_the_feature_channels_word_and_nothing_moved():
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    off = int(re.search(r"^DR_ABI_OFFSET\(DrRenderDesc, material_channel, (\d+)\);", header, flags=re.M).group(1))
    D = _abi.DrRenderDesc
    assert off == D.material_channel.offset == D.feature_channel.offset == 1340 and C.sizeof(D) == 1352
    assert "#define DR_INTEGRATOR_MATERIAL 13" in header and "#define DR_ABI_VERSION 9" in header and _abi.DR_ABI_VERSION == 9
    assert re.search(r"^#define DR_MATERIAL_CHANNEL_ALBEDO 0\b", header, flags=re.M) and re.search(r"^#define DR_MATERIAL_CHANNEL_EMISSION 1\b", header, flags=re.M)
    cam = scenes.cornell_camera(4, 4)
    d, keep = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, core.PathIntegrator(5), core.EmissionIntegrator()).describe()
    assert d.material_channel == 0
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    assert "const int OFF_DrRenderDesc_material_channel = 1340;" in dart and "const int DR_INTEGRATOR_MATERIAL = 13;" in dart
    assert "DR_MATERIAL_CHANNEL_ALBEDO = 0, DR_MATERIAL_CHANNEL_EMISSION = 1" in dart
    assert "class MaterialIntegrator extends SurfaceIntegrator" in dart and "rd.i32(OFF_DrRenderDesc_material_channel, mat.channel);" in dart
    for sym in ("dr_material_check", "dr_demodulate_check", "dr_demodulate_host", "dr_demodulate", "dr_demodulate_device", "dr_remodulate_host",
                "dr_remodulate", "dr_remodulate_device"):
        assert "'%s'" % sym in dart and sym in _abi.EXPORTS and re.search(r"^int %s\(" % sym, header, flags=re.M), sym


def test_the_loader_still_refuses_it():
    with pytest.raises(pbrt.UnsupportedFeature) as e:
        pbrt.loads('SurfaceIntegrator "material"\nWorldBegin\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                   '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nWorldEnd\n')
    assert "SurfaceIntegrator" in str(e.value) and "material" in str(e.value)


# ---- the restatement's known answers ----
def _ortho(res=4):
    """tests/test_feature_integrator.py's camera: at the origin looking down -z over the window [-1, 1]^2, every entry a dyadic rational."""
    s = 2.0 / res
    r2c = [s, 0.0, 0.0, -1.0, 0.0, -s, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    c2w = [-1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    return fe.OrthographicCamera(r2c, c2w)


def _unit_quad(ccw_from_camera, material, light=None):
    """The unit quad [-1/2, 1/2]^2 in the plane z = -2.  Listed counter-clockwise as the camera sees it its geometric normal is (0, 0, 1),
    towards the camera; listed clockwise (0, 0, -1) (tests/test_feature_integrator.py derives both)."""
    P = [(-0.5, -0.5, -2.0), (0.5, -0.5, -2.0), (0.5, 0.5, -2.0), (-0.5, 0.5, -2.0)]
    return mc.mesh(P if ccw_from_camera else P[::-1], material, light=light)


PIXELS = [(1, 1), (2, 1), (1, 2), (2, 2)]                           # the four centre pixels: |x|, |y| < 1/2
VEC = np.array([[0.25, 0.25, 0, 0, 0, 0, 0], [0.75, 0.5, 0, 0, 0, 0, 0]] * 4, np.float32)
BOX = [1.0] * 256


def _render(prims, lights, channel, pixels=PIXELS):
    acc = core.BVHAccel(prims)
    scene = mc.restated(acc, acc.lights() + list(lights))
    return me.render(scene, me.CHANNELS[channel], _ortho(4), 4, 4, 0.5, 0.5, BOX, 2, pixels, VEC[:2 * len(pixels)])


def test_a_grey_quad_gives_its_kd_and_no_emission():
    prims = [_unit_quad(True, core.MatteMaterial((0.5, 0.25, 0.125)))]
    Ls, hit, film, rgb = _render(prims, [], "albedo")
    assert hit.all() and (Ls == np.array((0.5, 0.25, 0.125), np.float32)).all() and (film[1:3, 1:3, 3] == 2.0).all()
    Ls, hit, film, rgb = _render(prims, [], "emission")
    assert hit.all() and (Ls == 0.0).all()
    # a negative colour is clamped as getBSDF clamps it; mirror and glass give Kr, plastic Kd
    for material, want in ((core.MatteMaterial((-1.0, 0.5, 2.0)), (0.0, 0.5, 2.0)), (core.MirrorMaterial((0.9, 0.8, 0.7)), (0.9, 0.8, 0.7)),
                           (core.GlassMaterial((0.6, 0.5, 0.4), (0.1, 0.1, 0.1)), (0.6, 0.5, 0.4)),
                           (core.PlasticMaterial((0.3, 0.2, 0.1), (0.9, 0.9, 0.9), 0.1), (0.3, 0.2, 0.1))):
        Ls = _render([_unit_quad(True, material)], [], "albedo")[0]
        assert (Ls == np.array(want, np.float32)).all(), (type(material).__name__, Ls)


@pytest.mark.parametrize("ccw,seen", [(True, True), (False, False)])
def test_an_emitter_quad_from_the_front_and_from_behind(ccw, seen):
    """wo = -ray.d = (0, 0, 1).  Listed counter-clockwise nn = (0, 0, 1): Dot(nn, wo) = 1 > 0, Lemit; clockwise nn = (0, 0, -1): 0."""
    L = (36.0, 30.0, 24.0)
    prims = [_unit_quad(ccw, core.MatteMaterial((0.5, 0.5, 0.5)), core.DiffuseAreaLight(L, 1))]
    Ls, hit, film, rgb = _render(prims, [], "emission")
    assert hit.all() and (Ls == np.array(L if seen else (0.0, 0.0, 0.0), np.float32)).all()
    # reverseOrientation turns the normal and with it the lit side (DifferentialGeometry.set)
    P = [(-0.5, -0.5, -2.0), (0.5, -0.5, -2.0), (0.5, 0.5, -2.0), (-0.5, 0.5, -2.0)]
    rev = mc.mesh(P if ccw else P[::-1], core.MatteMaterial((0.5, 0.5, 0.5)), light=core.DiffuseAreaLight(L, 1), reverseOrientation=True)
    Ls = _render([rev], [], "emission")[0]
    assert (Ls == np.array((0.0, 0.0, 0.0) if seen else L, np.float32)).all()
    # the albedo of an emitter is its own material's colour
    assert (_render(prims, [], "albedo")[0] == 0.5).all()


def test_a_disk_emitter_gives_its_lemit_where_hit():
    """A disk of radius 3/4 in the plane z = -2 whose object-space +z -- its normal -- is the world's: it faces the camera at the origin.  The
    samples of the four centre pixels lie at |x|, |y| <= 3/8, at most sqrt(9/32) < 3/4 from the axis: inside; the corner pixel (0, 0) samples
    (-7/8, 7/8) and (-5/8, 3/4), both farther than 3/4: misses."""
    at = pbrt.Transform.Translate(0.0, 0.0, -2.0)
    L = (2.0, 7.0, 1.0)
    disk = core.GeometricPrimitive(core.Disk(at.m, at.mInv, False, 0.0, 0.75, 0.0), core.MatteMaterial((0.5, 0.5, 0.5)), core.DiffuseAreaLight(L, 1))
    Ls, hit, film, rgb = _render([disk], [], "emission")
    assert hit.all() and (Ls == np.array(L, np.float32)).all()
    Ls, hit, film, rgb = _render([disk], [], "emission", [(0, 0)])
    assert not hit.any() and (Ls == 0.0).all() and film[0, 0, 3] == 2.0
    flipped = core.GeometricPrimitive(core.Disk(at.m, at.mInv, True, 0.0, 0.75, 0.0), core.MatteMaterial((0.5, 0.5, 0.5)), core.DiffuseAreaLight(L, 1))
    assert (_render([flipped], [], "emission")[0] == 0.0).all()


def test_a_miss_gives_the_infinite_lights_radiance_or_black():
    """The 1 x 1 white map of an infinite light without a file: Le(ray) = 1 * L whatever the direction."""
    prims = [_unit_quad(True, core.MatteMaterial((0.5, 0.5, 0.5)))]
    env = core.InfiniteAreaLight(None, (0.25, 0.5, 2.0), 1, None)
    Ls, hit, film, rgb = _render(prims, [env], "emission", [(0, 0), (3, 3)])
    assert not hit.any() and (Ls == np.array((0.25, 0.5, 2.0), np.float32)).all()
    Ls, hit, film, rgb = _render(prims, [], "emission", [(0, 0), (3, 3)])
    assert not hit.any() and (Ls == 0.0).all()
    Ls, hit, film, rgb = _render(prims, [env], "albedo", [(0, 0), (3, 3)])
    assert not hit.any() and (Ls == 0.0).all()
    # at a hit the infinite light adds nothing: isect.Le is the primitive's own area light's
    Ls, hit, film, rgb = _render(prims, [env], "emission")
    assert hit.all() and (Ls == 0.0).all()
