"""AmbientOcclusionIntegrator on the host (no GPU): the class, what it marshals, the plugin, its refusals by name, the loader's standing
refusal, and the Python restatement (tests/ao_restatement.py) against answers known without computing anything."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt, scenes

import ao_restatement as ao

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def host_builder(monkeypatch):
    monkeypatch.setenv("DARTRAY_BVH_BUILDER", "host")


# ---- the class ----
def test_defaults_and_rounding():
    a = core.AmbientOcclusionIntegrator()                          # ambient_occlusion_integrator.dart:55-60
    assert (a.nSamples, a.minDist, a.maxDist) == (2048, 1.0e-4, math.inf)
    assert core.AmbientOcclusionIntegrator(5).nSamples == 8        # :25  RoundUpPow2
    assert [core.AmbientOcclusionIntegrator(n).nSamples for n in (1, 2, 3, 128, 129, 4096)] == [1, 2, 4, 128, 256, 4096]
    c = core.AmbientOcclusionIntegrator.Create({"nsamples": 100, "mindist": 0.5, "maxdist": 3.0})
    assert (c.nSamples, c.minDist, c.maxDist) == (128, 0.5, 3.0)
    assert core.AmbientOcclusionIntegrator.kind == _abi.DR_INTEGRATOR_AO == 4
    assert ao.AmbientOcclusionIntegrator(5).nSamples == 8 and ao.AmbientOcclusionIntegrator().nSamples == 2048


def test_plugin_creates_it_by_the_references_name():
    make = core.Plugin.get("surfaceIntegrator", "ambientocclusion")   # render_manager_interface.dart:61-62
    assert make is not None
    a = make()
    assert isinstance(a, core.AmbientOcclusionIntegrator) and (a.nSamples, a.minDist, a.maxDist) == (2048, 1.0e-4, math.inf)
    assert make({"nsamples": 5}).nSamples == 8


@pytest.mark.parametrize("args,needle", [
    ((0,), "ambient occlusion integrator: nsamples must be at least 1"),
    ((-3,), "ambient occlusion integrator: nsamples must be at least 1"),
    ((4097,), "ambient occlusion integrator: nsamples above 4096 after rounding"),
    ((8, -1.0e-3), "ambient occlusion integrator: mindist must not be negative"),
    ((8, 1.0, 1.0), "ambient occlusion integrator: maxdist must be greater than mindist"),
    ((8, 1.0, 0.5), "ambient occlusion integrator: maxdist must be greater than mindist"),
    ((8, 0.0, math.nan), "ambient occlusion integrator: maxdist must be greater than mindist"),
])
def test_refusals_by_name(args, needle):
    with pytest.raises(ValueError, match=needle):
        core.AmbientOcclusionIntegrator(*args)


def _renderer(sampler, cam, integ=None):
    return core.SamplerRenderer(sampler, cam, integ or core.AmbientOcclusionIntegrator(16, 0.25, 7.5), core.EmissionIntegrator())


def test_descriptor_carries_the_three_parameters_and_moves_nothing():
    cam = scenes.cornell_camera(8, 8)
    d, keep = _renderer(core.LowDiscrepancySampler(cam, 2, 5489), cam).describe()
    assert (d.integrator, d.spp, d.sampler_mode, d.seed) == (4, 2, _abi.DR_SAMPLER_COUNTER, 5489)
    assert (d.ao_nsamples, d.ao_mindist, d.ao_maxdist) == (16, 0.25, 7.5)
    D = _abi.DrRenderDesc
    assert C.sizeof(D) == 1352 and (D.sample_stride.offset, D.ao_nsamples.offset, D.max_tail.offset) == (1320, 1324, 1336)
    assert D.tail.offset == D.ao_mindist.offset == 1328 and D.tail_offsets.offset == D.ao_maxdist.offset == 1344
    # the default maxdist: infinity crosses as a double
    d, keep = _renderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, core.AmbientOcclusionIntegrator(4)).describe()
    assert d.ao_maxdist == math.inf and d.ao_mindist == 1.0e-4
    # no requestSamples: only the volume integrator's two 1-D slots, as dr_sample_floats says
    assert core.StratifiedSampler(cam, 2, 1, True, 5489).slot_counts(_renderer(None, cam), None) == ([1, 1], [])
    assert _abi.lib().dr_sample_floats(_abi.DR_INTEGRATOR_AO, 3) == 7
    # every other integrator's descriptor: the tail fields are the tail's, the new word stays zero
    r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, core.PathIntegrator(5), core.EmissionIntegrator())
    d, keep = r.describe()
    assert (d.ao_nsamples, d.tail, d.tail_offsets) == (0, None, None)


def test_header_python_and_dart_agree():
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    assert "#define DR_INTEGRATOR_AO 4" in header and "#define DR_ABI_VERSION 9" in header and _abi.DR_ABI_VERSION == 9
    for line in ("DR_ABI_OFFSET(DrRenderDesc, ao_nsamples, 1324);", "DR_ABI_OFFSET(DrRenderDesc, ao_mindist, 1328);",
                 "DR_ABI_OFFSET(DrRenderDesc, ao_maxdist, 1344);", "DR_ABI_SIZE(DrRenderDesc, 1352);"):
        assert line in header
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    assert "DR_INTEGRATOR_AO = 4" in dart and "'AmbientOcclusionIntegrator'" in dart
    for name, off in (("ao_nsamples", 1324), ("ao_mindist", 1328), ("ao_maxdist", 1344)):
        assert "const int OFF_DrRenderDesc_%s = %d;" % (name, off) in dart


def test_a_host_buffer_replay_must_name_its_seed_and_the_adaptive_sampler_is_refused():
    cam = scenes.cornell_camera(8, 8)
    vec = np.zeros((2, 7), np.float32)
    with pytest.raises(ValueError, match="give the HostBufferSampler the seed"):
        _renderer(core.HostBufferSampler(cam, 2, [(0, 0)], vec), cam).describe()
    d, keep = _renderer(core.HostBufferSampler(cam, 2, [(0, 0)], vec, seed=77), cam).describe()
    assert d.seed == 77 and (d.ao_nsamples, d.ao_mindist, d.ao_maxdist) == (16, 0.25, 7.5)
    with pytest.raises(ValueError, match="ambient occlusion integrator: the adaptive sampler is not supported"):
        _renderer(core.AdaptiveSampler(cam, 2, 8, "contrast", 5489), cam).describe()
    assert core.AmbientOcclusionIntegrator.li_draws_recorded is False


def test_the_loader_still_refuses_it():
    with pytest.raises(pbrt.UnsupportedFeature) as e:
        pbrt.loads('SurfaceIntegrator "ambientocclusion"\nWorldBegin\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                   '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nWorldEnd\n')
    assert "SurfaceIntegrator" in str(e.value) and "ambientocclusion" in str(e.value)


# ---- the restatement's known answers ----
def _quad_y(y, half, up=True):
    """A matte quad in the plane Y = y; up: its normal is +Y (else -Y)."""
    h = half
    P = [(-h, y, -h), (-h, y, h), (h, y, h), (h, y, -h)] if up else [(-h, y, -h), (h, y, -h), (h, y, h), (-h, y, h)]
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array(P, np.float32))
    return core.GeometricPrimitive(mesh, core.MatteMaterial((0.5, 0.5, 0.5)), None)


def _stream(i=0):
    return ao.keyed_rng(5489, (0, 9, 0, 9))(3, 4, i)


@pytest.mark.parametrize("ns", [1, 2, 8, 64, 256])
def test_a_lone_quad_sees_the_whole_sky(ns):
    """Nothing but the quad itself, whose plane no ray of the upper hemisphere can reach again: every ray is clear, whatever the scramble."""
    scene = mrf.build_scene([_quad_y(0.0, 1.0)])
    integ = ao.AmbientOcclusionIntegrator(ns)
    for k, (x, z) in enumerate([(0.3, 0.2), (-0.7, 0.55)]):
        L = ao.RendererLi(scene, integ, ao.Ray(ao.Vec(x, 1.0, z), ao.Vec(0.0, -1.0, 0.0)), _stream(k))
        assert L.tuple() == (1.0, 1.0, 1.0)
    # seen from below the normal is flipped towards the camera ray (FaceForward): the lower hemisphere, clear as well
    L = ao.RendererLi(scene, integ, ao.Ray(ao.Vec(0.3, -1.0, 0.2), ao.Vec(0.0, 1.0, 0.0)), _stream())
    assert L.tuple() == (1.0, 1.0, 1.0)


def _box_scene():
    """A closed box of six quads around the origin, half side 2."""
    s = 2.0
    q = lambda a, b, c, d: core.GeometricPrimitive(core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([a, b, c, d], np.float32)),
                                                    core.MatteMaterial((0.5, 0.5, 0.5)), None)
    return mrf.build_scene([
        q((-s, -s, -s), (-s, -s, s), (s, -s, s), (s, -s, -s)), q((-s, s, -s), (s, s, -s), (s, s, s), (-s, s, s)),      # floor, ceiling
        q((-s, -s, -s), (-s, s, -s), (-s, s, s), (-s, -s, s)), q((s, -s, -s), (s, -s, s), (s, s, s), (s, s, -s)),      # left, right
        q((-s, -s, s), (-s, s, s), (s, s, s), (s, -s, s)), q((-s, -s, -s), (s, -s, -s), (s, s, -s), (-s, s, -s))])     # back, front


@pytest.mark.parametrize("ns", [1, 8, 256])
def test_inside_a_closed_box(ns):
    """From a point of the floor every ray of the hemisphere ends on a wall or the ceiling: 0 with an infinite maxdist.  With a maxdist
    shorter than the nearest wall (the hit is 0.75 from the nearest side wall) no ray reaches anything: 1."""
    scene = _box_scene()
    ray = lambda: ao.Ray(ao.Vec(0.25, 0.0, -1.25), ao.Vec(0.0, -1.0, 0.0))   # hits the floor at (0.25, -2, -1.25)
    assert ao.RendererLi(scene, ao.AmbientOcclusionIntegrator(ns), ray(), _stream()).tuple() == (0.0, 0.0, 0.0)
    assert ao.RendererLi(scene, ao.AmbientOcclusionIntegrator(ns, 1.0e-4, 0.5), ray(), _stream()).tuple() == (1.0, 1.0, 1.0)


def test_a_roof_over_half_the_sky_counts_in_steps_of_one_ray():
    """An occluder quad over the hit point: the answer is k / nSamples for an integer k strictly between the two ends, and it depends on the
    scramble, that is on the stream."""
    roof = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([(0.0, 1.0, -50.0), (50.0, 1.0, -50.0), (50.0, 1.0, 50.0), (0.0, 1.0, 50.0)], np.float32))
    scene = mrf.build_scene([_quad_y(0.0, 1.0), core.GeometricPrimitive(roof, core.MatteMaterial((0.5, 0.5, 0.5)), None)])
    ray = lambda: ao.Ray(ao.Vec(0.0, 0.5, 0.3), ao.Vec(0.0, -1.0, 0.0))
    vals = [ao.RendererLi(scene, ao.AmbientOcclusionIntegrator(64), ray(), _stream(i)).tuple()[0] for i in range(4)]
    for v in vals:
        assert 0.25 < v < 0.75 and v * 64 == int(v * 64)           # (half the hemisphere is under the roof)
    assert len(set(vals)) > 1
    # a mindist past everything the rays can reach: all clear
    assert ao.RendererLi(scene, ao.AmbientOcclusionIntegrator(64, 1.0e3, math.inf), ray(), _stream()).tuple() == (1.0, 1.0, 1.0)


def test_an_escaped_camera_ray_takes_the_lights_le():
    scene = mrf.build_scene([_quad_y(0.0, 1.0)])
    assert ao.RendererLi(scene, ao.AmbientOcclusionIntegrator(8), ao.Ray(ao.Vec(5.0, 1.0, 0.0), ao.Vec(0.0, -1.0, 0.0)), _stream()).isBlack()


# ---- the draws ----
def test_keyed_rng_is_the_li_stream_and_draws_two_words():
    a, b = _stream(1), ao.rr.RNG(ao.rr.counter_key(5489, 4 * 9 + 3, 1, 2))
    assert [a.randomFloat() for _ in range(5)] == [b.randomFloat() for _ in range(5)]   # one generator, two restatements

    class Counting:
        def __init__(self, rng):
            self.rng, self.n = rng, 0

        def randomUint(self):
            self.n += 1
            return self.rng.randomUint()
    rng = Counting(_stream())
    scene = mrf.build_scene([_quad_y(0.0, 1.0)])
    ao.RendererLi(scene, ao.AmbientOcclusionIntegrator(8), ao.Ray(ao.Vec(0.3, 1.0, 0.2), ao.Vec(0.0, -1.0, 0.0)), rng)
    assert rng.n == 2


# ---- one definition each on the device ----
def test_the_sphere_sampling_lines_are_still_dr_devices_own():
    """dr_li_sampling.h states UniformSampleSphere as a function; dr_device.h, whose hash the committed profiles pin, has the same lines
    inline in sphere_sample.  Every line of the function's body must be found there word for word, so the two cannot drift apart unseen."""
    csrc = os.path.join(ROOT, "dartray_amd", "csrc")
    header = open(os.path.join(csrc, "dr_li_sampling.h")).read()
    device = open(os.path.join(csrc, "dr_device.h")).read()
    body = header[header.index("DR_DEV F3 UniformSampleSphere("):]
    body = body[body.index("\n") + 1:body.index("\n}")].splitlines()
    assert len(body) == 4
    for line in body[:3]:
        assert line.split("//")[0].rstrip() in device, line
    assert "f3(r * cos(phi), r * sin(phi), z)" in body[3] and "f3(r * cos(phi), r * sin(phi), z)" in device
    # the radical inverses and the in-Li stream exist once outside dr_kernels.hip: in the header, used by the units that had them
    for name, users in (("scrambled_radical", ("dr_sampler_strat.hip", "dr_shade_ao.hip")), ("li_stream", ("dr_shade_whitted.hip", "dr_shade_ao.hip"))):
        assert header.count("DR_DEV") >= 4 and name in header
        for u in users:
            text = open(os.path.join(csrc, u)).read()
            assert '#include "dr_li_sampling.h"' in text and ("DR_DEV float " + name) not in text and ("DR_DEV DartRandom " + name) not in text
    assert "Sample02" in open(os.path.join(csrc, "dr_shade_ao.hip")).read()
