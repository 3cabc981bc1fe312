"""WhittedIntegrator on the host (no GPU): the class, what it marshals, the plugin, the loader's standing refusal, and the Python
restatement (tests/whitted_restatement.py) against values worked out by hand."""
import math
import os
import sys

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt, scenes

import whitted_restatement as wr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402


@pytest.fixture(autouse=True)
def host_builder(monkeypatch):
    monkeypatch.setenv("DARTRAY_BVH_BUILDER", "host")


def test_defaults():
    assert core.WhittedIntegrator().maxDepth == 5                  # whitted_integrator.dart:75
    assert core.WhittedIntegrator(3).maxDepth == 3
    assert core.WhittedIntegrator.Create().maxDepth == 5 and core.WhittedIntegrator.Create({"maxdepth": 2}).maxDepth == 2
    assert core.WhittedIntegrator.kind == _abi.DR_INTEGRATOR_WHITTED == 3


def test_descriptor_carries_the_integrator_and_max_depth():
    cam = scenes.cornell_camera(8, 8)
    r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, core.WhittedIntegrator(4), core.EmissionIntegrator())
    d, keep = r.describe()
    assert (d.integrator, d.max_depth, d.spp, d.sampler_mode) == (3, 4, 2, _abi.DR_SAMPLER_COUNTER)
    # no requestSamples: only the volume integrator's two 1-D slots
    assert core.StratifiedSampler(cam, 2, 1, True, 5489).slot_counts(r, None) == ([1, 1], [])


def test_plugin_creates_it_by_name():
    make = core.Plugin.get("surfaceIntegrator", "whitted")
    assert make is not None
    assert isinstance(make(), core.WhittedIntegrator) and make().maxDepth == 5
    assert make({"maxdepth": 7}).maxDepth == 7


def test_the_loader_still_refuses_it():
    with pytest.raises(pbrt.UnsupportedFeature) as e:
        pbrt.loads('SurfaceIntegrator "whitted"\nWorldBegin\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                   '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nWorldEnd\n')
    assert "SurfaceIntegrator" in str(e.value) and "whitted" in str(e.value)


class CountingRng:
    """Any values will do where the lights are delta lights or the answer does not depend on them; counts the draws."""

    def __init__(self):
        self.n = 0

    def randomFloat(self):
        self.n += 1
        return (0.137 * self.n) % 1.0


def _quad_y(y, half, material, light=None, up=True):
    """A quad in the plane Y = y; up: its normal is +Y (else -Y)."""
    h = half
    P = [(-h, y, -h), (-h, y, h), (h, y, h), (h, y, -h)] if up else [(-h, y, -h), (h, y, -h), (h, y, h), (-h, y, h)]
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array(P, np.float32))
    return core.GeometricPrimitive(mesh, material, light)


def test_matte_quad_under_a_point_light_at_normal_incidence():
    """Kd / pi * I / r^2: the light straight above the hit point, AbsDot(wi, n) = 1, pdf = 1, nothing in between."""
    Kd, I = (0.5, 0.4, 0.3), (8.0, 6.0, 4.0)
    scene = mrf.build_scene([_quad_y(0.0, 1.0, core.MatteMaterial(Kd))])
    scene.lights.append(wr.PointLight((0.5, 2.0, -0.25), I))
    ray = lambda: wr.Ray(wr.Vec(0.5, 1.0, -0.25), wr.Vec(0.0, -1.0, 0.0))  # (a fresh one per call: intersect shortens the ray it is given)
    for maxDepth, draws in ((1, 3), (5, 3 + 6)):                   # LightSample.random; + the two Specular* burns while depth + 1 < maxDepth
        rng = CountingRng()
        L = wr.RendererLi(scene, ray(), rng, maxDepth)
        assert L.tuple() == pytest.approx([k / math.pi * i / 4.0 for k, i in zip(Kd, I)], rel=1e-6)
        assert rng.n == draws
    # seen from below, wo and wi lie on opposite sides of the surface: BSDF.f evaluates the transmission lobes, and a matte surface has none
    up = wr.Ray(wr.Vec(0.5, -1.0, -0.25), wr.Vec(0.0, 1.0, 0.0))
    assert wr.RendererLi(scene, up, CountingRng(), 5).isBlack()


def test_mirror_facing_an_emitter():
    """The emitter's Le once at maxdepth 2 (Kr = 1, normal incidence: f * AbsDot / pdf = 1), nothing at maxdepth 1: a mirror has no
    lobe that f() evaluates, so its own light sample adds nothing."""
    Le = (5.0, 6.0, 7.0)
    prims = [_quad_y(0.0, 1.0, core.MirrorMaterial((1.0, 1.0, 1.0))),
             _quad_y(3.0, 4.0, core.MatteMaterial((0.5, 0.5, 0.5)), core.DiffuseAreaLight(Le, 1), up=False)]
    scene = mrf.build_scene(prims)
    assert len(scene.lights) == 1
    ray = lambda: wr.Ray(wr.Vec(0.3, 1.0, 0.2), wr.Vec(0.0, -1.0, 0.0))
    assert wr.RendererLi(scene, ray(), CountingRng(), 1).isBlack()
    rng = CountingRng()
    assert wr.RendererLi(scene, ray(), rng, 2).tuple() == pytest.approx(Le, rel=1e-6)
    assert rng.n == 3 + 3 + 3 + 3                                  # mirror: light, reflect burn; emitter vertex (depth 1): light; mirror: transmit burn
    # deeper: the emitter vertex now recurses too (two burns, no lobes) -- the same radiance, six draws more
    rng = CountingRng()
    assert wr.RendererLi(scene, ray(), rng, 5).tuple() == pytest.approx(Le, rel=1e-6)
    assert rng.n == 12 + 6


def test_keyed_rng_reads_the_li_stream_in_order():
    ext = (0, 9, 0, 9)
    a, b = wr.keyed_rng(5489, ext)(3, 4, 1), wr.rr.RNG(wr.rr.counter_key(5489, 4 * 9 + 3, 1, 2))
    assert [a.randomFloat() for _ in range(5)] == [b.randomFloat() for _ in range(5)]
    assert wr.keyed_rng(5489, ext)(3, 4, 0).randomFloat() != wr.keyed_rng(5489, ext)(3, 4, 1).randomFloat()


def test_a_host_buffer_replay_must_name_its_seed():
    """The draws inside Li are keyed by DrRenderDesc.seed, not by the buffers: a replay that forgets the seed is refused on the host."""
    cam = scenes.cornell_camera(8, 8)
    vec = np.zeros((2, 7), np.float32)
    mk = lambda **kw: core.SamplerRenderer(core.HostBufferSampler(cam, 2, [(0, 0)], vec, **kw), cam, core.WhittedIntegrator(2), core.EmissionIntegrator())
    with pytest.raises(ValueError, match="give the HostBufferSampler the seed"):
        mk().describe()
    assert mk(seed=77).describe()[0].seed == 77
    # every other integrator's replay is as before: no seed asked for, the field left alone
    r = core.SamplerRenderer(core.HostBufferSampler(cam, 2, [(0, 0)], np.zeros((2, 13), np.float32)), cam, core.DirectLightingIntegrator(0, 5), core.EmissionIntegrator())
    assert r.describe()[0].seed == 0


def test_the_restated_helpers_are_still_dr_kernels_own():
    """dr_shade_common.h restates helpers of dr_kernels.hip (whose hash the committed profiles pin) instead of moving them: every
    block of the header must still be found, word for word, in dr_kernels.hip, so the two cannot drift apart unseen."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dartray_amd", "csrc")
    header = open(os.path.join(csrc, "dr_shade_common.h")).read()
    kernels = open(os.path.join(csrc, "dr_kernels.hip")).read()
    body = header[header.index("#define DR_SHADE_COMMON_H") + len("#define DR_SHADE_COMMON_H"):header.rindex("#endif")]
    blocks = [b.strip() for b in body.split("\n\n") if b.strip()]
    assert len(blocks) == 3  # shade_count; the launch shape with the LDS tables; launch_shade with lightsInLds
    code = lambda text: "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("//"))  # (whole-line comments apart: one sits elsewhere there)
    for b in blocks:
        assert code(b) in code(kernels), b.splitlines()[0]
    for name in ("shade_count", "stage_lights", "light_table_bytes", "mat_table_bytes", "launch_shade", "lightsInLds", "DR_LDS_LIGHT_BYTES", "SHADE_WAVES_OF"):
        assert name in body
