"""The integrators' sample slots, stated once on each side of the C ABI: kIntegratorTraits (dr_host.h, read through dr_sample_floats) and the
Python classes' requestSamples (core/renderer.py, read through sampler.slot_counts) must agree; and which integrator's Li draws from the
serial stream that serial_samples replays.  No GPU: the library loads without a device."""
import pytest

from dartray_amd import _abi, core, scenes

INTEGRATORS = {
    "path": lambda: core.PathIntegrator(5),
    "direct_all": lambda: core.DirectLightingIntegrator(core.DirectLightingIntegrator.SAMPLE_ALL_UNIFORM, 5),
    "direct_one": lambda: core.DirectLightingIntegrator(core.DirectLightingIntegrator.SAMPLE_ONE_UNIFORM, 5),
    "whitted": lambda: core.WhittedIntegrator(5),
}
SAMPLERS = {
    "stratified": lambda cam: core.StratifiedSampler(cam, 2, 1, True, 5489),
    "halton": lambda cam: core.HaltonSampler(cam, 2, 5489),
    "random": lambda cam: core.RandomSampler(cam, 2, 5489),
}
LI_DRAWS_TEXT = "serial_samples: a PathIntegrator with maxDepth >= 3 draws inside Li; pass li_draws"


@pytest.fixture(autouse=True)
def host_builder(monkeypatch):
    monkeypatch.setenv("DARTRAY_BVH_BUILDER", "host")


def _scene(nlights):
    """The floor quad under nlights point lights (nsamples 1 each)."""
    accel = core.BVHAccel([scenes.floor_quad()])
    return core.Scene(accel, [core.PointLight(None, (1.0 + i, 1.0, 1.0)) for i in range(nlights)])


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("integrator", sorted(INTEGRATORS))
def test_the_c_table_and_the_python_classes_count_the_same_slots(integrator, sampler):
    cam = scenes.cornell_camera(2, 2)
    integ = INTEGRATORS[integrator]()
    r = core.SamplerRenderer(SAMPLERS[sampler](cam), cam, integ, core.EmissionIntegrator())
    for nlights in (0, 1, 3):
        scene = _scene(nlights)
        assert all(L.nSamples == 1 for L in scene.lights) and len(scene.lights) == nlights
        n1D, n2D = r.sampler.slot_counts(r, scene)
        got = _abi.lib().dr_sample_floats(integ.kind, nlights)
        assert got == 5 + sum(n1D) + 2 * sum(n2D), (integrator, sampler, nlights, n1D, n2D)
        if integrator == "path":
            assert got == 37
        if integrator == "whitted":
            assert got == 7
        # the volume integrator's tau + scatter close the 1-D slots of every integrator
        assert n1D[-2:] == [1, 1]


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
def test_serial_samples_asks_for_li_draws_exactly_where_li_draws_from_the_stream(sampler):
    cam = scenes.cornell_camera(2, 2)
    scene = _scene(1)
    cases = [(core.PathIntegrator(d), d >= 3) for d in (0, 2, 3, 5)] + [(mk(), False) for name, mk in sorted(INTEGRATORS.items()) if name != "path"]
    for integ, needs in cases:
        r = core.SamplerRenderer(SAMPLERS[sampler](cam), cam, integ, core.EmissionIntegrator())
        if needs:
            with pytest.raises(ValueError) as e:
                r.sampler.serial_samples(r, scene)
            assert str(e.value) == LI_DRAWS_TEXT
            hb = r.sampler.serial_samples(r, scene, li_draws=lambda px, py, v, rng: [rng.randomFloat()])
            assert hb.tail is not None and hb.tail_offsets is not None and len(hb.tail) == len(hb.sample_vec)
        else:
            hb = r.sampler.serial_samples(r, scene)
            assert hb.tail is None
        assert isinstance(hb, core.HostBufferSampler) and len(hb.sample_vec) == len(hb.pixel_xy) * hb.samplesPerPixel > 0
        assert hb.sample_vec.shape[1] == _abi.lib().dr_sample_floats(integ.kind, 1)
