"""What the render planner derives from the integrator (kIntegratorTraits in dr_host.h), seen from outside: of two broken rules the same one
wins as ever, and every integrator runs its own number of stages and reports its own dr_scene_last_render_info word.  The Whitted test's box
(mirror, glass, an area light, a point light and a spot light).  Every call of the first test is refused: nothing is rendered there."""
import ctypes as C
import re

import numpy as np
import pytest

from dartray_amd import _abi, core

from test_gpu_whitted import SEED, Setup

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4  # DR_ERR_INVALID, DR_ERR_UNSUPPORTED (include/dartray_hip.h)
UNKNOWN = 99
LINE = re.compile(r"^stage_counts batch (\d+) stage (\d+): in (\d+) ", re.M)


@pytest.fixture(scope="module")
def box(gpu):
    return Setup()


def _camera(n):
    """The box's camera over an n x n film."""
    return core.PerspectiveCamera.lookAt((0.5, -1.0, -9.5), (0.0, -3.0, 2.0), (0.0, 1.0, 0.0), 70.0, core.ImageFilm(n, n, core.BoxFilter(0.5, 0.5)))


def test_of_two_broken_rules_the_same_one_wins(box):
    lib = _abi.lib()
    cam = _camera(4)
    film = np.zeros((4, 4, 4), np.float32)
    ld = lambda: core.LowDiscrepancySampler(cam, 2, SEED)
    adaptive = lambda: core.AdaptiveSampler(cam, 2, 8, "contrast", SEED)

    def refused(sampler, surface, code, needle, absent=None, camera_type=None, **fields):
        d, keep = core.SamplerRenderer(sampler, cam, surface, core.EmissionIntegrator()).describe()
        for name, value in fields.items():
            setattr(d, name, value)
        if camera_type is not None:
            d.camera.type = camera_type
        rc = lib.dr_render(box.scene._device().handle, C.byref(d), film.ctypes.data, None)
        msg = lib.dr_last_error().decode()
        assert rc == code, (rc, msg)
        assert needle in msg and (absent is None or absent not in msg), msg

    # the sampler's rules run in front of the integrator's ...
    refused(ld(), core.PathIntegrator(5), INVALID, "spp must be a power of two", absent="unknown integrator", integrator=UNKNOWN, spp=3)
    # ... but strat_xsamples is checked behind it
    refused(core.StratifiedSampler(cam, 2, 2, True, SEED), core.PathIntegrator(5), INVALID, "unknown integrator", absent="strat_xsamples",
            integrator=UNKNOWN, strat_xsamples=3)
    # the integrator's own max_depth rule in front of the general one, and in front of its refusal of the adaptive sampler
    refused(ld(), core.WhittedIntegrator(5), INVALID, "whitted integrator: max_depth must be at least 1", absent="out of range", max_depth=-1)
    refused(adaptive(), core.WhittedIntegrator(5), INVALID, "whitted integrator: max_depth must be at least 1", absent="adaptive", max_depth=0)
    # the adaptive refusal in front of the camera's
    refused(adaptive(), core.WhittedIntegrator(5), UNSUPPORTED, "whitted integrator: the adaptive sampler is not supported", absent="camera",
            camera_type=UNKNOWN)

    # ---- one pair per seam between the planner's units (dr_plan.hip): sampler, integrator in general, camera and film, the integrator's own
    # rules, the pixel source ----
    path = core.PathIntegrator(5)
    strat = lambda: core.StratifiedSampler(cam, 2, 2, True, SEED)  # (spp 4: strat_xsamples=3 does not divide it)
    ao, prt = lambda: core.AmbientOcclusionIntegrator(8), lambda: core.DiffusePRTIntegrator(2, 8)
    # the sampler kind's own rules in front of the integrator
    refused(core.HaltonSampler(cam, 4, SEED), path, UNSUPPORTED, "halton sampler: tile_count > 1", absent="unknown integrator", integrator=UNKNOWN,
            tile_count=2)
    refused(adaptive(), path, INVALID, "adaptive sampler: minSamples", absent="unknown integrator", integrator=UNKNOWN, strat_xsamples=3)
    # an unknown sampler mode is refused late, where the pixel source is chosen
    refused(ld(), path, INVALID, "unknown integrator", absent="sampler mode", integrator=UNKNOWN, sampler_mode=UNKNOWN)
    refused(ld(), path, INVALID, "unknown sampler mode", sampler_mode=UNKNOWN)
    # the integrator's general rules in front of the camera
    refused(ld(), path, INVALID, "max_depth out of range", absent="camera", max_depth=65, camera_type=UNKNOWN)
    # the camera in front of the integrator's own rules
    refused(ld(), ao(), INVALID, "unknown camera type", absent="nsamples must be at least 1", camera_type=UNKNOWN, ao_nsamples=0)
    refused(ld(), core.FeatureIntegrator("ng"), INVALID, "unknown camera type", absent="unknown channel", camera_type=UNKNOWN, feature_channel=UNKNOWN)
    refused(ld(), prt(), INVALID, "unknown camera type", absent="lmax must be at least 1", camera_type=UNKNOWN, prt_lmax=0)
    refused(ld(), core.MaterialIntegrator("albedo"), INVALID, "unknown camera type", absent="unknown channel", camera_type=UNKNOWN,
            material_channel=UNKNOWN)
    # the integrator's own rules in front of the pixel source
    refused(strat(), ao(), INVALID, "ambient occlusion integrator: nsamples must be at least 1", absent="strat_xsamples", strat_xsamples=3, ao_nsamples=0)
    refused(strat(), ao(), INVALID, "maxdist must be greater", absent="strat_xsamples", strat_xsamples=3, ao_maxdist=0.0)
    refused(strat(), prt(), UNSUPPORTED, "diffuse PRT: material", absent="strat_xsamples", strat_xsamples=3)  # (the box has a mirror and glass)
    refused(strat(), core.GlossyPRTIntegrator(lmax=2, nSamples=8), INVALID, "glossy PRT: lmax above 4", absent="strat_xsamples", strat_xsamples=3, prt_lmax=5)
    refused(strat(), core.UseProbesIntegrator(), INVALID, "use probes: no probe grid", absent="strat_xsamples", strat_xsamples=3)
    refused(strat(), core.MaterialIntegrator("albedo"), INVALID, "material integrator: unknown channel", absent="strat_xsamples", strat_xsamples=3,
            material_channel=UNKNOWN)
    # within an integrator: its parameters in front of the scene's materials
    refused(ld(), prt(), INVALID, "lmax must be at least 1", absent="material", prt_lmax=0)
    # the pixel source's own rules
    refused(strat(), path, INVALID, "strat_xsamples must be positive and divide spp", strat_xsamples=3)
    refused(ld(), path, INVALID, "host-buffer sampler: nsamples must be a positive multiple", sampler_mode=_abi.DR_SAMPLER_HOST_BUFFER, nsamples=0)
    assert not film.any()


@pytest.mark.parametrize("name", ["direct_all", "path", "direct_one", "whitted"])
def test_every_integrator_reports_its_word_and_runs_its_stages(box, name, capfd):
    """8 x 8 at 2 samples per pixel.  Three lights of nsamples 1: DirectLighting "all" runs a stage per light sample + 1, "one" its single
    stage + 1, Whitted a stage per light + 1, the path integrator maxDepth + 2 (DARTRAY_STAGE_COUNTS prints a line per stage and batch)."""
    assert len(box.scene.lights) == 3 and all(L.nSamples == 1 for L in box.scene.lights)
    integ, stages, word = {"direct_all": (core.DirectLightingIntegrator(0, 5), 3 + 1, -1),
                           "path": (core.PathIntegrator(5), 5 + 2, -1),
                           "direct_one": (core.DirectLightingIntegrator(1, 5), 1 + 1, -1),
                           "whitted": (core.WhittedIntegrator(5), 3 + 1, _abi.DR_INTEGRATOR_WHITTED | 0x100 | 0x200)}[name]
    r = core.SamplerRenderer(core.LowDiscrepancySampler(box.camera, 2, SEED), box.camera, integ, core.EmissionIntegrator())
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(b"STAGE_COUNTS", b"1"))
        capfd.readouterr()
        film = r.render(box.scene).film
        err = capfd.readouterr().err
    finally:
        _abi.check(lib.dr_set_option(b"STAGE_COUNTS", b""))
    assert np.isfinite(film).all() and film[..., :3].max() > 0.0
    arr = (C.c_int32 * 8)()
    _abi.check(lib.dr_scene_last_render_info(box.scene._device().handle, C.byref(arr)))
    assert int(arr[3]) == word, (name, int(arr[3]))
    info = box.scene._device().last_render_info()
    assert info["integrator"] == ("whitted" if name == "whitted" else None)
    assert info["shade_kernels"] == (["k_shade_whitted", "k_shade_spec"] if name == "whitted" else [])
    rows = [tuple(int(v) for v in m.groups()) for m in LINE.finditer(err)]
    assert info["batches"] == 1 and [(b, s) for b, s, _ in rows] == [(1, s) for s in range(stages)], (name, rows)
    assert rows[0][2] == 81 * 2  # the camera samples enter stage 0
