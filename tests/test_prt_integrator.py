"""DiffusePRTIntegrator on the host (no GPU): the host build of dr_sh.h against the Python restatement (tests/prt_restatement.py) bit for bit, the
restatement's harmonics against orthonormality, the class, what it marshals, the plugin and the refusals by name."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt, scenes

import prt_restatement as prt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMAX_MAX = 8  # dr_sh.h: DR_SH_LMAX_MAX


def _directions():
    """A few hundred unit directions as Vectors hold them (f32 components): random ones, the axes, +-z (the xyLen == 0 branch) and
    directions within 1e-7 of +-z."""
    rng = np.random.RandomState(7)
    v = rng.normal(size=(300, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    near = [(1.0e-7, 0.0, 1.0), (0.0, -1.0e-7, 1.0), (6.0e-8, 6.0e-8, -1.0), (-1.0e-7, 3.0e-8, -1.0), (1.0e-4, 0.0, 1.0), (3.0e-4, -2.0e-4, -1.0)]
    axes = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0)]
    return np.concatenate([v, np.array(near), np.array(axes)]).astype(np.float32).astype(np.float64)


def _device_header_evaluate(dirs, lmax):
    out = np.zeros((len(dirs), (lmax + 1) ** 2), np.float64)
    d = np.ascontiguousarray(dirs, np.float64)
    _abi.check(_abi.lib().dr_sh_evaluate(d.ctypes.data, len(d), lmax, out.ctypes.data))
    return out


@pytest.mark.parametrize("lmax", [1, 2, 4, LMAX_MAX])
def test_host_build_of_the_sh_header_equals_the_restatement_bit_for_bit(lmax):
    dirs = _directions()
    got, want = _device_header_evaluate(dirs, lmax), prt.EvaluateMany(dirs, lmax)
    assert got.shape == want.shape == (len(dirs), prt.Terms(lmax))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.isfinite(got).all() and np.abs(got[:, 0] - 0.5 * math.sqrt(1.0 / math.pi)).max() < 1e-15   # Y00
    # the vectorised restatement is the scalar one
    for k in (0, 17, 300, 303, 306):
        assert prt.Evaluate(prt.Vec(*dirs[k]), lmax) == [float(x) for x in want[k]]


def _gram(lmax, ntheta):
    """The Gram matrix of the restatement's harmonics by the midpoint rule over a lat-long grid of ntheta x 2 ntheta cells."""
    nphi = 2 * ntheta
    th = (np.arange(ntheta) + 0.5) * math.pi / ntheta
    ph = (np.arange(nphi) + 0.5) * 2.0 * math.pi / nphi
    T, P = np.meshgrid(th, ph, indexing="ij")
    w = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], axis=-1).reshape(-1, 3)
    Y = prt.EvaluateMany(w, lmax)
    dw = (np.sin(T) * (math.pi / ntheta) * (2.0 * math.pi / nphi)).reshape(-1, 1)
    return (Y * dw).T @ Y


def test_the_harmonics_are_orthonormal():
    """Integrated over a fine lat-long quadrature the harmonics give the identity.  The midpoint rule converges as 1 / n^2 in theta (it is
    exact in phi once 2 n exceeds 2 lmax), so the error at n = 128 is at most a third of the CHANGE between n = 64 and n = 128 (Richardson:
    e(64) = 4 e(128), so the change is 3 e(128)); the tolerance is that change itself, three times the expected error."""
    lmax = 4
    g64, g128 = _gram(lmax, 64), _gram(lmax, 128)
    # (the harmonics integrated are also the library's: the header's host build gives the same doubles on a sample of the grid)
    w = _directions()
    assert np.array_equal(_device_header_evaluate(w, lmax), prt.EvaluateMany(w, lmax))
    tol = np.abs(g128 - g64).max()
    err = np.abs(g128 - np.eye(prt.Terms(lmax))).max()
    print("orthonormality: |G - I| = %.3g at 128, change 64 -> 128 = %.3g" % (err, tol))
    assert 0.0 < tol < 1e-2 and err <= tol


def test_k_and_ringing_values():
    # K(l, 0) is what the header's harmonics are at +z, where P(l, 0) = 1 and every m != 0 term vanishes
    Y = _device_header_evaluate(np.array([[0.0, 0.0, 1.0]]), 4)[0]
    assert [Y[prt.Index(l, 0)] for l in range(5)] == [prt._K(l, 0) for l in range(5)] and np.count_nonzero(Y) == 5
    assert prt._K(0, 0) == math.sqrt(1.0 * prt.INV_FOURPI * 1.0) and prt._divfact(3, 2) == 1.0 / (2.0 * 3.0 * 4.0 * 5.0)
    c = [prt.RGB(1.0) for _ in range(prt.Terms(2))]
    prt.ReduceRinging(c, 2)
    assert c[0].tuple() == (1.0,) * 3 and c[2].r == prt.f32(1.0 / (1.0 + 0.005 * 4.0)) and c[6].r == prt.f32(1.0 / (1.0 + 0.005 * 36.0))


# ---- the class ----
def test_defaults_rounding_and_slots():
    a = core.DiffusePRTIntegrator.Create({})                       # diffuse_prt_integrator.dart:83-87
    assert (a.lmax, a.nSamples) == (4, 4096) and (core.DiffusePRTIntegrator().lmax, core.DiffusePRTIntegrator().nSamples) == (4, 4096)
    assert core.DiffusePRTIntegrator.Create({"nsamples": 5}).nSamples == 8 and core.DiffusePRTIntegrator.Create({"lmax": 2, "nsamples": 100}).nSamples == 128
    assert core.DiffusePRTIntegrator.kind == _abi.DR_INTEGRATOR_DIFFUSE_PRT == 7 and a.requestSamples(None, None) == ([], [])
    assert a.li_draws_recorded is False and a.maxDepth == 1
    assert prt.DiffusePRTIntegrator(4, 5).nSamples == 8
    make = core.Plugin.get("surfaceIntegrator", "diffuseprt")
    assert isinstance(make(), core.DiffusePRTIntegrator) and make({"lmax": 3}).lmax == 3
    cam = scenes.cornell_camera(8, 8)
    r = core.SamplerRenderer(None, cam, a, core.EmissionIntegrator())
    assert core.StratifiedSampler(cam, 2, 1, True, 5489).slot_counts(r, None) == ([1, 1], [])   # only the volume integrator's two
    assert _abi.lib().dr_sample_floats(_abi.DR_INTEGRATOR_DIFFUSE_PRT, 3) == 7
    # the value in between stays unassigned: it counts as DirectLighting "all", like every value the table does not know
    assert _abi.lib().dr_sample_floats(6, 3) == _abi.lib().dr_sample_floats(8, 3) == _abi.lib().dr_sample_floats(_abi.DR_INTEGRATOR_DIRECT_ALL, 3) == 25


@pytest.mark.parametrize("args,needle", [
    ((0,), "diffuse PRT: lmax must be at least 1"),
    ((-2,), "diffuse PRT: lmax must be at least 1"),
    ((LMAX_MAX + 1,), "diffuse PRT: lmax above 8"),
    ((4, 0), "diffuse PRT: nsamples must be at least 1"),
    ((4, 4097), "diffuse PRT: nsamples above 4096 after rounding"),
])
def test_refusals_by_name(args, needle):
    with pytest.raises(ValueError, match=needle):
        core.DiffusePRTIntegrator(*args)
    assert core.DiffusePRTIntegrator(LMAX_MAX, 4096).nSamples == 4096
    # the library's own text for lmax, without a device
    out = np.zeros(3 * 81, np.float64)
    d = np.array([[0.0, 0.0, 1.0]])
    for bad in (0, LMAX_MAX + 1):
        assert _abi.lib().dr_sh_evaluate(d.ctypes.data, 1, bad, out.ctypes.data) == -1
        assert "diffuse PRT: lmax" in _abi.lib().dr_last_error().decode()


def test_the_adaptive_sampler_is_refused_and_a_replay_names_its_seed():
    cam = scenes.cornell_camera(8, 8)
    mk = lambda s: core.SamplerRenderer(s, cam, core.DiffusePRTIntegrator(2, 16), core.EmissionIntegrator())
    with pytest.raises(ValueError, match="diffuse PRT: the adaptive sampler is not supported"):
        mk(core.AdaptiveSampler(cam, 2, 8, "contrast", 5489)).describe()
    vec = np.zeros((2, 7), np.float32)
    with pytest.raises(ValueError, match="give the HostBufferSampler the seed"):
        mk(core.HostBufferSampler(cam, 2, [(0, 0)], vec)).describe()
    d, keep = mk(core.HostBufferSampler(cam, 2, [(0, 0)], vec, seed=77)).describe()
    assert (d.seed, d.prt_nsamples, d.prt_lmax) == (77, 16, 2)


def test_descriptor_keeps_its_size_and_every_offset():
    cam = scenes.cornell_camera(8, 8)
    d, keep = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, core.DiffusePRTIntegrator(3, 100), core.EmissionIntegrator()).describe()
    assert (d.integrator, d.prt_nsamples, d.prt_lmax, d.max_depth) == (7, 128, 3, 1) and (d.tail, d.tail_offsets) == (None, None)
    D = _abi.DrRenderDesc
    assert C.sizeof(D) == 1352
    assert (D.sample_stride.offset, D.ao_nsamples.offset, D.prt_nsamples.offset, D.tail.offset, D.ao_mindist.offset) == (1320, 1324, 1324, 1328, 1328)
    assert (D.max_tail.offset, D.feature_channel.offset, D.prt_lmax.offset, D.tail_offsets.offset, D.ao_maxdist.offset) == (1336, 1340, 1340, 1344, 1344)
    assert (D.integrator.offset, D.strat_xsamples.offset, D.nsamples.offset) == (1248, 1292, 1296)
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    for line in ("#define DR_INTEGRATOR_DIFFUSE_PRT 7 ", "#define DR_ABI_VERSION 9", "DR_ABI_OFFSET(DrRenderDesc, prt_nsamples, 1324);",
                 "DR_ABI_OFFSET(DrRenderDesc, prt_lmax, 1340);", "DR_ABI_OFFSET(DrRenderDesc, ao_nsamples, 1324);",
                 "DR_ABI_OFFSET(DrRenderDesc, feature_channel, 1340);", "DR_ABI_SIZE(DrRenderDesc, 1352);"):
        assert line in header, line
    assert re.search(r"\bdr_prt_incident\s*\(", header) and "dr_prt_incident" in _abi.EXPORTS and "dr_sh_evaluate" in _abi.EXPORTS
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    assert "DR_INTEGRATOR_DIFFUSE_PRT = 7;" in dart and "const int OFF_DrRenderDesc_prt_nsamples = 1324;" in dart
    assert "const int OFF_DrRenderDesc_prt_lmax = 1340;" in dart and "'DiffusePRTIntegrator'" in dart
    # another integrator's descriptor leaves the two words alone
    d, keep = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, core.PathIntegrator(5), core.EmissionIntegrator()).describe()
    assert (d.prt_nsamples, d.prt_lmax) == (0, 0)


def test_the_loader_still_refuses_it():
    with pytest.raises(pbrt.UnsupportedFeature) as e:
        pbrt.loads('SurfaceIntegrator "diffuseprt"\nWorldBegin\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                   '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nWorldEnd\n')
    assert "diffuseprt" in str(e.value)
    assert core.Plugin.get("surfaceIntegrator", "diffuseprt") is not None   # (the integrator exists; only the front end's directive is refused)


# ---- the restatement's own known answers ----
def test_point_light_projection_is_the_harmonics_of_its_direction():
    light = prt.wr.PointLight((0.0, 2.0, 0.0), (8.0, 4.0, 2.0))
    c = prt.shProject_point(light, prt.Vec(0.0, 0.0, 0.0), 2)
    Y = prt.Evaluate(prt.Vec(0.0, 1.0, 0.0), 2)
    assert Y == [float(y) for y in _device_header_evaluate(np.array([[0.0, 1.0, 0.0]]), 2)[0]]
    assert [x.r for x in c] == [prt.f32(2.0 * y) for y in Y] and c[0].g == prt.f32(1.0 * Y[0])


def test_transfer_of_an_open_plane_is_the_clamped_cosine():
    """No occluder: c[0] estimates the integral of Y00 * cos over the hemisphere, Y00 * pi."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_restatement_fixtures as mrf
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([(-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1)], np.float32))
    scene = mrf.build_scene([core.GeometricPrimitive(mesh, core.MatteMaterial((0.5, 0.5, 0.5)), None)])
    c = prt.ComputeDiffuseTransfer(prt.Vec(0.0, 0.0, 0.0), prt.Vec(0.0, 1.0, 0.0), 1e-3, scene, prt.keyed_rng(5489, (0, 9, 0, 9))(3, 4, 0), 256, 2)
    assert abs(c[0].r - 0.5 * math.sqrt(1.0 / math.pi) * math.pi) < 0.02 and c[0].r == c[0].g == c[0].b
    # the library's own Y00, through the header's host build, is the constant the estimate was compared with
    assert abs(_device_header_evaluate(np.array([[0.6, 0.0, 0.8]]), 2)[0][0] - 0.5 * math.sqrt(1.0 / math.pi)) < 1e-15
