"""GlossyPRTIntegrator on the host (no GPU): the host builds of dr_sh_glossy.h -- the reference's Rotate, object sharing included, and its
ComputeBSDFMatrix -- against the Python restatement (tests/glossy_prt_restatement.py) bit for bit; RotateZ and RotateXPlus as rotations; a known
answer for the BSDF matrix; the class, the constants, the plugin, the refusals by name."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt, scenes

import glossy_prt_restatement as gp
import prt_restatement as prt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB = gp.RGB


def frames():
    """64 shading frames as Matrix4x4.values(r1.x, r2.x, nl.x, 0, r1.y, ...) holds them (f32): 58 random orthonormal ones, the normal at +z and
    -z (the sy <= 16 * FLT_EPSILON branch of _toZYZ), two of them turned about z, a normal within 1e-6 of +z, and frames of negative handedness."""
    rng = np.random.RandomState(11)
    out = []
    for k in range(58):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if k % 5 == 4:
            q[:, 1] = -q[:, 1]                                     # negative handedness
        out.append(q)
    c, s = math.cos(0.7), math.sin(0.7)
    out += [np.eye(3), np.diag([1.0, -1.0, -1.0]), np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]), np.array([[c, s, 0], [s, -c, 0], [0, 0, -1.0]]),
            np.array([[1.0, 0, 1e-6], [0, 1.0, 0], [-1e-6, 0, 1.0]]), np.diag([1.0, 1.0, -1.0])]
    m = np.zeros((len(out), 16), np.float32)
    for k, q in enumerate(out):
        m[k, [0, 1, 2]], m[k, [4, 5, 6]], m[k, [8, 9, 10]], m[k, 15] = q[0], q[1], q[2], 1.0
    assert len(m) == 64
    return m


def coefficients(lmax, seed=3):
    return np.random.RandomState(seed + lmax).uniform(-1.0, 1.0, size=(64, prt.Terms(lmax), 3)).astype(np.float32)


def restated_rotate(c, m16, lmax, fresh=False, angles=None):
    c_in = [RGB(*(float(x) for x in row)) for row in c]
    c_out = [RGB(0.0) for _ in c]
    gp.Rotate(c_in, c_out, [float(x) for x in m16], lmax, fresh=fresh, angles=angles)
    return np.array([x.tuple() for x in c_out], np.float32)


def host_rotate(c, m16, lmax):
    out = np.zeros_like(c)
    _abi.check(_abi.lib().dr_sh_rotate(np.ascontiguousarray(c).ctypes.data, np.ascontiguousarray(m16).ctypes.data, lmax, out.ctypes.data))
    return out


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("lmax", [1, 2, 3, 4])
def test_host_rotate_equals_the_restatement_and_the_aliasing_is_real(lmax):
    """The host libm serves both sides, so any difference is a logic error.  The same frames through a Rotate whose steps get private copies of
    their inputs give a different answer: the reference's lists share objects, and the device code reproduces what that gives."""
    M, Cf = frames(), coefficients(lmax)
    branch = differs = 0
    for m16, c in zip(M, Cf):
        want = restated_rotate(c, m16, lmax)
        assert _same(host_rotate(c, m16, lmax), want)
        branch += math.sqrt(float(m16[9]) ** 2 + float(m16[8]) ** 2) <= 16 * gp.FLT_EPSILON
        differs += not _same(restated_rotate(c, m16, lmax, fresh=True), want)
    print("lmax %d: %d frames in the sy <= 16 eps branch, %d of 64 frames differ from a Rotate without shared objects" % (lmax, branch, differs))
    assert branch >= 4 and differs >= 1


def _evaluate_function(c, w, lmax):
    return prt.EvaluateMany(w, lmax) @ c.astype(np.float64)


@pytest.mark.parametrize("lmax", [1, 2, 3, 4])
def test_rotate_z_and_rotate_x_plus_alone_are_rotations(lmax):
    """Guards the RESTATEMENT, not the library (it passes without the feature): the restated rows of RotateZ and RotateXPlus, which the library is
    then held to bit for bit by the test above, are checked against what a rotation must do.  On fresh inputs.  RotateZ(alpha): c'(l, +-m) pair
    with cos / sin (m alpha), i.e. f'(theta, phi) = f(theta, phi + alpha).  RotateXPlus: from its
    band-1 rows (Y(1, -1) = -k y, Y(1, 0) = k z, Y(1, 1) = -k x): f'(x, y, z) = f(x, z, -y), which every band must then follow.
    Tolerance: an output coefficient is at most three f32 products and two f32 sums of values below 1 in magnitude (5 roundings of 2^-24 each, plus
    one for the sum's growth), a function value sums Terms of them against |Ylm| <= sqrt((2 lmax + 1) / (2 pi))."""
    terms = prt.Terms(lmax)
    tol = terms * 6 * 2.0 ** -24 * math.sqrt((2 * lmax + 1) / (2.0 * math.pi))
    rng = np.random.RandomState(5)
    w = rng.normal(size=(32, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    c = coefficients(lmax)[0]
    obj = lambda: [RGB(*(float(x) for x in row)) for row in c]
    arr = lambda lst: np.array([x.tuple() for x in lst], np.float32)
    worst = 0.0
    for alpha in (0.3, -1.1, 2.5):
        out = [RGB(0.0) for _ in range(terms)]
        gp.RotateZ(obj(), out, alpha, lmax)
        ca, sa = math.cos(alpha), math.sin(alpha)
        wr = np.stack([ca * w[:, 0] - sa * w[:, 1], sa * w[:, 0] + ca * w[:, 1], w[:, 2]], axis=1)   # phi + alpha
        worst = max(worst, float(np.abs(_evaluate_function(arr(out), w, lmax) - _evaluate_function(c, wr, lmax)).max()))
    out = [None] * terms
    gp.RotateXPlus(obj(), out, lmax)
    wr = np.stack([w[:, 0], w[:, 2], -w[:, 1]], axis=1)
    worst = max(worst, float(np.abs(_evaluate_function(arr(out), w, lmax) - _evaluate_function(c, wr, lmax)).max()))
    print("lmax %d: largest deviation %.3g, tolerance %.3g" % (lmax, worst, tol))
    assert worst <= tol


KD, KS, ROUGH, SCR = (0.6, 0.45, 0.3), (0.2, 0.25, 0.35), 0.1, (0x9E3779B9, 0x7F4A7C15)


def host_bsdf_matrix(Kd, Ks, roughness, scramble, n, lmax):
    t = prt.Terms(lmax)
    out = np.zeros((t, t, 3), np.float32)
    kd, ks, scr = np.array(Kd, np.float32), np.array(Ks, np.float32), np.array(scramble, np.uint32)
    _abi.check(_abi.lib().dr_sh_bsdf_matrix_host(kd.ctypes.data, ks.ctypes.data, float(roughness), scr.ctypes.data, n, lmax, out.ctypes.data))
    return out


@pytest.mark.parametrize("lmax,n", [(1, 4), (2, 16), (4, 32)])
def test_host_bsdf_matrix_equals_the_restatement(lmax, n):
    """Blinn's pow is the numerics contract's documented ulp case, but here both sides call the host libm: bit for bit."""
    f = lambda v: tuple(float(np.float32(x)) for x in v)
    want = gp.ComputeBSDFMatrix(f(KD), f(KS), ROUGH, list(SCR), n, lmax)
    got = host_bsdf_matrix(KD, KS, ROUGH, SCR, n, lmax)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    print("(%d, %d): max |host - restatement| = %.3g of %.3g" % (lmax, n, float(np.abs(got - want).max()), float(np.abs(want).max())))
    assert _same(got, want)
    # the specular lobe is in it: Ks = 0 gives another matrix
    assert not _same(got, host_bsdf_matrix(KD, (0.0, 0.0, 0.0), ROUGH, SCR, n, lmax))


def test_bsdf_matrix_known_answer():
    """With Ks = 0 the BSDF is Kd / pi on same-hemisphere pairs: B[0][0] -> Y_00^2 * Kd / pi * integral over wo, wi in one hemisphere of |cos wi|
    = (1 / 4 pi) * Kd / pi * 2 * (2 pi) * pi = Kd.  Allowed: twice the restatement's own relative deviation at the same (lmax 1, nsamples_b 256);
    measured 0 for the restatement -- 256 points of the (0, 2)-sequence put exactly half the pairs in one hemisphere and integrate |cos| exactly,
    and the f32 sum rounds to Kd -- so 0 allowed, and 0 for the host build (which is the restatement bit for bit)."""
    kd = (0.5, 0.25, 0.125)
    want = gp.ComputeBSDFMatrix(kd, (0.0, 0.0, 0.0), ROUGH, list(SCR), 256, 1)
    got = host_bsdf_matrix(kd, (0.0, 0.0, 0.0), ROUGH, SCR, 256, 1)
    rel = lambda B: float(np.abs(B[0, 0].astype(np.float64) / np.array(kd) - 1.0).max())
    own = rel(want)
    print("known answer: restatement's relative deviation of B[0][0] from Kd = %.4g, allowed = %.4g, host build = %.4g" % (own, 2.0 * own, rel(got)))
    assert own < 0.1 and rel(got) <= 2.0 * own


# ---- the class, the constants ----
def test_defaults_constants_slots_and_plugin():
    a = core.GlossyPRTIntegrator.Create({})                        # glossy_prt_integrator.dart:118-125
    assert (a.Kd, a.Ks, a.roughness, a.lmax, a.nSamples) == ((0.5, 0.5, 0.5), (0.25, 0.25, 0.25), 0.1, 4, 4096)
    b = core.GlossyPRTIntegrator((0.1, 0.2, 0.3), 0.0, 0.05, 2, 100)
    assert (b.Kd, b.Ks, b.roughness, b.lmax, b.nSamples) == ((0.1, 0.2, 0.3), (0.0, 0.0, 0.0), 0.05, 2, 128)
    assert core.GlossyPRTIntegrator.kind == _abi.DR_INTEGRATOR_GLOSSY_PRT == 9 and a.requestSamples(None, None) == ([], [])
    make = core.Plugin.get("surfaceIntegrator", "glossyprt")
    assert isinstance(make(), core.GlossyPRTIntegrator) and make({"lmax": 3, "roughness": 0.2}).roughness == 0.2
    lib = _abi.lib()
    assert lib.dr_sample_floats(9, 3) == lib.dr_sample_floats(_abi.DR_INTEGRATOR_DIFFUSE_PRT, 3) == 7
    # 6 and 8 stay unassigned: answered as every unknown value is (DirectLighting "all")
    assert lib.dr_sample_floats(6, 3) == lib.dr_sample_floats(8, 3) == lib.dr_sample_floats(10, 3) == lib.dr_sample_floats(_abi.DR_INTEGRATOR_DIRECT_ALL, 3) == 25
    assert lib.dr_abi_version() == 9 and C.sizeof(_abi.DrRenderDesc) == 1352 and C.sizeof(_abi.DrGlossyPrtParams) == 32
    cam = scenes.cornell_camera(8, 8)
    d, keep = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, b, core.EmissionIntegrator()).describe()
    assert (d.integrator, d.prt_nsamples, d.prt_lmax, d.max_depth) == (9, 128, 2, 1)
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    for line in ("#define DR_INTEGRATOR_GLOSSY_PRT 9 ", "#define DR_ABI_VERSION 9", "DR_ABI_SIZE(DrRenderDesc, 1352);", "typedef struct DrGlossyPrtParams {",
                 "int dr_scene_set_glossy_prt(", "int dr_prt_bsdf_matrix(", "int dr_sh_rotate(", "int dr_sh_bsdf_matrix_host(", "int dr_sh_rotate_device("):
        assert line in header, line
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    assert "DR_INTEGRATOR_GLOSSY_PRT = 9;" in dart and "'dr_scene_set_glossy_prt'" in dart and "'GlossyPRTIntegrator'" in dart
    assert "SIZEOF_DrGlossyPrtParams = 32" in dart


@pytest.mark.parametrize("kw,needle", [
    (dict(lmax=0), "glossy PRT: lmax must be at least 1"),
    (dict(lmax=5), "glossy PRT: lmax above 4"),
    (dict(nSamples=0), "glossy PRT: nsamples must be at least 1"),
    (dict(nSamples=4097), "glossy PRT: nsamples above 4096 after rounding"),
])
def test_refusals_by_name(kw, needle):
    with pytest.raises(ValueError, match=needle):
        core.GlossyPRTIntegrator(**kw)
    c, m, out = np.zeros((4, 3), np.float32), np.zeros(16, np.float32), np.zeros((36, 3), np.float32)
    for bad in (0, 5):
        assert _abi.lib().dr_sh_rotate(c.ctypes.data, m.ctypes.data, bad, out.ctypes.data) == -1
        assert "glossy PRT: lmax" in _abi.lib().dr_last_error().decode()


def test_the_adaptive_sampler_is_refused_and_the_loader_still_refuses_the_directive():
    cam = scenes.cornell_camera(8, 8)
    mk = lambda s: core.SamplerRenderer(s, cam, core.GlossyPRTIntegrator(lmax=2, nSamples=16), core.EmissionIntegrator())
    with pytest.raises(ValueError, match="glossy PRT: the adaptive sampler is not supported"):
        mk(core.AdaptiveSampler(cam, 2, 8, "contrast", 5489)).describe()
    with pytest.raises(ValueError, match="give the HostBufferSampler the seed"):
        mk(core.HostBufferSampler(cam, 2, [(0, 0)], np.zeros((2, 7), np.float32))).describe()
    with pytest.raises(pbrt.UnsupportedFeature) as e:
        pbrt.loads('SurfaceIntegrator "glossyprt"\nWorldBegin\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                   '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nWorldEnd\n')
    assert "glossyprt" in str(e.value)
