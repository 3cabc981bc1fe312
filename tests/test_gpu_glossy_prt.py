"""GlossyPRTIntegrator on the GPU (DR_INTEGRATOR_GLOSSY_PRT: k_shade_gprt, k_gprt_finish, the BSDF-matrix kernels of dr_prt_project.hip; DESIGN.md
2.17), bit for bit against the Python restatement (tests/glossy_prt_restatement.py) at three seams: the rotation run by one device lane, the BSDF
matrix, and the film -- the restatement fed the device sampler's own vectors, the keyed in-Li streams and the host build's BSDF matrix at 1024
directions (which the device's own is compared with).  The yard scene of tests/test_gpu_prt.py, rebuilt here: 8 x 8 images (a 9 x 9 sampler
window); restated films are computed once per configuration and shared.  Nothing is started after a failed call: every return code raises."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dartray_amd import _abi, core

import glossy_prt_restatement as gp
import prt_restatement as prt
from test_glossy_prt_integrator import coefficients, frames, host_bsdf_matrix, host_rotate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 5489
KD, KS, ROUGH = (0.6, 0.45, 0.3), (0.2, 0.25, 0.35), 0.1
F = lambda v: tuple(float(np.float32(x)) for x in v)

FLOOR = ((-4.0, 0.0, -4.0), (-4.0, 0.0, 6.0), (4.0, 0.0, 6.0), (4.0, 0.0, -4.0))
BLOCKER = ((0.0, 1.5, -1.0), (3.0, 1.5, -1.0), (3.0, 1.5, 3.0), (0.0, 1.5, 3.0))
UP = ((-3.0, 1.5, -1.0), (-3.0, 1.5, 3.0), (0.0, 1.5, 3.0), (0.0, 1.5, -1.0))   # the emitter: beside the blocker, facing up (the camera is above)
# a tilted quad in front of the blocker with per-vertex N that lean away from its plane: its shading frame is not its geometric one
LEANING = ((-2.5, 0.2, -2.5), (-2.5, 1.2, -1.5), (-0.3, 1.2, -1.5), (-0.3, 0.2, -2.5))
LEANING_N = np.array([(0.3, 0.7, -0.6), (-0.2, 0.9, -0.3), (-0.3, 0.8, -0.5), (0.4, 0.6, -0.7)], np.float32)


def _quad(p0, p1, p2, p3, kd=(0.5, 0.5, 0.5), light=None, mat=None, **kw):
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([p0, p1, p2, p3], np.float32), **kw)
    if light is not None:
        light = core.DiffuseAreaLight(light[0], light[1], mesh)
    return core.GeometricPrimitive(mesh, mat or core.MatteMaterial(kd), light)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _yard_prims(blocker=True, mats=(None, None, None)):
    return [_quad(*FLOOR, mat=mats[0]), _quad(*UP, light=((6.0, 5.0, 4.0), 1)), _quad(*LEANING, kd=(0.6, 0.5, 0.4), n=LEANING_N, mat=mats[1])] + \
        ([_quad(*BLOCKER, mat=mats[2])] if blocker else [])


def _env():
    return core.InfiniteAreaLight(None, (0.8, 0.9, 1.0), 1, None)


class Setup:
    """One scene on both sides: `prims` on the device, `restate_prims` (default: the same) in the restatement -- the integrator reads no material,
    so a scene of mirror, glass, plastic and Oren-Nayar is restated by the same geometry in matte."""

    def __init__(self, prims, restate_prims=None):
        accel = core.BVHAccel(prims)
        self.scene = core.Scene(accel, accel.lights() + [_env()])
        racc = accel if restate_prims is None else core.BVHAccel(restate_prims)
        self.restated = prt.with_shading_geometry(mrf.build_scene(prims if restate_prims is None else restate_prims, _env()), racc)
        for rl, cl in zip(self.restated.lights, accel.lights()):
            rl.nSamples = cl.nSamples
        film = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
        self.camera = core.PerspectiveCamera.lookAt((0.5, 5.0, -7.0), (0.0, 0.5, 1.0), (0.0, 1.0, 0.0), 80.0, film)
        self.films, self.pre = {}, {}

    def integrator(self, args, ks=KS):
        return core.GlossyPRTIntegrator(KD, ks, ROUGH, *args)

    def renderer(self, args, sampler, ks=KS):
        return core.SamplerRenderer(sampler, self.camera, self.integrator(args, ks), core.EmissionIntegrator())

    def preprocess(self, lmax, ks=KS):
        """c_in by the restatement, the scramble ComputeBSDFMatrix then draws from the same RNG, and B at 1024 directions by the host build."""
        if (lmax, ks) not in self.pre:
            rng = prt.dr.RNG()
            cin = prt.ProjectIncidentDirectRadiance(prt.world_centre(self.restated), 0.0, self.restated.lights, lmax, rng)
            scr = (rng.randomUint(), rng.randomUint())
            self.pre[(lmax, ks)] = (cin, scr, host_bsdf_matrix(KD, ks, ROUGH, scr, 1024, lmax))
        return self.pre[(lmax, ks)]

    def restated_film(self, args, sampler, key, ks=KS):
        if (args, key, ks) not in self.films:
            r = self.renderer(args, sampler, ks)
            pixels = r.pixels()
            vec = r.generate_samples(self.scene, pixels)
            integ = gp.GlossyPRTIntegrator(*args)
            integ.c_in, _, integ.B = self.preprocess(args[0], ks)
            self.films[(args, key, ks)] = (prt.render(self.restated, integ, mrf.restated_camera(self.camera), self.camera.film, sampler.samplesPerPixel,
                                                      pixels, vec, prt.keyed_rng(SEED, prt.rr.sample_extent(self.camera.film))), pixels, vec)
        return self.films[(args, key, ks)]

    def device_film(self, args, sampler, ks=KS):
        return self.renderer(args, sampler, ks).render(self.scene).film


def _ld(s, spp=1):
    return core.LowDiscrepancySampler(s.camera, spp, SEED)


@pytest.fixture(scope="module")
def yard(gpu):
    return Setup(_yard_prims())


# ---- 1. the rotation by one device lane ----
@pytest.mark.parametrize("lmax", [1, 2, 3, 4])
def test_device_rotate_equals_the_host_build(gpu, lmax):
    """The device's f64 atan2 / sin / cos against the host libm's: the largest difference is printed in f32 ulp of the largest coefficient."""
    M, Cf = frames(), coefficients(lmax)
    got = np.zeros_like(Cf)
    _abi.check(_abi.lib().dr_sh_rotate_device(Cf.ctypes.data, M.ctypes.data, lmax, len(M), got.ctypes.data))
    want = np.stack([host_rotate(c, m, lmax) for c, m in zip(Cf, M)])
    ulp = float(np.spacing(np.float32(np.abs(want).max())))
    print("lmax %d: max |device - host| = %.3g = %.3g ulp of the largest coefficient" % (lmax, float(np.abs(got - want).max()), float(np.abs(got - want).max()) / ulp))
    assert _same(got, want)


# ---- 2. the BSDF matrix ----
@pytest.mark.parametrize("lmax,n", [(1, 4), (2, 16), (4, 32), (2, 1024)])
def test_device_bsdf_matrix_equals_the_host_build(yard, lmax, n):
    _, scr, _ = yard.preprocess(lmax)
    got = yard.integrator((lmax, 1)).bsdf_matrix(yard.scene, n)
    want = host_bsdf_matrix(KD, KS, ROUGH, scr, n, lmax)
    print("(%d, %d): max |device - host| = %.3g of %.3g" % (lmax, n, float(np.abs(got - want).max()), float(np.abs(want).max())))
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0 and _same(got, want)


# ---- 3. the film ----
@pytest.mark.parametrize("args", [(1, 1), (2, 8), (4, 64), (4, 128), (4, 256)])
def test_film_equals_the_restatement(yard, args):
    """A round of the stage loop is min(nSamples, 128) rays: 128 is ONE full round and two 64-sample chunks of the finish kernel; 256 is TWO rounds --
    the round lists, the scramble reloaded from the slot words in round 1, the visibility words kept across the counter reset, the one finish
    launch behind the last round -- and four chunks, visibility words 0 to 7; 1 and 8 leave chunk lanes idle; lmax 1 uses 10 of T's elements."""
    want, pixels, vec = yard.restated_film(args, _ld(yard), "ld")
    got = yard.device_film(args, _ld(yard))
    assert np.isfinite(got).all() and got[..., :3].max() > 0.0
    print("%s: max |device - restatement| = %.3g of %.3g" % (args, float(np.abs(got - want).max()), float(np.abs(want).max())))
    assert _same(got, want)


def _camera_hits(s, pixels, vec):
    rcam = mrf.restated_camera(s.camera)
    return [s.restated.bvh.intersect(rcam.generateRay(int(px) + float(v[0]), int(py) + float(v[1]), float(v[2]), float(v[3]))) for (px, py), v in zip(pixels, vec)]


def test_the_film_has_misses_emitter_hits_and_shading_frames(yard):
    want, pixels, vec = yard.restated_film((4, 64), _ld(yard), "ld")
    hits = _camera_hits(yard, pixels, vec)
    assert 3 < sum(h is None for h in hits) < len(hits) - 3
    assert sum(h is not None and h.prim.light is not None for h in hits) >= 1
    leaning = [h for h in hits if h is not None and isinstance(h.prim.shape, prt.fe.Triangle)]
    assert len(leaning) >= 2
    for h in leaning:
        ns, ng = gp.shading_frame(h).nn, h.dg.nn
        assert abs(ns.length() - 1.0) < 1e-6 and prt.Dot(ns, ng) < 0.999   # more than 2.5 degrees apart


def test_removing_the_blocker_changes_the_floor_under_it_and_no_sky_pixel(gpu, yard):
    open_ = Setup(_yard_prims(blocker=False))
    a, b = yard.device_film((4, 64), _ld(yard)), open_.device_film((4, 64), _ld(open_))
    changed = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
    want, pixels, vec = yard.restated_film((4, 64), _ld(yard), "ld")
    under = 0
    for (px, py), h in zip(pixels, _camera_hits(yard, pixels, vec)):
        if not (0 <= px < 8 and 0 <= py < 8):
            continue
        if h is None:
            assert not changed[py, px]
        elif h.prim.light is None and abs(h.dg.p.y) < 1e-6 and 0.0 < h.dg.p.x < 3.0 and -1.0 < h.dg.p.z < 3.0:   # the floor straight under the blocker
            assert changed[py, px]
            under += 1
    assert under >= 2 and 2 < changed.sum() < 64


def test_ks_changes_hit_pixels_and_no_miss_pixel(yard):
    a, b = yard.device_film((4, 64), _ld(yard), ks=(0.0, 0.0, 0.0)), yard.device_film((4, 64), _ld(yard), ks=(0.25, 0.25, 0.25))
    changed = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
    want, pixels, vec = yard.restated_film((4, 64), _ld(yard), "ld")
    nhit = 0
    for (px, py), h in zip(pixels, _camera_hits(yard, pixels, vec)):
        if 0 <= px < 8 and 0 <= py < 8:
            if h is None:
                assert not changed[py, px]
            elif h.prim.light is None:
                nhit += int(changed[py, px])
    assert nhit >= 8
    # ... and Ks = 0 is the restatement's film too (another B, the scene's cache keyed by it)
    assert _same(a, yard.restated_film((4, 64), _ld(yard), "ld", ks=(0.0, 0.0, 0.0))[0])


def test_every_material_renders_and_equals_the_restatement(gpu):
    """Mirror, glass, plastic and Oren-Nayar matte: diffuse PRT refuses all four by name; glossy PRT reads no material function."""
    mats = (core.PlasticMaterial((0.4, 0.4, 0.4), (0.3, 0.3, 0.3), 0.1), core.MatteMaterial((0.5, 0.5, 0.5), 20.0), core.MirrorMaterial((0.9, 0.9, 0.9)))
    prims = _yard_prims(mats=mats) + [_quad((-3.5, 0.1, 3.5), (-3.5, 1.0, 3.5), (-2.0, 1.0, 4.5), (-2.0, 0.1, 4.5), mat=core.GlassMaterial((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.5))]
    matte = _yard_prims() + [_quad((-3.5, 0.1, 3.5), (-3.5, 1.0, 3.5), (-2.0, 1.0, 4.5), (-2.0, 0.1, 4.5))]
    s = Setup(prims, matte)
    want = s.restated_film((2, 8), _ld(s), "ld")[0]
    got = s.device_film((2, 8), _ld(s))
    assert got[..., :3].max() > 0.0 and _same(got, want)


# ---- 4. layouts, traversal kernels, samplers ----
def _with_option(name, value, fn):
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(name.encode(), str(value).encode()))
        return fn()
    finally:
        lib.dr_set_option(name.encode(), None)


@pytest.mark.parametrize("impl", ["2", "3", "5f"])
def test_every_traversal_kernel_gives_the_same_film(yard, impl):
    want = yard.restated_film((4, 256), _ld(yard), "ld")[0]   # two rounds of the stage loop
    assert _same(_with_option("TRACE_IMPL", impl, lambda: yard.device_film((4, 256), _ld(yard))), want)


@pytest.mark.parametrize("layout", [64, 4])
def test_both_state_layouts_give_the_same_film(yard, layout):
    want = yard.restated_film((4, 256), _ld(yard), "ld")[0]   # two rounds of the stage loop

    def run():
        return yard.device_film((4, 256), _ld(yard)), yard.scene._device().last_render_info()
    got, info = _with_option("STATE_LAYOUT", layout, run)
    assert info["state_layout"] == layout and _same(got, want)


@pytest.fixture(scope="module")
def yard_sphere(gpu):
    """The yard and a matte sphere of reversed orientation on the floor in front of the blocker: with the plain floor and the leaning quad's
    per-vertex N, every branch of the camera hit's geometry (quadric, triangle with DR_SHADING_N, plain triangle)."""
    from dartray_amd import pbrt
    at = pbrt.Transform.Translate(2.0, 1.5, -2.6)
    ball = core.GeometricPrimitive(core.Sphere(at.m, at.mInv, True, 1.5), core.MatteMaterial((0.4, 0.5, 0.6)), None)
    return Setup(_yard_prims() + [ball])


@pytest.mark.parametrize("layout", [64, 4])
def test_a_quadric_among_the_camera_hits(yard_sphere, layout):
    s = yard_sphere
    want, pixels, vec = s.restated_film((2, 8), _ld(s), "ld")
    hits = _camera_hits(s, pixels, vec)
    on = [sum(h is not None and isinstance(h.prim.shape, cls) for h in hits) for cls in (prt.dr.Sphere, prt.fe.Triangle)]
    on.append(sum(h is not None and type(h.prim.shape) is prt.dr.Triangle for h in hits))
    print("camera hits: %d on the sphere, %d on the mesh with N, %d on plain triangles" % tuple(on))
    assert min(on) >= 2

    def run():
        return s.device_film((2, 8), _ld(s)), s.scene._device().last_render_info()
    got, info = _with_option("STATE_LAYOUT", layout, run)
    assert info["state_layout"] == layout and _same(got, want)


@pytest.mark.parametrize("name", ["random", "stratified"])
def test_other_samplers_equal_the_restatement_fed_their_vectors(yard, name):
    mk = {"stratified": lambda: core.StratifiedSampler(yard.camera, 2, 1, True, SEED), "random": lambda: core.RandomSampler(yard.camera, 2, SEED)}[name]
    want = yard.restated_film((2, 8), mk(), name)[0]
    assert _same(yard.device_film((2, 8), mk()), want)


# ---- 5. what ran; leaks; refusals ----
def test_last_render_info_and_the_path_integrator_before_and_after(yard):
    path = lambda: core.SamplerRenderer(_ld(yard, 2), yard.camera, core.PathIntegrator(3), core.EmissionIntegrator()).render(yard.scene).film
    before = path()
    r = yard.renderer((4, 256), _ld(yard))
    got = r.render(yard.scene).film
    assert _same(got, yard.restated_film((4, 256), _ld(yard), "ld")[0])
    info = yard.scene._device().last_render_info()
    assert info["integrator"] == "glossyprt" and info["shade_kernels"] == ["k_shade_gprt", "k_gprt_finish"]
    st = r.last_stats
    assert st["camera_samples"] == 81 and 0 < st["shade_vertices"] <= 81 and st["any_launches"] == 256 and st["closest_launches"] == 1   # two rounds of 128
    assert st["any_rays"] == st["shade_vertices"] * 256   # every ray is traced: no Dot(w, n) test
    after = path()
    assert _same(before, after) and before[..., :3].max() > 0.0
    info = yard.scene._device().last_render_info()
    assert info["integrator"] is None and info["shade_kernels"] == []


def test_refusals_by_name_leave_the_scene_usable(yard):
    lib = _abi.lib()
    film = np.zeros((8, 8, 4), np.float32)

    def refused(code, needle, mutate):
        d, keep = yard.renderer((2, 8), _ld(yard)).describe()
        mutate(d)
        rc = lib.dr_render(yard.scene._device().handle, C.byref(d), film.ctypes.data, None)
        assert rc == code, rc
        assert needle in lib.dr_last_error().decode(), lib.dr_last_error()

    refused(-1, "glossy PRT: lmax must be at least 1", lambda d: setattr(d, "prt_lmax", 0))
    refused(-1, "glossy PRT: lmax above 4", lambda d: setattr(d, "prt_lmax", 5))
    refused(-1, "glossy PRT: nsamples must be at least 1", lambda d: setattr(d, "prt_nsamples", 0))
    refused(-1, "glossy PRT: nsamples above 4096", lambda d: setattr(d, "prt_nsamples", 4097))
    refused(-1, "unknown integrator", lambda d: setattr(d, "integrator", 8))

    def adaptive(d):
        d.sampler_mode, d.spp, d.strat_xsamples = _abi.DR_SAMPLER_ADAPTIVE, 8, 2
    refused(-4, "glossy PRT: the adaptive sampler is not supported", adaptive)
    yard.integrator((2, 8)).bind(yard.scene)
    d, keep = yard.renderer((2, 8), _ld(yard)).describe()
    d.prt_nsamples = 5   # rounded up by the library as by the constructor
    _abi.check(lib.dr_render(yard.scene._device().handle, C.byref(d), film.ctypes.data, None))
    assert _same(film, yard.restated_film((2, 8), _ld(yard), "ld")[0])


def test_diffuse_then_glossy_then_diffuse_on_one_scene(gpu):
    """Each film is what its integrator gives alone on a scene of its own: the side buffers' sizing and the scene's caches do not leak."""
    diffuse = lambda s: core.SamplerRenderer(_ld(s), s.camera, core.DiffusePRTIntegrator(4, 64), core.EmissionIntegrator()).render(s.scene).film
    alone_d, alone_g = Setup(_yard_prims()), Setup(_yard_prims())
    d0, g0 = diffuse(alone_d), alone_g.device_film((4, 256), _ld(alone_g))
    s = Setup(_yard_prims())
    d1 = diffuse(s)
    g1 = s.device_film((4, 256), _ld(s))
    d2 = diffuse(s)
    assert _same(d1, d0) and _same(g1, g0) and _same(d2, d0) and not _same(d0[..., :3], g0[..., :3])
