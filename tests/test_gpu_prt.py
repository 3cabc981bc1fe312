"""DiffusePRTIntegrator on the GPU (DR_INTEGRATOR_DIFFUSE_PRT: k_shade_prt, dr_prt_project.hip), bit for bit against the Python
restatement (tests/prt_restatement.py) at two seams: the incident-light coefficients (dr_prt_incident), one light at a time and together, and the
film, the restatement fed the device sampler's own vectors and the keyed in-Li streams.  8 x 8 images (a 9 x 9 sampler window); restated films and
coefficients are computed once per configuration and shared.  Nothing is started after a failed call: every call's return code raises."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt

import prt_restatement as prt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 5489
T = pbrt.Transform


def _quad(p0, p1, p2, p3, kd=(0.5, 0.5, 0.5), light=None, mat=None, **kw):
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([p0, p1, p2, p3], np.float32), **kw)
    if light is not None:
        light = core.DiffuseAreaLight(light[0], light[1], mesh)
    return core.GeometricPrimitive(mesh, mat or core.MatteMaterial(kd), light)


FLOOR = ((-4.0, 0.0, -4.0), (-4.0, 0.0, 6.0), (4.0, 0.0, 6.0), (4.0, 0.0, -4.0))
BLOCKER = ((0.0, 1.5, -1.0), (3.0, 1.5, -1.0), (3.0, 1.5, 3.0), (0.0, 1.5, 3.0))
EMITTER = ((-3.0, 3.0, 0.0), (-1.0, 3.0, 0.0), (-1.0, 3.0, 2.0), (-3.0, 3.0, 2.0))   # faces down (towards the floor)


# a tilted quad in front of the blocker with per-vertex N that lean away from its plane: its shading normal is not its geometric one
LEANING = ((-2.5, 0.2, -2.5), (-2.5, 1.2, -1.5), (-0.3, 1.2, -1.5), (-0.3, 0.2, -2.5))
LEANING_N = np.array([(0.3, 0.7, -0.6), (-0.2, 0.9, -0.3), (-0.3, 0.8, -0.5), (0.4, 0.6, -0.7)], np.float32)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _restated_delta(L):
    t3 = lambda v: tuple(float(x) for x in v)
    if isinstance(L, core.SpotLight):
        return prt.wr.SpotLight(t3(L.lightPos), t3(L.intensity), L.worldToLight.reshape(-1), L.width, L.fall)
    if isinstance(L, core.PointLight):
        return prt.wr.PointLight(t3(L.lightPos), t3(L.intensity))
    return prt.DistantLight(t3(L.lightDir), t3(L.intensity))


class Setup:
    """One scene on both sides.  prims: the geometry (area lights among it); env: a core.InfiniteAreaLight or None; delta: point / spot / distant
    lights.  The device's lights are the area lights, the infinite light, then the delta lights; the restated list is built in that order."""

    def __init__(self, prims, env=None, delta=(), camera="wide", restate=True):
        accel = core.BVHAccel(prims)
        self.scene = core.Scene(accel, accel.lights() + ([env] if env is not None else []) + list(delta))
        if restate:
            self.restated = prt.with_shading_geometry(mrf.build_scene(prims, env), accel)
            for rl, cl in zip(self.restated.lights, accel.lights()):   # (the restated area lights carry no sample count of their own)
                rl.nSamples = cl.nSamples
            self.restated.lights = list(self.restated.lights) + [_restated_delta(L) for L in delta]
        film = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
        if camera == "wide":    # from above: also sees past the floor (escaped camera rays), the blocker and the emitter beside it
            self.camera = core.PerspectiveCamera.lookAt((0.5, 5.0, -7.0), (0.0, 0.5, 1.0), (0.0, 1.0, 0.0), 80.0, film)
        else:                   # looks down at the floor only
            self.camera = core.PerspectiveCamera.lookAt((0.0, 6.0, 0.5), (0.0, 0.0, 0.6), (0.0, 0.0, 1.0), 40.0, film)
        self.films, self.cin = {}, {}

    def renderer(self, args, sampler):
        return core.SamplerRenderer(sampler, self.camera, core.DiffusePRTIntegrator(*args), core.EmissionIntegrator())

    def restated_cin(self, lmax):
        if lmax not in self.cin:
            self.cin[lmax] = prt.DiffusePRTIntegrator(lmax, 1).preprocess(self.restated).c_in
        return self.cin[lmax]

    def restated_film(self, args, sampler, key):
        if (args, key) not in self.films:
            r = self.renderer(args, sampler)
            pixels = r.pixels()
            vec = r.generate_samples(self.scene, pixels)
            assert vec.shape == (len(pixels) * sampler.samplesPerPixel, 7)
            integ = prt.DiffusePRTIntegrator(*args)
            integ.c_in = self.restated_cin(args[0])
            self.films[(args, key)] = (prt.render(self.restated, integ, mrf.restated_camera(self.camera), self.camera.film, sampler.samplesPerPixel,
                                                  pixels, vec, prt.keyed_rng(SEED, prt.rr.sample_extent(self.camera.film))), pixels, vec)
        return self.films[(args, key)]

    def device_film(self, args, sampler):
        return self.renderer(args, sampler).render(self.scene).film

    def device_cin(self, lmax):
        return core.DiffusePRTIntegrator(lmax, 1).incident(self.scene)


def _cin_array(c):
    return np.array([x.tuple() for x in c], np.float32)


def _ld(s, spp=1):
    return core.LowDiscrepancySampler(s.camera, spp, SEED)


def _yard_prims(blocker=True):
    up = ((-3.0, 1.5, -1.0), (-3.0, 1.5, 3.0), (0.0, 1.5, 3.0), (0.0, 1.5, -1.0))   # the film scenes' emitter: beside the blocker, facing up (the camera is above)
    return [_quad(*FLOOR), _quad(*up, light=((6.0, 5.0, 4.0), 1)), _quad(*LEANING, kd=(0.6, 0.5, 0.4), n=LEANING_N)] + ([_quad(*BLOCKER)] if blocker else [])


@pytest.fixture(scope="module")
def yard(gpu):
    """Floor, blocker, an up-facing emitter beside it, under a map-less infinite light: the film has misses, emitter hits and occluded floor."""
    return Setup(_yard_prims(), core.InfiniteAreaLight(None, (0.8, 0.9, 1.0), 1, None))


# ---- 1. the incident light, one light at a time and together ----
def _env_map(w, h):
    rng = np.random.RandomState(w * 131 + h)
    return rng.uniform(0.05, 2.0, size=(h, w, 3)).astype(np.float32)


def _light_case(name):
    pt, sp = T.Translate(1.5, 4.0, -2.0), T.Translate(0.3, 5.0, 1.2) * T.Rotate(90.0, 1.0, 0.0, 0.0)
    plain = [_quad(*FLOOR), _quad(*BLOCKER)]
    if name == "point":
        return Setup(plain, None, [core.PointLight(pt.m, (30.0, 26.0, 22.0))])
    if name == "spot":
        return Setup(plain, None, [core.SpotLight(sp.m, (50.0, 60.0, 70.0), 60.0, 25.0, sp.mInv)])
    if name == "distant":
        return Setup(plain, None, [core.DistantLight(None, (1.5, 2.0, 2.5), (0.3, 1.0, -0.2))])
    if name in ("area4", "area3"):
        return Setup(plain + [_quad(*EMITTER, light=((6.0, 5.0, 4.0), 4 if name == "area4" else 3))])
    if name == "mapless":
        return Setup(plain, core.InfiniteAreaLight(None, (0.8, 0.9, 1.0), 1, None))
    if name.startswith("map"):
        w, h = (int(v) for v in name[3:].split("x"))
        return Setup(plain, core.InfiniteAreaLight(T.Rotate(30.0, 0.2, 1.0, 0.1).m, (1.0, 0.7, 0.5), 1, _env_map(w, h)))
    assert name == "together"
    return Setup(plain + [_quad(*EMITTER, light=((6.0, 5.0, 4.0), 4))], core.InfiniteAreaLight(None, (0.8, 0.9, 1.0), 1, None),
                 [core.PointLight(pt.m, (30.0, 26.0, 22.0)), core.SpotLight(sp.m, (50.0, 60.0, 70.0), 60.0, 25.0, sp.mInv)])


@pytest.mark.parametrize("name", ["point", "spot", "distant", "area4", "area3", "mapless", "map64x52", "map64x50", "map64x32", "together"])
def test_incident_light_equals_the_restatement(gpu, name):
    """map64x52 and map64x50: MIPMap.texture resamples both to 64 x 64 (mipmap.dart:71-138), so BOTH take the lat-long branch of the reference
    (its test reads the resampled map's sides); map64x32, a power of two, is the mapped light that takes the cube branch.  `together`: an area
    light (four samples: three draws of the shared RNG), an infinite light, a point light (no draws) and a spot light (the next three draws)."""
    s = _light_case(name)
    lmax = 4 if name not in ("map64x32",) else 2
    want, got = _cin_array(s.restated_cin(lmax)), s.device_cin(lmax)
    assert got.shape == want.shape == ((lmax + 1) ** 2, 3) and np.isfinite(got).all() and np.abs(got).max() > 0.0
    print("%s: max |device - restatement| = %.3g of %.3g" % (name, float(np.abs(got - want).max()), float(np.abs(want).max())))
    assert _same(got, want)
    if name == "area3":   # three samples round up to four
        assert _same(got, _light_case("area4").device_cin(lmax))


# ---- 2. the film ----
@pytest.mark.parametrize("args", [(1, 1), (2, 8), (4, 64), (4, 256)])
def test_film_equals_the_restatement(yard, args):
    want, pixels, vec = yard.restated_film(args, _ld(yard), "ld")
    got = yard.device_film(args, _ld(yard))
    assert np.isfinite(got).all() and got[..., :3].max() > 0.0
    assert _same(got, want)


def _camera_hits(s, pixels, vec):
    rcam = mrf.restated_camera(s.camera)
    return [s.restated.bvh.intersect(rcam.generateRay(int(px) + float(v[0]), int(py) + float(v[1]), float(v[2]), float(v[3]))) for (px, py), v in zip(pixels, vec)]


def test_the_film_has_misses_emitter_hits_shading_normals_and_shadow(yard):
    """The scene is what the film tests need: camera rays that miss, that see the emitter's lit side (Le), and that hit the mesh with per-vertex N,
    where the shading normal -- the one the integrator uses -- is not the geometric one."""
    want, pixels, vec = yard.restated_film((4, 64), _ld(yard), "ld")
    hits = _camera_hits(yard, pixels, vec)
    assert 3 < sum(h is None for h in hits) < len(hits) - 3
    assert sum(h is not None and h.prim.light is not None for h in hits) >= 1
    leaning = [h for h in hits if h is not None and isinstance(h.prim.shape, prt.fe.Triangle)]
    assert len(leaning) >= 2
    for h in leaning:
        ns, ng = prt.getBSDF(h).nn, h.dg.nn
        assert abs(ns.length() - 1.0) < 1e-6 and prt.Dot(ns, ng) < 0.999   # more than 2.5 degrees apart


def test_removing_the_blocker_changes_the_floor_under_it_only(gpu, yard):
    """The blocker lies inside the other shapes' bounds, so the world bound -- and with it c_in -- stays.  Without it the transfer of the floor
    points that saw it changes; pixels that miss the scene or hit the emitter keep their bytes."""
    open_ = Setup(_yard_prims(blocker=False), core.InfiniteAreaLight(None, (0.8, 0.9, 1.0), 1, None))
    assert _same(open_.device_cin(4), yard.device_cin(4))
    a, b = yard.device_film((4, 64), _ld(yard)), open_.device_film((4, 64), _ld(open_))
    changed = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
    want, pixels, vec = yard.restated_film((4, 64), _ld(yard), "ld")
    under = 0
    for (px, py), h in zip(pixels, _camera_hits(yard, pixels, vec)):
        if not (0 <= px < 8 and 0 <= py < 8):
            continue
        if h is None or h.prim.light is not None:      # the sky, and the emitter, which lies in the blocker's own plane and cannot see it
            assert not changed[py, px]
        elif abs(h.dg.p.y) < 1e-6 and 0.0 < h.dg.p.x < 3.0 and -1.0 < h.dg.p.z < 3.0:   # the floor straight under the blocker
            assert changed[py, px]
            under += 1
    assert under >= 2
    # (a pixel that showed the blocker's own lit top now shows the floor below it, so the change has no fixed sign)
    assert 2 < changed.sum() < 64


# ---- 3. layouts, traversal kernels, samplers ----
def _with_option(name, value, fn):
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(name.encode(), str(value).encode()))
        return fn()
    finally:
        lib.dr_set_option(name.encode(), None)


@pytest.mark.parametrize("impl", ["2", "3", "5f"])
def test_every_traversal_kernel_gives_the_same_film(yard, impl):
    want = yard.restated_film((4, 256), _ld(yard), "ld")[0]
    assert _same(_with_option("TRACE_IMPL", impl, lambda: yard.device_film((4, 256), _ld(yard))), want)


@pytest.mark.parametrize("layout", [64, 4])
def test_both_state_layouts_give_the_same_film(yard, layout):
    want = yard.restated_film((4, 256), _ld(yard), "ld")[0]

    def run():
        return yard.device_film((4, 256), _ld(yard)), yard.scene._device().last_render_info()
    got, info = _with_option("STATE_LAYOUT", layout, run)
    assert info["state_layout"] == layout and _same(got, want)


@pytest.fixture(scope="module")
def yard_sphere(gpu):
    """The yard and a matte sphere of reversed orientation on the floor in front of the blocker: with the plain floor and the leaning quad's
    per-vertex N, every branch of the camera hit's geometry (quadric, triangle with DR_SHADING_N, plain triangle)."""
    at = T.Translate(2.0, 1.5, -2.6)
    ball = core.GeometricPrimitive(core.Sphere(at.m, at.mInv, True, 1.5), core.MatteMaterial((0.4, 0.5, 0.6)), None)
    return Setup(_yard_prims() + [ball], core.InfiniteAreaLight(None, (0.8, 0.9, 1.0), 1, None))


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


def test_halton_sampler_against_the_restatement(yard):
    """The Halton sampler's samples belong to the image: one slot per accepted index k, the in-Li stream keyed (seed, k, 0, kind 2), and a film
    that atomics add in no fixed order, so bit equality of the film is not defined for this sampler (as for ambient occlusion, whose test this
    follows).  What is: the dumped vectors equal the Halton restatement's bit for bit, the weights equal exactly (integer table), and the film
    lies within tests/film_reference.py's derived bound of the f64 sum of the PRT restatement's radiances."""
    import film_reference as fr
    import halton_restatement as hr
    film = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
    film.filterTable[:] = fr.INT_TABLE
    cam = core.PerspectiveCamera.lookAt((0.5, 5.0, -7.0), (0.0, 0.5, 1.0), (0.0, 1.0, 0.0), 80.0, film)
    r = core.SamplerRenderer(core.HaltonSampler(cam, 2, SEED), cam, core.DiffusePRTIntegrator(2, 8), core.EmissionIntegrator())
    k, xy, vec = r.generate_halton_samples(yard.scene)
    want = hr.keyed(hr.task_window(film), 2, SEED, [1, 1], [], 0)
    assert len(k) > 100 and np.array_equal(k, want.k) and np.array_equal(xy, want.pixel_xy)
    assert vec.shape == want.vec.shape == (len(k), 7) and _same(vec, want.vec)
    rcam, integ = mrf.restated_camera(cam), prt.DiffusePRTIntegrator(2, 8)
    integ.c_in = yard.restated_cin(2)
    Ls = np.array([prt.sample_Li(yard.restated, integ, rcam, int(px), int(py), v, prt.dr.RNG(prt.rr.counter_key(SEED, int(kk), 0, prt.rr.LI_KIND)))[0].tuple()
                   for kk, (px, py), v in zip(k, xy, vec)], np.float32)
    ref = fr.reference_from_samples(film, xy, 1, vec[:, 0], vec[:, 1], Ls, serial=False)
    got = r.render(yard.scene).film
    assert np.array_equal(got[..., 3].astype(np.float64), ref.sum[..., 3])
    err, lim = np.abs(got.astype(np.float64) - ref.sum), fr.bound(ref.S, ref.n)
    print("halton: max |device - f64 sum| / bound = %.3g" % float((err[..., :3] / np.maximum(lim[..., :3], 1e-300)).max()))
    assert (err <= lim).all() and np.isfinite(got).all() and got[..., :3].max() > 0


def test_host_buffer_replay_of_the_dumped_vectors(yard):
    want, pixels, vec = yard.restated_film((2, 8), _ld(yard), "ld")
    got = yard.renderer((2, 8), core.HostBufferSampler(yard.camera, 1, pixels, vec, seed=SEED)).render(yard.scene).film
    assert _same(got, want)


# ---- 4. what ran; leaks ----
def test_last_render_info_and_the_path_integrator_before_and_after(yard):
    path = lambda: core.SamplerRenderer(_ld(yard, 2), yard.camera, core.PathIntegrator(3), core.EmissionIntegrator()).render(yard.scene).film
    before = path()
    r = yard.renderer((4, 256), _ld(yard))
    r.render(yard.scene)
    info = yard.scene._device().last_render_info()
    assert info["integrator"] == "diffuseprt" and info["shade_kernels"] == ["k_shade_prt"]
    st = r.last_stats
    assert st["camera_samples"] == 81 and 0 < st["shade_vertices"] <= 81 and st["any_launches"] == 256 and st["closest_launches"] == 1
    assert 0 < st["any_rays"] < st["shade_vertices"] * 256   # the rays below the shading normal's plane are never traced
    after = path()
    assert _same(before, after) and before[..., :3].max() > 0.0
    info = yard.scene._device().last_render_info()
    assert info["integrator"] is None and info["shade_kernels"] == []


# ---- 5. refusals ----
def test_refusals_by_name_leave_the_scene_usable(yard):
    lib = _abi.lib()
    film = np.zeros((8, 8, 4), np.float32)

    def refused(code, needle, mutate):
        d, keep = yard.renderer((2, 8), _ld(yard)).describe()
        mutate(d)
        rc = lib.dr_render(yard.scene._device().handle, C.byref(d), film.ctypes.data, None)
        assert rc == code, rc
        assert needle in lib.dr_last_error().decode(), lib.dr_last_error()

    refused(-1, "diffuse PRT: lmax must be at least 1", lambda d: setattr(d, "prt_lmax", 0))
    refused(-1, "diffuse PRT: lmax above 8", lambda d: setattr(d, "prt_lmax", 9))
    refused(-1, "diffuse PRT: nsamples must be at least 1", lambda d: setattr(d, "prt_nsamples", 0))
    refused(-1, "diffuse PRT: nsamples above 4096", lambda d: setattr(d, "prt_nsamples", 4097))

    def adaptive(d):
        d.sampler_mode, d.spp, d.strat_xsamples = _abi.DR_SAMPLER_ADAPTIVE, 8, 2
    refused(-4, "diffuse PRT: the adaptive sampler is not supported", adaptive)
    d, keep = yard.renderer((2, 8), _ld(yard)).describe()
    d.prt_nsamples = 5   # rounded up by the library as by the constructor
    _abi.check(lib.dr_render(yard.scene._device().handle, C.byref(d), film.ctypes.data, None))
    assert _same(film, yard.restated_film((2, 8), _ld(yard), "ld")[0])


@pytest.mark.parametrize("name,mat", [("matte with sigma != 0", lambda: core.MatteMaterial((0.5, 0.5, 0.5), 20.0)), ("mirror", lambda: core.MirrorMaterial((0.9, 0.9, 0.9))),
                                      ("glass", lambda: core.GlassMaterial((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.5)),
                                      ("plastic", lambda: core.PlasticMaterial((0.4, 0.4, 0.4), (0.3, 0.3, 0.3), 0.1))])
def test_unsupported_materials_are_refused_by_name(gpu, name, mat):
    env = lambda: core.InfiniteAreaLight(None, (1.0, 1.0, 1.0), 1, None)
    bad = Setup([_quad(*FLOOR), _quad(*BLOCKER, mat=mat())], env(), restate=False)
    with pytest.raises(_abi.DartRayHipError, match="diffuse PRT: material " + name.replace("!", "\\!") + ".*is not supported"):
        bad.device_film((2, 8), _ld(bad))
    # the scene is still usable (another integrator), and the same geometry in matte renders
    assert np.isfinite(core.SamplerRenderer(_ld(bad), bad.camera, core.AmbientOcclusionIntegrator(8), core.EmissionIntegrator()).render(bad.scene).film).all()
    good = Setup([_quad(*FLOOR), _quad(*BLOCKER)], env())
    assert good.device_film((2, 8), _ld(good))[..., :3].max() > 0.0


# ---- 6. a known answer that does not come from the restatement ----
def test_an_open_plane_under_a_constant_sky_tends_to_kd_times_l(gpu):
    """An unoccluded matte plane (Kd 0.5, 0.25, 0.125) under a map-less infinite light L = 1, lmax 2, nsamples 256.  A constant sky has only its
    l = 0 coefficient, so Lo = c_in[0] * c[0] -> (2 sqrt(pi)) * (sqrt(pi) / 2) = pi and Li -> Kd / pi * pi = Kd * L.  The allowed deviation is
    twice the restatement's own largest relative deviation from Kd over the same samples, computed here on the CPU and printed with the device's:
    measured 0.006519 for the restatement, so 0.01304 allowed, and 0.006519 for the device (which is the restatement bit for bit, as
    test_film_equals_the_restatement pins on the other scene)."""
    kd = (0.5, 0.25, 0.125)
    s = Setup([_quad((-40.0, 0.0, -40.0), (-40.0, 0.0, 40.0), (40.0, 0.0, 40.0), (40.0, 0.0, -40.0), kd=kd)], core.InfiniteAreaLight(None, (1.0, 1.0, 1.0), 1, None), camera="down")
    want = s.restated_film((2, 256), _ld(s), "ld")[0]
    got = s.device_film((2, 256), _ld(s))
    rel = lambda f: np.abs(f[..., :3] / f[..., 3:4] / _xyz_of(kd) - 1.0).max()
    own = float(rel(want))
    print("known answer: restatement's largest relative deviation from Kd * L = %.4g, allowed = %.4g, device = %.4g" % (own, 2.0 * own, float(rel(got))))
    assert (got[..., 3] > 0).all() and own < 0.1 and rel(got) <= 2.0 * own


def _xyz_of(rgb):
    r, g, b = rgb   # RGBToXYZ (spectrum.dart): the film holds XYZ
    return np.array([0.412453 * r + 0.357580 * g + 0.180423 * b, 0.212671 * r + 0.715160 * g + 0.072169 * b, 0.019334 * r + 0.119193 * g + 0.950227 * b])
