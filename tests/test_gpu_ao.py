"""AmbientOcclusionIntegrator on the GPU (DR_INTEGRATOR_AO, k_shade_ao), bit for bit against the Python restatement
(tests/ao_restatement.py) fed the device sampler's own vectors (dr_generate_samples) and the keyed in-Li streams read in order: the
radiance of a sample is an integer over a power of two, so there is no tolerance anywhere (the Halton film apart, which atomics add in no
fixed order: see its test).  8 x 8 images (a 9 x 9 sampler window) at 2 samples per pixel; a restated film is computed once per
configuration and shared.  Nothing is started after a failed call: every call's return code raises."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt

import ao_restatement as ao

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 5489
T = pbrt.Transform


def _quad(p0, p1, p2, p3):
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([p0, p1, p2, p3], np.float32))
    return core.GeometricPrimitive(mesh, core.MatteMaterial((0.5, 0.5, 0.5)), None)


def _prims():
    """A floor quad, an occluder quad 1.5 above part of it, and a sphere standing on the floor whose orientation is reversed (the quadric
    hit path; its geometric normal points inwards and FaceForward turns it).  No light: the integrator needs none."""
    at = T.Translate(-1.5, 1.0, 1.0)
    return [_quad((-4.0, 0.0, -4.0), (-4.0, 0.0, 6.0), (4.0, 0.0, 6.0), (4.0, 0.0, -4.0)),
            _quad((0.0, 1.5, -1.0), (3.0, 1.5, -1.0), (3.0, 1.5, 3.0), (0.0, 1.5, 3.0)),
            core.GeometricPrimitive(core.Sphere(at.m, at.mInv, True, 1.0), core.MatteMaterial((0.5, 0.5, 0.5)), None)]


def _leaning():
    """A small tilted quad with per-vertex N that lean away from its plane (a shading record with DR_SHADING_N).  The integrator reads
    isect.dg.nn and dgShading.p, which Triangle.getShadingGeometry leaves alone, so the restatement's plain triangles stay its reference."""
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([(0.2, 0.2, -2.5), (0.2, 1.2, -1.5), (2.4, 1.2, -1.5), (2.4, 0.2, -2.5)], np.float32),
                             n=np.array([(0.3, 0.7, -0.6), (-0.2, 0.9, -0.3), (-0.3, 0.8, -0.5), (0.4, 0.6, -0.7)], np.float32))
    return core.GeometricPrimitive(mesh, core.MatteMaterial((0.5, 0.5, 0.5)), None)


class Setup:
    """One scene on both sides: `scene` for the device, `restated` for tests/ao_restatement.py.  wide: a camera that also sees past the
    floor, under a constant infinite light (the Le route of an escaped camera ray)."""

    def __init__(self, wide=False, leaning=False):
        prims = _prims() + ([_leaning()] if leaning else [])
        self.env = core.InfiniteAreaLight(None, (1.0, 1.0, 1.0), 1, np.full((2, 4, 3), (0.5, 0.6, 0.9), np.float32)) if wide else None
        accel = self.accel = core.BVHAccel(prims)
        self.scene = core.Scene(accel, accel.lights() + ([self.env] if wide else []))
        self.restated = mrf.build_scene(prims, self.env)
        film = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
        if wide:
            self.camera = core.PerspectiveCamera.lookAt((0.0, 2.5, -9.0), (0.0, 1.5, 1.0), (0.0, 1.0, 0.0), 75.0, film)
        else:
            self.camera = core.PerspectiveCamera.lookAt((0.5, 4.0, -5.0), (0.3, 0.2, 1.0), (0.0, 1.0, 0.0), 50.0, film)
        self.films = {}

    def renderer(self, integ, sampler):
        return core.SamplerRenderer(sampler, self.camera, integ, core.EmissionIntegrator())

    def restated_film(self, args, sampler, key):
        """The restatement's film for AmbientOcclusionIntegrator(*args) and the vectors the device sampler `sampler` generates (cached)."""
        if (args, key) not in self.films:
            r = self.renderer(core.AmbientOcclusionIntegrator(*args), sampler)
            pixels = r.pixels()
            vec = r.generate_samples(self.scene, pixels)
            assert vec.shape == (len(pixels) * sampler.samplesPerPixel, 7)  # image, lens, time, tau, scatter: no slots of its own
            ext = ao.rr.sample_extent(self.camera.film)
            self.films[(args, key)] = (ao.render(self.restated, ao.AmbientOcclusionIntegrator(*args), mrf.restated_camera(self.camera), self.camera.film,
                                                 sampler.samplesPerPixel, pixels, vec, ao.keyed_rng(SEED, ext)), pixels, vec)
        return self.films[(args, key)]

    def device_film(self, args, sampler):
        return self.renderer(core.AmbientOcclusionIntegrator(*args), sampler).render(self.scene).film


@pytest.fixture(scope="module")
def yard(gpu):
    return Setup()


@pytest.fixture(scope="module")
def wide(gpu):
    return Setup(wide=True)


def _ld(s, spp=2):
    return core.LowDiscrepancySampler(s.camera, spp, SEED)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- 1. the film against the restatement: one ray, one round, two rounds (256 crosses the 128 rays of a round) ----
@pytest.mark.parametrize("ns", [1, 8, 256])
def test_film_equals_the_restatement(yard, ns):
    want, pixels, vec = yard.restated_film((ns,), _ld(yard), "ld")
    assert len(pixels) == 81
    got = yard.device_film((ns,), _ld(yard))
    assert np.isfinite(got).all() and got[..., :3].max() > 0.0
    assert _same(got, want)


def test_the_scene_occludes_and_the_sample_count_shows(yard):
    """The restated films themselves: neither all clear nor all blocked, and the three counts differ."""
    f = {ns: yard.restated_film((ns,), _ld(yard), "ld")[0] for ns in (1, 8, 256)}
    y = f[256][..., 1] / np.maximum(f[256][..., 3], 1e-30)
    assert y.min() < 0.6 and y.max() > 0.9
    assert not _same(f[1], f[8]) and not _same(f[8], f[256])


# ---- 2. the other device samplers, nSamples 8 ----
@pytest.mark.parametrize("name", ["random", "stratified"])
def test_other_samplers_equal_the_restatement_fed_their_vectors(yard, name):
    mk = {"stratified": lambda: core.StratifiedSampler(yard.camera, 2, 1, True, SEED),
          "random": lambda: core.RandomSampler(yard.camera, 2, SEED)}[name]
    want = yard.restated_film((8,), mk(), name)[0]
    assert _same(yard.device_film((8,), mk()), want)
    assert not _same(want, yard.restated_film((8,), _ld(yard), "ld")[0])


def test_halton_sampler_against_the_restatement(yard):
    """The Halton sampler's samples belong to the image: one slot per accepted index k, the in-Li stream keyed (seed, k, 0, kind 2), and a
    film that atomics add in no fixed order, so bit equality of the film is not defined for this sampler.  What is: the dumped 7-float
    vectors equal the Halton restatement's bit for bit, the weights equal exactly (integer table), and the film lies within
    tests/film_reference.py's derived bound of the f64 sum of the AO restatement's radiances."""
    import film_reference as fr
    import halton_restatement as hr
    film = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
    film.filterTable[:] = fr.INT_TABLE
    cam = core.PerspectiveCamera.lookAt((0.5, 4.0, -5.0), (0.3, 0.2, 1.0), (0.0, 1.0, 0.0), 50.0, film)
    r = core.SamplerRenderer(core.HaltonSampler(cam, 2, SEED), cam, core.AmbientOcclusionIntegrator(8), core.EmissionIntegrator())
    k, xy, vec = r.generate_halton_samples(yard.scene)
    want = hr.keyed(hr.task_window(film), 2, SEED, [1, 1], [], 0)
    assert len(k) > 100 and np.array_equal(k, want.k) and np.array_equal(xy, want.pixel_xy)
    assert vec.shape == want.vec.shape == (len(k), 7) and _same(vec, want.vec)
    rcam, integ = mrf.restated_camera(cam), ao.AmbientOcclusionIntegrator(8)
    Ls = np.array([ao.sample_Li(yard.restated, integ, rcam, int(px), int(py), v, ao.dr.RNG(ao.rr.counter_key(SEED, int(kk), 0, ao.rr.LI_KIND)))[0].tuple()
                   for kk, (px, py), v in zip(k, xy, vec)], np.float32)
    ref = fr.reference_from_samples(film, xy, 1, vec[:, 0], vec[:, 1], Ls, serial=False)
    got = r.render(yard.scene).film
    assert np.array_equal(got[..., 3].astype(np.float64), ref.sum[..., 3])
    err, lim = np.abs(got.astype(np.float64) - ref.sum), fr.bound(ref.S, ref.n)
    print("max |device - f64 sum| / bound = %.3g" % float((err[..., :3] / np.maximum(lim[..., :3], 1e-300)).max()))
    assert (err <= lim).all() and np.isfinite(got).all() and got[..., :3].max() > 0


# ---- 3. the rays' extent ----
def test_mindist_skips_the_occluder_and_maxdist_ends_the_rays(yard):
    """mindist 2.5: a ray from the floor under the occluder (1.5 above) only counts it where it meets it further than 2.5 away; maxdist 6."""
    want = yard.restated_film((8, 2.5, 6.0), _ld(yard), "ld")[0]
    assert _same(yard.device_film((8, 2.5, 6.0), _ld(yard)), want)
    assert not _same(want, yard.restated_film((8,), _ld(yard), "ld")[0])


# ---- 4. escaped camera rays: the lights' Le ----
def test_part_of_the_film_misses_the_scene(wide):
    want, pixels, vec = wide.restated_film((8,), _ld(wide), "ld")
    got = wide.device_film((8,), _ld(wide))
    assert _same(got, want)
    # the case is what it says: some camera rays leave the scene, some do not
    rcam = mrf.restated_camera(wide.camera)
    missed = [wide.restated.bvh.intersect(rcam.generateRay(int(px) + float(v[0]), int(py) + float(v[1]), float(v[2]), float(v[3]))) is None
              for (px, py), v in zip(np.repeat(pixels, 2, axis=0), vec)]
    assert 5 < sum(missed) < len(missed) - 5


# ---- 5. the traversal kernel does not matter ----
def _with_option(name, value, fn):
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(name.encode(), str(value).encode()))
        return fn()
    finally:
        lib.dr_set_option(name.encode(), None)


@pytest.mark.parametrize("impl", ["2", "3", "5f"])
def test_every_traversal_kernel_gives_the_same_film(yard, impl):
    want = yard.restated_film((256,), _ld(yard), "ld")[0]
    got = _with_option("TRACE_IMPL", impl, lambda: yard.device_film((256,), _ld(yard)))
    assert _same(got, want)


@pytest.mark.parametrize("layout", [64, 4])
def test_both_state_layouts_give_the_same_film(yard, layout):
    want = yard.restated_film((256,), _ld(yard), "ld")[0]

    def run():
        film = yard.device_film((256,), _ld(yard))
        return film, yard.scene._device().last_render_info()
    got, info = _with_option("STATE_LAYOUT", layout, run)
    assert info["state_layout"] == layout and _same(got, want)


# ---- 5b. every branch of the camera hit's geometry: quadric, triangle with per-vertex N, plain triangle ----
@pytest.fixture(scope="module")
def yard_n(gpu):
    return Setup(leaning=True)


@pytest.mark.parametrize("layout", [64, 4])
def test_a_mesh_with_vertex_normals_among_the_camera_hits(yard_n, layout):
    want, pixels, vec = yard_n.restated_film((4,), _ld(yard_n), "ld")
    rcam = mrf.restated_camera(yard_n.camera)
    hits = [yard_n.restated.bvh.intersect(rcam.generateRay(int(px) + float(v[0]), int(py) + float(v[1]), float(v[2]), float(v[3])))
            for (px, py), v in zip(np.repeat(pixels, 2, axis=0), vec)]
    on_mesh = sum(h is not None and abs(h.dg.p.y - (h.dg.p.z + 2.7)) < 1e-3 and 0.2 < h.dg.p.y < 1.2 for h in hits)   # the leaning quad's plane y = z + 2.7
    on_sphere = sum(h is not None and isinstance(h.prim.shape, ao.dr.Sphere) for h in hits)
    on_floor = sum(h is not None and h.dg.p.y == 0.0 for h in hits)
    print("camera hits: %d on the mesh with N, %d on the sphere, %d on the floor" % (on_mesh, on_sphere, on_floor))
    assert on_mesh >= 2 and on_sphere >= 2 and on_floor >= 2
    flags = yard_n.accel.tri_shading
    assert flags is not None and (flags & 1).any() and (flags == 0).any()   # DR_SHADING_N on the mesh's triangles, no record on the others

    def run():
        return yard_n.device_film((4,), _ld(yard_n)), yard_n.scene._device().last_render_info()
    got, info = _with_option("STATE_LAYOUT", layout, run)
    assert info["state_layout"] == layout and _same(got, want)


# ---- 6. what ran ----
def test_last_render_info_names_the_integrator_and_its_kernel(yard):
    r = yard.renderer(core.AmbientOcclusionIntegrator(256), _ld(yard))
    r.render(yard.scene)
    info = yard.scene._device().last_render_info()
    assert info["integrator"] == "ambientocclusion" and info["shade_kernels"] == ["k_shade_ao"]
    st = r.last_stats
    hits = st["shade_vertices"]
    assert st["camera_samples"] == 81 * 2 and 0 < hits <= 81 * 2
    assert st["any_rays"] == hits * 256 and st["any_launches"] == 256  # every hit sends every ray, one any-hit launch per ray index
    assert st["closest_launches"] == 1                                 # the camera rays, once: no later round traces them again
    # another integrator's render: the word is -1 again
    core.SamplerRenderer(_ld(yard), yard.camera, core.DirectLightingIntegrator(0, 5), core.EmissionIntegrator()).render(yard.scene)
    info = yard.scene._device().last_render_info()
    assert info["integrator"] is None and info["shade_kernels"] == []


# ---- 7. the host-buffer replay of the dumped vectors ----
def test_host_buffer_replay_of_the_dumped_vectors(yard):
    want, pixels, vec = yard.restated_film((256,), _ld(yard), "ld")
    r = yard.renderer(core.AmbientOcclusionIntegrator(256), core.HostBufferSampler(yard.camera, 2, pixels, vec, seed=SEED))
    got = r.render(yard.scene).film
    assert _same(got, yard.device_film((256,), _ld(yard))) and _same(got, want)


# ---- 8. the refusals, by name ----
def test_refusals_by_name_leave_the_scene_usable(yard):
    lib = _abi.lib()
    film = np.zeros((8, 8, 4), np.float32)

    def refused(code, needle, mutate):
        d, keep = yard.renderer(core.AmbientOcclusionIntegrator(8), _ld(yard)).describe()
        mutate(d)
        rc = lib.dr_render(yard.scene._device().handle, C.byref(d), film.ctypes.data, None)
        assert rc == code, rc
        assert needle in lib.dr_last_error().decode(), lib.dr_last_error()

    for n in (0, -5):
        refused(-1, "ambient occlusion integrator: nsamples must be at least 1", lambda d: setattr(d, "ao_nsamples", n))
    refused(-1, "ambient occlusion integrator: nsamples above 4096 after rounding", lambda d: setattr(d, "ao_nsamples", 4097))
    refused(-1, "ambient occlusion integrator: mindist must not be negative", lambda d: setattr(d, "ao_mindist", -1.0e-3))
    refused(-1, "ambient occlusion integrator: maxdist must be greater than mindist", lambda d: setattr(d, "ao_maxdist", 1.0e-4))

    def adaptive(d):
        d.sampler_mode, d.spp, d.strat_xsamples = _abi.DR_SAMPLER_ADAPTIVE, 8, 2
    refused(-4, "ambient occlusion integrator: the adaptive sampler is not supported", adaptive)
    # a count that is no power of two is rounded up by the library as by the constructor
    d, keep = yard.renderer(core.AmbientOcclusionIntegrator(8), _ld(yard)).describe()
    d.ao_nsamples = 5
    _abi.check(lib.dr_render(yard.scene._device().handle, C.byref(d), film.ctypes.data, None))
    assert _same(film, yard.restated_film((8,), _ld(yard), "ld")[0])
