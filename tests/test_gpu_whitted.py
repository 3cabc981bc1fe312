"""WhittedIntegrator on the GPU (DR_INTEGRATOR_WHITTED, k_shade_whitted), bit for bit against the Python restatement
(tests/whitted_restatement.py) fed the device sampler's own vectors (dr_generate_samples) and the keyed in-Li streams read in order.
8 x 8 images (a 9 x 9 sampler window) at 2 and 4 samples per pixel; a restated film is computed once per configuration and shared.
Nothing is started after a failed call: every call's return code raises."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt, scenes

import prt_restatement as prt
import table_placement as tp
import whitted_restatement as wr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 5489
T = pbrt.Transform


def _quad(p0, p1, p2, p3, material, light=None):
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([p0, p1, p2, p3], np.float32))
    return core.GeometricPrimitive(mesh, material, light)


def _leaning():
    """A tilted matte quad near the floor in front of the glass with per-vertex N that lean away from its plane: a shading record with
    DR_SHADING_N, so its BSDF is built on Triangle.getShadingGeometry's frame."""
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([(2.5, -9.5, -4.0), (2.5, -6.0, -0.5), (6.0, -6.0, -0.5), (6.0, -9.5, -4.0)], np.float32),
                             n=np.array([(0.3, 0.7, -0.6), (-0.2, 0.9, -0.3), (-0.3, 0.8, -0.5), (0.4, 0.6, -0.7)], np.float32))
    return core.GeometricPrimitive(mesh, core.MatteMaterial((0.6, 0.5, 0.4)), None)


def _prims(sphere=True, area=True, specular=True, leaning=False, emitter=None, floor=None):
    """A closed box of matte quads (the camera is inside) with one emissive triangle under the ceiling, a mirror quad in front of the
    left wall, a glass sphere and a glass triangle mesh.  emitter: a primitive in the emissive triangle's place; floor: a list of
    primitives in the floor quad's place."""
    s = 10.0
    white = core.MatteMaterial((0.75, 0.75, 0.75))
    prims = scenes.cornell_walls() + [_quad((-s, -s, -s), (-s, s, -s), (s, s, -s), (s, -s, -s), white)]  # + the wall behind the camera
    if floor is not None:
        prims = prims[1:] + list(floor)
    if emitter is not None:
        prims.append(emitter)
    elif area:
        tri = core.TriangleMesh(np.array([[0, 1, 2]], np.uint32), np.array([(-3, 9.5, -2), (3, 9.5, -2), (0, 9.5, 4)], np.float32))
        prims.append(core.GeometricPrimitive(tri, core.MatteMaterial((0.5, 0.5, 0.5)), core.DiffuseAreaLight((40.0, 36.0, 30.0), 1)))
    if specular:
        prims.append(_quad((-9.0, -6.0, 8.0), (-9.0, 5.0, 8.0), (-6.0, 5.0, 0.0), (-6.0, -6.0, 0.0), core.MirrorMaterial((0.9, 0.85, 0.8))))
        prims.append(core.GeometricPrimitive(scenes.blob_mesh(8, 4, radius=2.6, centre=(4.5, -5.5, 3.0)),
                                             core.GlassMaterial((1.0, 1.0, 1.0), (0.95, 1.0, 0.9), 1.5)))
        if sphere:
            at = T.Translate(-1.0, -6.5, 2.0)
            prims.append(core.GeometricPrimitive(core.Sphere(at.m, at.mInv, False, 3.0), core.GlassMaterial((1.0, 1.0, 1.0), (1.0, 0.95, 0.9), 1.5)))
    if leaning:
        prims.append(_leaning())
    return prims


def _delta_lights():
    """-> ([core lights], [restated lights]): a point light and a spot light that points down and a little forward."""
    pt = T.Translate(5.0, 6.0, -4.0)
    sp = T.Translate(-4.0, 8.0, 2.0) * T.Rotate(80.0, 1.0, 0.0, 0.0)
    point = core.PointLight(pt.m, (300.0, 260.0, 220.0))
    spot = core.SpotLight(sp.m, (500.0, 600.0, 700.0), 40.0, 25.0, sp.mInv)
    rp = wr.PointLight(tuple(float(v) for v in point.lightPos), tuple(float(v) for v in point.intensity))
    rs = wr.SpotLight(tuple(float(v) for v in spot.lightPos), tuple(float(v) for v in spot.intensity), spot.worldToLight.reshape(-1), 40.0, 25.0)
    return [point, spot], [rp, rs]


def _constant_env():
    """The 4 x 2 constant map of the environment tests."""
    return core.InfiniteAreaLight(None, (1.0, 1.0, 1.0), 1, np.full((2, 4, 3), (0.5, 0.6, 0.9), np.float32))


class Setup:
    """One scene on both sides: `scene` for the device, `restated` for tests/whitted_restatement.py; lights in the same order (area
    lights, the point light, the spot light, the infinite light)."""

    def __init__(self, env=False, **kw):
        prims = _prims(**kw)
        lights, restated_lights = _delta_lights()
        self.env = _constant_env() if env else None
        if env:  # open the box: no ceiling, so that camera and child rays escape
            assert kw.get("floor") is None
            prims = [p for i, p in enumerate(prims) if i != 1]
        accel = core.BVHAccel(prims)
        self.scene = core.Scene(accel, accel.lights() + lights + ([self.env] if env else []))
        self.restated = mrf.build_scene(prims, None)
        if kw.get("leaning"):
            prt.with_shading_geometry(self.restated, accel)
        self.restated.lights += restated_lights
        if env:
            e = self.env
            texels = [tuple(float(c) for c in e.texels[y, x]) for y in range(2) for x in range(4)]
            self.restated.lights.append(wr.dr.InfiniteAreaLight(e.lightToWorld.reshape(-1), e.worldToLight.reshape(-1), tuple(float(c) for c in e.L), texels, 4, 2))
        film = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
        self.camera = core.PerspectiveCamera.lookAt((0.5, -1.0, -9.5), (0.0, -3.0, 2.0), (0.0, 1.0, 0.0), 70.0, film)
        self.films = {}

    def renderer(self, maxDepth, sampler):
        return core.SamplerRenderer(sampler, self.camera, core.WhittedIntegrator(maxDepth), core.EmissionIntegrator())

    def restated_film(self, maxDepth, sampler, key):
        """The restatement's film for the vectors the device sampler `sampler` generates (cached under `key`)."""
        if (maxDepth, key) not in self.films:
            r = self.renderer(maxDepth, sampler)
            pixels = r.pixels()
            vec = r.generate_samples(self.scene, pixels)
            assert vec.shape == (len(pixels) * sampler.samplesPerPixel, 7)  # image, lens, time, tau, scatter: no light or BSDF blocks
            ext = wr.rr.sample_extent(self.camera.film)
            self.films[(maxDepth, key)] = (wr.render(self.restated, mrf.restated_camera(self.camera), self.camera.film, maxDepth,
                                                     sampler.samplesPerPixel, pixels, vec, wr.keyed_rng(SEED, ext)), pixels, vec)
        return self.films[(maxDepth, key)]


@pytest.fixture(scope="module")
def box(gpu):
    return Setup()


@pytest.fixture(scope="module")
def open_box(gpu):
    return Setup(env=True)


def _ld(s, spp):
    return core.LowDiscrepancySampler(s.camera, spp, SEED)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- 1. the film against the restatement ----
@pytest.mark.parametrize("maxDepth,spp", [(1, 2), (2, 2), (5, 2), (5, 4)])
def test_film_equals_the_restatement(box, maxDepth, spp):
    want, pixels, vec = box.restated_film(maxDepth, _ld(box, spp), "ld%d" % spp)
    assert len(pixels) == 81
    got = box.renderer(maxDepth, _ld(box, spp)).render(box.scene).film
    assert np.isfinite(got).all() and got[..., :3].max() > 0.0
    assert _same(got, want)


def test_depth_changes_the_image(box):
    """The mirror and the glass show: each depth adds radiance somewhere."""
    f = {d: box.restated_film(d, _ld(box, 2), "ld2")[0] for d in (1, 2, 5)}
    assert not _same(f[1], f[2]) and not _same(f[2], f[5])


# ---- 1b. both forms of the kernel: light tables in LDS and in global memory ("Where the tables live") ----
@pytest.fixture(scope="module")
def table_sizes(gpu):
    """(the largest fan for which k_shade_whitted<true> runs, the smallest for which k_shade_whitted<false> does, the tile count one over
    the material cap), by tests/table_placement.py's formula from the counts of the box with a fan of two triangles over its floor quad."""
    c = tp.table_counts(Setup(emitter=tp.fan_emitter(2)).scene)
    n_lds, n_global = tp.fan_sizes(c, "whitted", 2)
    k_over = 1 + max(k for k in range(1, 1000) if tp.mat_table_bytes(tp.with_tiles(c, k, 1)))
    return c, n_lds, n_global, k_over


_placed = {}


@pytest.mark.parametrize("case", ["fan_smallest-global", "fan_largest-lds", "tiles_over_cap-lds_lights_global_mats"])
def test_film_equals_the_restatement_on_both_sides_of_the_table_caps(table_sizes, case):
    """The restatement walks every light triangle in Python: the fan stays at the two sizes next to the cap, at 2 samples per pixel and
    maxDepth 2, and each configuration's restated film is computed once."""
    c, n_lds, n_global, k_over = table_sizes
    what, want = case.split("-")
    if case not in _placed:
        _placed[case] = {"fan_smallest": lambda: Setup(emitter=tp.fan_emitter(n_global)), "fan_largest": lambda: Setup(emitter=tp.fan_emitter(n_lds)),
                         "tiles_over_cap": lambda: Setup(emitter=tp.fan_emitter(2), floor=tp.tiled_floor(k_over))}[what]()
    s = _placed[case]
    counts = {"fan_smallest": tp.with_fan(c, n_global, 2), "fan_largest": tp.with_fan(c, n_lds, 2), "tiles_over_cap": tp.with_tiles(c, k_over, 1)}[what]
    assert tp.table_counts(s.scene) == counts and n_global == n_lds + 1
    assert tp.placement(s.scene, "whitted") == want
    want_film = s.restated_film(2, _ld(s, 2), "ld2")[0]
    got = s.renderer(2, _ld(s, 2)).render(s.scene).film
    assert np.isfinite(got).all() and got[..., :3].max() > 0.0
    assert _same(got, want_film)


# ---- 2. the infinite light: an escaped child ray adds Le ----
@pytest.mark.parametrize("maxDepth", [1, 5])
def test_film_under_the_infinite_light(open_box, maxDepth):
    want = open_box.restated_film(maxDepth, _ld(open_box, 2), "ld2")[0]
    got = open_box.renderer(maxDepth, _ld(open_box, 2)).render(open_box.scene).film
    assert _same(got, want)


# ---- 3. the host-buffer replay of the dumped vectors ----
def test_host_buffer_replay_of_the_dumped_vectors(box):
    want, pixels, vec = box.restated_film(5, _ld(box, 2), "ld2")
    r = box.renderer(5, core.HostBufferSampler(box.camera, 2, pixels, vec, seed=SEED))
    assert _same(r.render(box.scene).film, want)


# ---- 4. the other device samplers ----
@pytest.mark.parametrize("name", ["stratified", "stratified_nojitter", "random"])
def test_other_samplers_equal_the_restatement_fed_their_vectors(box, name):
    mk = {"stratified": lambda: core.StratifiedSampler(box.camera, 2, 2, True, SEED),
          "stratified_nojitter": lambda: core.StratifiedSampler(box.camera, 2, 2, False, SEED),
          "random": lambda: core.RandomSampler(box.camera, 4, SEED)}[name]
    want = box.restated_film(2, mk(), name)[0]
    got = box.renderer(2, mk()).render(box.scene).film
    assert _same(got, want)
    assert not _same(want, box.restated_film(2, _ld(box, 2), "ld2")[0])


def test_halton_sampler_against_the_restatement(box):
    """The Halton sampler's samples belong to the image: one slot per accepted index k, the in-Li stream keyed (seed, k, 0, kind 2), and
    a film that atomics add in no fixed order.  So: the dumped 7-float vectors equal the Halton restatement's, and the film lies within
    tests/film_reference.py's derived bound of the f64 sum of the Whitted restatement's radiances (weights: bit equal, integer table)."""
    import film_reference as fr
    import halton_restatement as hr
    film = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
    film.filterTable[:] = fr.INT_TABLE
    cam = core.PerspectiveCamera.lookAt((0.5, -1.0, -9.5), (0.0, -3.0, 2.0), (0.0, 1.0, 0.0), 70.0, film)
    r = core.SamplerRenderer(core.HaltonSampler(cam, 2, SEED), cam, core.WhittedIntegrator(5), core.EmissionIntegrator())
    k, xy, vec = r.generate_halton_samples(box.scene)
    want = hr.keyed(hr.task_window(film), 2, SEED, [1, 1], [], 0)
    assert len(k) > 100 and np.array_equal(k, want.k) and np.array_equal(xy, want.pixel_xy)
    assert vec.shape == want.vec.shape == (len(k), 7) and _same(vec, want.vec)
    rcam = mrf.restated_camera(cam)
    Ls = np.array([wr.sample_Li(box.restated, rcam, int(px), int(py), v, wr.rr.RNG(wr.rr.counter_key(SEED, int(kk), 0, wr.rr.LI_KIND)), 5)[0].tuple()
                   for kk, (px, py), v in zip(k, xy, vec)], np.float32)
    ref = fr.reference_from_samples(film, xy, 1, vec[:, 0], vec[:, 1], Ls, serial=False)
    got = r.render(box.scene).film
    assert np.array_equal(got[..., 3].astype(np.float64), ref.sum[..., 3])
    err, lim = np.abs(got.astype(np.float64) - ref.sum), fr.bound(ref.S, ref.n)
    print("max |device - f64 sum| / bound = %.3g" % float((err[..., :3] / np.maximum(lim[..., :3], 1e-300)).max()))
    assert (err <= lim).all() and np.isfinite(got).all() and got[..., :3].max() > 0


# ---- 5. / 6. the traversal kernel and the state layout do not matter ----
def _with_option(name, value, fn):
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(name.encode(), str(value).encode()))
        return fn()
    finally:
        lib.dr_set_option(name.encode(), None)


@pytest.mark.parametrize("impl", ["2", "3", "5", "2f", "3f", "5f"])
def test_every_traversal_kernel_gives_the_same_film(box, impl):
    want = box.restated_film(5, _ld(box, 2), "ld2")[0]
    got = _with_option("TRACE_IMPL", impl, lambda: box.renderer(5, _ld(box, 2)).render(box.scene).film)
    assert _same(got, want)


@pytest.fixture(scope="module")
def triangles_only(gpu):
    """The same box without the sphere: a scene of triangles alone, which the sibling-pair traversal kernels can take."""
    s = Setup(sphere=False)
    return s, s.renderer(5, _ld(s, 2)).render(s.scene).film


@pytest.mark.parametrize("impl", ["2", "3", "5", "3f"])
def test_every_traversal_kernel_on_triangles_alone(triangles_only, impl):
    s, ref = triangles_only

    def run():
        film = s.renderer(5, _ld(s, 2)).render(s.scene).film
        return film, s.scene._device().last_render_info()
    got, info = _with_option("TRACE_IMPL", impl, run)
    assert info["closest_kernel"] == int(impl[0]) and _same(got, ref)
    if impl == "2":
        assert _same(got, s.restated_film(5, _ld(s, 2), "ld2")[0])


@pytest.mark.parametrize("layout", [64, 4])
def test_both_state_layouts_give_the_same_film(box, layout):
    want = box.restated_film(5, _ld(box, 2), "ld2")[0]

    def run():
        film = box.renderer(5, _ld(box, 2)).render(box.scene).film
        return film, box.scene._device().last_render_info()
    got, info = _with_option("STATE_LAYOUT", layout, run)
    assert info["state_layout"] == layout and _same(got, want)


@pytest.fixture(scope="module")
def box_n(gpu):
    """The box with the leaning quad: with the walls' plain triangles and the glass sphere, every branch of the hit geometry."""
    return Setup(leaning=True)


@pytest.mark.parametrize("layout", [64, 4])
def test_a_mesh_with_vertex_normals_among_the_hits(box_n, layout, monkeypatch):
    """The restatement builds its BSDF on Triangle.getShadingGeometry's frame (tests/prt_restatement.py's getBSDF over
    tests/feature_restatement.py's Triangle); every other shape keeps the geometric frame, as before."""
    monkeypatch.setattr(wr, "getBSDF", prt.getBSDF)
    want, pixels, vec = box_n.restated_film(2, _ld(box_n, 2), "ld2")
    rcam = mrf.restated_camera(box_n.camera)
    hits = [box_n.restated.bvh.intersect(rcam.generateRay(int(px) + float(v[0]), int(py) + float(v[1]), float(v[2]), float(v[3])))
            for (px, py), v in zip(np.repeat(pixels, 2, axis=0), vec)]
    on = [sum(h is not None and isinstance(h.prim.shape, cls) for h in hits) for cls in (wr.dr.Sphere, prt.fe.Triangle)]
    on.append(sum(h is not None and type(h.prim.shape) is wr.dr.Triangle for h in hits))
    print("camera hits: %d on the sphere, %d on the mesh with N, %d on plain triangles" % tuple(on))
    assert min(on) >= 2
    for h in hits:
        if h is not None and isinstance(h.prim.shape, prt.fe.Triangle):
            assert prt.Dot(prt.getBSDF(h).nn, h.dg.nn) < 0.999   # the shading normal is not the geometric one

    def run():
        film = box_n.renderer(2, _ld(box_n, 2)).render(box_n.scene).film
        return film, box_n.scene._device().last_render_info()
    got, info = _with_option("STATE_LAYOUT", layout, run)
    assert info["state_layout"] == layout and _same(got, want)


# ---- 7. parity with DirectLighting where the two agree by construction ----
def test_delta_lights_on_matte_surfaces_equal_direct_lighting_all(gpu):
    """Delta lights only, matte surfaces only, maxdepth 1.  EstimateDirect's light half for a delta light is
    `Ld += f * Li * (AbsDot(wi, n) / lightPdf)` with lightPdf = 1 (integrator.dart:146-150), Whitted's is
    `L += f * Li * AbsDot(wi, n) * T / pdf` with T = 1 and pdf = 1 (whitted_integrator.dart:57-58): x / 1 and x * 1 are exact, so both
    store f32(f32(f * Li) * AbsDot); the BSDF half is skipped for a delta light; and with Le = 0 the sums 0 + (0 + X1 / 1 + X2 / 1) and
    (0 + X1) + X2 round alike.  No operator order in the two texts breaks bit equality."""
    s = Setup(area=False, specular=False)
    a = s.renderer(1, _ld(s, 4)).render(s.scene).film
    r = core.SamplerRenderer(_ld(s, 4), s.camera, core.DirectLightingIntegrator(0, 1), core.EmissionIntegrator())
    b = r.render(s.scene).film
    assert a[..., :3].max() > 0.0 and _same(a, b)


# ---- 8. the refusals, by name ----
def test_refusals_by_name_leave_the_scene_usable(box):
    lib = _abi.lib()
    film = np.zeros((8, 8, 4), np.float32)

    def refused(r, code, needle, mutate=None):
        d, keep = r.describe()
        if mutate:
            mutate(d)
        rc = lib.dr_render(box.scene._device().handle, C.byref(d), film.ctypes.data, None)
        assert rc == code, rc
        assert needle in lib.dr_last_error().decode(), lib.dr_last_error()

    for depth in (0, -1):
        refused(box.renderer(5, _ld(box, 2)), -1, "whitted integrator: max_depth must be at least 1", lambda d: setattr(d, "max_depth", depth))
    refused(box.renderer(5, core.AdaptiveSampler(box.camera, 2, 8, "contrast", SEED)), -4, "whitted integrator: the adaptive sampler is not supported")
    assert _same(box.renderer(5, _ld(box, 2)).render(box.scene).film, box.restated_film(5, _ld(box, 2), "ld2")[0])


# ---- 9. what ran ----
def test_last_render_info_names_the_integrator_and_its_kernels(box):
    r = box.renderer(5, _ld(box, 2))
    r.render(box.scene)
    info = box.scene._device().last_render_info()
    assert info["integrator"] == "whitted" and info["shade_kernels"] == ["k_shade_whitted", "k_shade_spec"]
    st = r.last_stats
    assert st["camera_samples"] == 81 * 2 and st["shade_vertices"] >= 81 * 2 and st["any_rays"] > 0
    # a scene without mirror / glass: no specular rounds; another integrator's render: the word is -1 again
    plain = Setup(specular=False)
    plain.renderer(5, _ld(plain, 2)).render(plain.scene)
    assert plain.scene._device().last_render_info()["shade_kernels"] == ["k_shade_whitted"]
    core.SamplerRenderer(_ld(plain, 2), plain.camera, core.DirectLightingIntegrator(0, 5), core.EmissionIntegrator()).render(plain.scene)
    info = plain.scene._device().last_render_info()
    assert info["integrator"] is None and info["shade_kernels"] == []
