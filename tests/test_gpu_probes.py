"""Radiance probes on the GPU: the four stages of the bake (dr_probes.hip) and UseProbesIntegrator's films (k_shade_probes), bit for
bit against tests/probes_restatement.py.  The scene: a closed room (12 triangles) with a closed solid box in a thin closed shell inside it (24 more),
a leaning quad with per-vertex N for the films; npoints 96.  Restated results are computed once per configuration and shared.  Nothing is started after a failed
call: every call's return code raises."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt

import probes_restatement as pr
import prt_restatement as prt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, NPOINTS = 5489, 96
T = pbrt.Transform
# the candidates' grid: 2 x 2 x 1 cells (binary fractions: delta / spacing is exact).  The solid box is [0, 1] x [0, 1.125] x [0, 1] inside a closed
# shell 0.01 larger: a surface point ON a closed box sees into it -- the ray starts behind the face it lies on -- so under the reference only a
# box that no walk reaches is solid, and the walks reach the shell.  Cell 0 lies wholly inside the box, cell 1 straddles its face x = 1, cells 2
# and 3 lie above the shell's top y = 1.135 (the lowest of their first 32 candidates is at 1.125 + 1 / 81)
GRID_BOUNDS, GRID_SPACING = (0.125, 0.125, 0.125, 1.625, 2.125, 0.875), 1.0


def _quad(p0, p1, p2, p3, kd=(0.5, 0.5, 0.5), light=None, **kw):
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([p0, p1, p2, p3], np.float32), **kw)
    if light is not None:
        light = core.DiffuseAreaLight(light[0], light[1], mesh)
    return core.GeometricPrimitive(mesh, core.MatteMaterial(kd), light)


def _box(x0, y0, z0, x1, y1, z1, kd):
    c = lambda x, y, z: (x, y, z)
    return [_quad(c(x0, y0, z0), c(x1, y0, z0), c(x1, y0, z1), c(x0, y0, z1), kd), _quad(c(x0, y1, z0), c(x0, y1, z1), c(x1, y1, z1), c(x1, y1, z0), kd),
            _quad(c(x0, y0, z0), c(x0, y1, z0), c(x1, y1, z0), c(x1, y0, z0), kd), _quad(c(x0, y0, z1), c(x1, y0, z1), c(x1, y1, z1), c(x0, y1, z1), kd),
            _quad(c(x0, y0, z0), c(x0, y0, z1), c(x0, y1, z1), c(x0, y1, z0), kd), _quad(c(x1, y0, z0), c(x1, y1, z0), c(x1, y1, z1), c(x1, y0, z1), kd)]


LEANING = ((-2.5, 0.2, -2.5), (-2.5, 1.2, -1.5), (-0.3, 1.2, -1.5), (-0.3, 0.2, -2.5))
LEANING_N = np.array([(0.3, 0.7, -0.6), (-0.2, 0.9, -0.3), (-0.3, 0.8, -0.5), (0.4, 0.6, -0.7)], np.float32)
EMITTER = ((-2.0, 2.9, -1.0), (0.5, 2.9, -1.0), (0.5, 2.9, 1.0), (-2.0, 2.9, 1.0))   # under the ceiling, facing down


def _prims(emitter=None, leaning=False, ceiling=True):
    room = _box(-3.0, 0.0, -3.0, 3.0, 3.0, 3.0, (0.5, 0.6, 0.7))
    if not ceiling:   # (the distant and the infinite light shine in from above)
        del room[1]
    p = room + _box(0.0, 0.0, 0.0, 1.0, 1.125, 1.0, (0.7, 0.4, 0.3)) + _box(-0.01, 0.0, -0.01, 1.01, 1.135, 1.01, (0.7, 0.4, 0.3))
    if emitter:
        p.append(_quad(*EMITTER, light=((6.0, 5.0, 4.0), emitter)))
    if leaning:
        p.append(_quad(*LEANING, kd=(0.6, 0.5, 0.4), n=LEANING_N))
    return p


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
    """One scene on both sides (tests/test_gpu_prt.py's): the device's lights are the area lights, the infinite light, then the delta lights."""

    def __init__(self, prims, env=None, delta=(), eye=(-1.5, 1.5, -2.5), look=(0.5, 0.5, 0.5)):
        accel = core.BVHAccel(prims)
        self.scene = core.Scene(accel, accel.lights() + ([env] if env is not None else []) + list(delta))
        self.restated = prt.with_shading_geometry(mrf.build_scene(prims, env), accel)
        for rl, cl in zip(self.restated.lights, accel.lights()):
            rl.nSamples = cl.nSamples
        for rl in self.restated.lights:   # (nor does the restated infinite light)
            if isinstance(rl, prt.dr.InfiniteAreaLight):
                rl.nSamples = env.nSamples
        self.restated.lights = list(self.restated.lights) + [_restated_delta(L) for L in delta]
        film = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
        self.camera = core.PerspectiveCamera.lookAt(eye, look, (0.0, 1.0, 0.0), 70.0, film)
        self.eye = prt.Vec(*[float(np.float32(v)) for v in eye])
        self.r = core.SamplerRenderer(core.LowDiscrepancySampler(self.camera, 1, SEED), self.camera, core.UseProbesIntegrator(), core.EmissionIntegrator())
        self._pts, self._acc = None, {}

    def points(self):
        if self._pts is None:
            self._pts = pr.surface_points(self.restated, self.eye, NPOINTS)
        return self._pts

    def accepted(self, cell):
        if cell not in self._acc:
            n, b = pr.make_grid(self.restated, GRID_SPACING, GRID_BOUNDS)
            self._acc[cell] = pr.accept(self.restated, n, b, cell, self.points()[0])
        return self._acc[cell]


def _pts_array(pts):
    return np.array([(p.x, p.y, p.z) for p in pts], np.float32)


# ---- 1. surface points ----
@pytest.fixture(scope="module")
def room(gpu):
    return Setup(_prims())


def test_surface_points_camera_inside_the_bounding_sphere(room):
    pts, walks = room.points()
    assert all(h == 32 for h in walks) and len(pts) == 1 + 32 * len(walks) == 97   # the closed room: every walk is full; the overshoot
    got = room.r.probes_surface_points(room.scene, NPOINTS)
    assert got.shape == (len(pts), 3) and _same(got, _pts_array(pts))


def test_surface_points_camera_outside_looking_past_the_scene(gpu):
    s = Setup(_prims(), eye=(10.0, 1.5, 0.5), look=(10.0, 1.5, 9.0))
    pts, walks = s.points()
    assert any(h < 32 for h in walks) and any(h > 0 for h in walks)   # walks that miss both the scene and its bounding sphere break at once
    got = s.r.probes_surface_points(s.scene, NPOINTS)
    print("outside: %d walks, %d short, %d points" % (len(walks), sum(h < 32 for h in walks), len(pts)))
    assert got.shape == (len(pts), 3) and _same(got, _pts_array(pts))


# ---- 2. candidates ----
def test_candidates_inside_straddling_and_open_cells(room):
    n, b = pr.make_grid(room.restated, GRID_SPACING, GRID_BOUNDS)
    assert n == [2, 2, 1]
    want = [room.accepted(c) for c in range(4)]
    inside, straddle, open_ = want[0], want[1], want[3]
    assert inside[0] == [] and len(inside[1]) == 256 and not any(inside[1])                  # wholly inside the solid box: all 256 tried, none accepted
    assert 0 < len(straddle[0]) and not all(straddle[1][:straddle[0][-1]])                   # some candidate before the last accepted one is rejected
    assert open_[0] == list(range(32))                                                        # open: the first 32 candidates
    nfound, acc = room.r.probes_candidates(room.scene, _pts_array(room.points()[0]), GRID_SPACING, GRID_BOUNDS)
    for c in range(4):
        assert nfound[c] == len(want[c][0]) and list(acc[c][:nfound[c]]) == want[c][0] and (acc[c][nfound[c]:] == -1).all()


# ---- 3. the bake ----
def _env_map(w, h):
    rng = np.random.RandomState(w * 131 + h)
    return rng.uniform(0.05, 2.0, size=(h, w, 3)).astype(np.float32)


def _light_case(name):
    pt, sp = T.Translate(1.6, 2.5, -1.0), T.Translate(2.0, 2.8, 0.5) * T.Rotate(90.0, 1.0, 0.0, 0.0)
    point, spot = lambda: core.PointLight(pt.m, (30.0, 26.0, 22.0)), lambda: core.SpotLight(sp.m, (50.0, 60.0, 70.0), 60.0, 25.0, sp.mInv)
    env = lambda: core.InfiniteAreaLight(T.Rotate(30.0, 0.2, 1.0, 0.1).m, (1.0, 0.7, 0.5), 4, _env_map(4, 2))
    distant = lambda: core.DistantLight(None, (1.5, 2.0, 2.5), (0.3, 1.0, -0.2))
    if name == "point":
        return Setup(_prims(), None, [point()])
    if name == "spot":
        return Setup(_prims(), None, [spot()])
    if name == "distant":
        return Setup(_prims(ceiling=False), None, [distant()])
    if name in ("area1", "area4"):
        return Setup(_prims(emitter=int(name[4:])))
    if name == "env4x2":
        return Setup(_prims(ceiling=False), env())
    # every kind together: the scramble groups of a candidate are indexed by the light's place among the FOUR non-point lights (area, infinite,
    # spot, distant), with the point light, which draws nothing, between them
    assert name == "together"
    return Setup(_prims(emitter=4, ceiling=False), env(), [distant(), point(), spot()])


def _check_bake(s, lmax):
    want = pr.bake(s.restated, s.eye, lmax, GRID_SPACING, GRID_BOUNDS, NPOINTS)
    got = s.r.create_probes(s.scene, lmax, GRID_SPACING, GRID_BOUNDS, npoints=NPOINTS)
    assert got.data.shape == want.shape == (15 + 4 * (lmax + 1) ** 2 * 3,) and np.isfinite(got.data).all()
    print("lmax %d: max |device - restatement| = %.3g of %.3g" % (lmax, float(np.abs(got.data - want).max()), float(np.abs(want[12:]).max())))
    assert _same(got.data[:12], want[:12]) and (got.data[-3:] == 0).all()
    assert _same(got.data, want)
    return got


@pytest.mark.parametrize("name", ["point", "spot", "distant", "area1", "area4", "env4x2"])
def test_bake_equals_the_restatement_one_light_at_a_time(gpu, name):
    g = _check_bake(_light_case(name), 2)
    assert (g.coefficients[0].view(np.uint32) == 0).all()   # the cell inside the solid box: nFound 0, exactly +0, no division
    assert np.abs(g.coefficients[3]).max() > 0.0            # ... and the light reaches the open cell


@pytest.fixture(scope="module")
def together(gpu):
    return _light_case("together")


@pytest.mark.parametrize("lmax", [1, 2, 4])
def test_bake_equals_the_restatement_all_lights_together(together, lmax):
    g = _check_bake(together, lmax)
    assert (g.coefficients[0].view(np.uint32) == 0).all() and np.abs(g.coefficients[3]).max() > 0.0


# A blocker between a point light and the cell behind it; a spot light beside the other cell, whose cone does not reach the first
SHADOW_BOUNDS, SHADOW_SPACING = (-2.0, 0.5, -0.5, 2.0, 1.5, 0.5), 2.0   # 2 x 1 x 1 cells: x in [-2, 0] behind the blocker, x in [0, 2] in front


def _shadow_case(blocker_y):
    pt, sp = T.Translate(0.0, 2.8, 0.0), T.Translate(2.0, 2.8, 0.5) * T.Rotate(90.0, 1.0, 0.0, 0.0)
    blocker = _quad((-2.5, blocker_y, -1.0), (-2.5, blocker_y, 1.0), (-0.5, blocker_y, 1.0), (-0.5, blocker_y, -1.0))
    return Setup(_box(-3.0, 0.0, -3.0, 3.0, 3.0, 3.0, (0.5, 0.6, 0.7)) + [blocker], None,
                 [core.PointLight(pt.m, (30.0, 26.0, 22.0)), core.SpotLight(sp.m, (50.0, 60.0, 70.0), 60.0, 25.0, sp.mInv)])


def test_moving_the_blocker_changes_the_cell_behind_it_only(gpu):
    """lmax 2.  The blocker hangs at y = 2 between the point light at (0, 2.8, 0) and most of cell 0; moved down to y = 0.05 it lies under both
    cells and shadows neither.  Cell 1's segments to the two lights cross neither position, so it keeps its bytes; cell 0 changes, and its band-0
    coefficient -- a sum of non-negative radiances times Y_00 -- is smaller under the blocker: the visibility rays shadow.  All of it is asserted
    from the restatement before the device is looked at."""
    hung, moved = _shadow_case(2.0), _shadow_case(0.05)
    want = [pr.bake(s.restated, s.eye, 2, SHADOW_SPACING, SHADOW_BOUNDS, NPOINTS) for s in (hung, moved)]
    cells = lambda a: a[12:-3].reshape(2, 9, 3)
    assert list(want[0][3:6]) == [2.0, 1.0, 1.0]
    assert _same(cells(want[0])[1], cells(want[1])[1]) and np.abs(cells(want[0])[1]).max() > 0.0
    assert not _same(cells(want[0])[0], cells(want[1])[0])
    # shadowing only takes non-negative terms away: strictly less light under the blocker, and not none (the candidates near x = 0 see past it)
    assert (cells(want[0])[0][0] < cells(want[1])[0][0]).all() and (cells(want[0])[0][0] > 0.0).all()
    got = [s.r.create_probes(s.scene, 2, SHADOW_SPACING, SHADOW_BOUNDS, npoints=NPOINTS).data for s in (hung, moved)]
    print("band 0 of the cell behind the blocker: hung %s, moved %s" % (cells(got[0])[0][0], cells(got[1])[0][0]))
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert _same(cells(got[0])[1], cells(got[1])[1]) and not _same(cells(got[0])[0], cells(got[1])[0])
    assert (cells(got[0])[0][0] < cells(got[1])[0][0]).all()


# ---- 4. films ----
class Film:
    """The film scene: the room with the leaning mesh, an area light and a point light; the grid is baked on the device over the world bound at
    spacing 2.5 (3 x 2 x 3 cells) -- its equality with the restatement is section 3's -- and both sides read the same array."""

    def __init__(self, extra=(), grid=None):
        pt = T.Translate(1.6, 2.5, -1.0)
        self.s = Setup(_prims(emitter=4, leaning=True) + list(extra), None, [core.PointLight(pt.m, (30.0, 26.0, 22.0))])
        self.films = {}
        if grid is not None:   # (a grid baked elsewhere: both sides still read the same array)
            self.grid = grid
            return
        self.grid = self.s.r.create_probes(self.s.scene, 2, 2.5, npoints=NPOINTS)
        # a second grid over the small bounds: most hits lie outside it, where the corner clamp holds the edge cells' values
        self.small = self.s.r.create_probes(self.s.scene, 2, GRID_SPACING, GRID_BOUNDS, npoints=NPOINTS)

    def renderer(self, grid, sampler):
        return core.SamplerRenderer(sampler, self.s.camera, core.UseProbesIntegrator(grid), core.EmissionIntegrator())

    def restated(self, grid, sampler, key):
        if key not in self.films:
            r = self.renderer(grid, sampler)
            pixels = r.pixels()
            vec = r.generate_samples(self.s.scene, pixels)
            integ = pr.UseProbesIntegrator(grid.data)
            film = prt.render(self.s.restated, integ, mrf.restated_camera(self.s.camera), self.s.camera.film, sampler.samplesPerPixel, pixels, vec,
                              prt.keyed_rng(SEED, prt.rr.sample_extent(self.s.camera.film)))
            self.films[key] = (film, pixels, vec, integ)
        return self.films[key]


@pytest.fixture(scope="module")
def film(gpu):
    return Film()


def _ld(f, spp=1):
    return core.LowDiscrepancySampler(f.s.camera, spp, SEED)


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("which", ["grid", "small"])
def test_film_equals_the_restatement(film, which, spp):
    grid = getattr(film, which)
    want, pixels, vec, integ = film.restated(grid, _ld(film, spp), (which, "ld", spp))
    # the sample vectors carry the scene's DirectLighting "all" slots: 5 + (2 + 2 * 2) per light of nsamples 1 + (2 * 4 + 2 * 2 * 4) for the emitter + tau, scatter
    assert vec.shape[1] == _abi.lib().dr_scene_sample_floats(film.s.scene._device().handle, _abi.DR_INTEGRATOR_DIRECT_ALL)
    got = film.renderer(grid, _ld(film, spp)).render(film.s.scene).film
    assert np.isfinite(got).all() and got[..., :3].max() > 0.0
    assert _same(got, want)
    if which == "small":
        assert integ.clamped >= 1   # at least one hit has vx < 0 or vx + 1 >= nProbes[0]


def test_the_film_sees_shading_normals_that_differ_from_the_geometric_ones(film):
    want, pixels, vec, integ = film.restated(film.grid, _ld(film, 4), ("grid", "ld", 4))
    rcam = mrf.restated_camera(film.s.camera)
    hits = [film.s.restated.bvh.intersect(rcam.generateRay(int(px) + float(v[0]), int(py) + float(v[1]), float(v[2]), float(v[3])))
            for (px, py), v in zip(np.repeat(pixels, 4, axis=0), vec)]
    leaning = [h for h in hits if h is not None and isinstance(h.prim.shape, prt.fe.Triangle)]
    assert len(leaning) >= 2
    for h in leaning:
        assert prt.Dot(prt.getBSDF(h).nn, h.dg.nn) < 0.999


def test_stratified_sampler_and_both_state_layouts(film):
    mk = lambda: core.StratifiedSampler(film.s.camera, 2, 2, True, SEED)
    want = film.restated(film.grid, mk(), ("grid", "strat", 4))[0]
    lib = _abi.lib()
    for layout in (64, 4):
        try:
            _abi.check(lib.dr_set_option(b"STATE_LAYOUT", str(layout).encode()))
            r = film.renderer(film.grid, mk())
            got = r.render(film.s.scene).film
            info = film.s.scene._device().last_render_info()
        finally:
            lib.dr_set_option(b"STATE_LAYOUT", None)
        assert info["state_layout"] == layout and _same(got, want)
        assert info["integrator"] == "useprobes" and info["shade_kernels"] == ["k_shade_probes"]
        st = r.last_stats
        assert st["any_launches"] == 0 and st["any_rays"] == 0 and st["closest_launches"] == 1 and 0 < st["shade_vertices"] <= st["camera_samples"]


BALL_C, BALL_R = (-1.1, 0.9, 0.6), 0.9


@pytest.fixture(scope="module")
def ball(film):
    """The film scene and a matte sphere of reversed orientation standing on the floor beside the box: with the room's plain quads and the leaning
    quad's per-vertex N, every branch of the camera hit's geometry (quadric, triangle with DR_SHADING_N, plain triangle).  The grid is
    the film scene's: the integrator only reads it.  (The bake of a scene with a quadric is tests/test_gpu_world_bound.py's.)"""
    at = T.Translate(*BALL_C)
    return Film([core.GeometricPrimitive(core.Sphere(at.m, at.mInv, True, BALL_R), core.MatteMaterial((0.4, 0.5, 0.6)), None)], grid=film.grid)


@pytest.mark.parametrize("layout", [64, 4])
def test_a_quadric_among_the_camera_hits(ball, layout):
    want, pixels, vec, integ = ball.restated(ball.grid, _ld(ball, 1), ("grid", "ld", 1))
    rcam = mrf.restated_camera(ball.s.camera)
    hits = [ball.s.restated.bvh.intersect(rcam.generateRay(int(px) + float(v[0]), int(py) + float(v[1]), float(v[2]), float(v[3]))) for (px, py), v in zip(pixels, vec)]
    on = [sum(h is not None and isinstance(h.prim.shape, cls) for h in hits) for cls in (prt.dr.Sphere, prt.fe.Triangle)]
    on.append(sum(h is not None and type(h.prim.shape) is prt.dr.Triangle for h in hits))
    print("camera hits: %d on the sphere, %d on the mesh with N, %d on plain triangles" % tuple(on))
    assert min(on) >= 2
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(b"STATE_LAYOUT", str(layout).encode()))
        got = ball.renderer(ball.grid, _ld(ball, 1)).render(ball.s.scene).film
        info = ball.s.scene._device().last_render_info()
    finally:
        lib.dr_set_option(b"STATE_LAYOUT", None)
    assert info["state_layout"] == layout and _same(got, want)


def test_halton_sampler_against_the_restatement(film):
    """The Halton sampler's samples belong to the image: one slot per accepted index k and a film that atomics add in no fixed order, so bit
    equality of the film is not defined for this sampler (as for ambient occlusion and PRT, whose tests this follows).  What is: the dumped
    vectors -- with the scene's DirectLighting "all" slots, which this integrator requests -- equal the Halton restatement's bit for bit, the
    weights equal exactly (integer table), and the film lies within tests/film_reference.py's derived bound of the f64 sum of the restated radiances."""
    import film_reference as fr
    import halton_restatement as hr
    s = film.s
    fl = core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5))
    fl.filterTable[:] = fr.INT_TABLE
    cam = core.PerspectiveCamera.lookAt((-1.5, 1.5, -2.5), (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), 70.0, fl)
    r = core.SamplerRenderer(core.HaltonSampler(cam, 2, SEED), cam, core.UseProbesIntegrator(film.grid), core.EmissionIntegrator())
    n1D, n2D = r.requestSamples(r.sampler, s.scene)
    assert n1D == [4, 4, 1, 1, 1, 1] and n2D == [4, 4, 1, 1]   # the emitter (4 samples), the point light, then tau and scatter
    s.scene._device()
    _abi.check(_abi.lib().dr_scene_set_probes(s.scene._device().handle, None, 0))   # (the dump itself must attach the grid)
    k, xy, vec = r.generate_halton_samples(s.scene)
    want = hr.keyed(hr.task_window(fl), 2, SEED, n1D, n2D, 0)
    assert len(k) > 100 and np.array_equal(k, want.k) and np.array_equal(xy, want.pixel_xy)
    assert vec.shape == want.vec.shape == (len(k), 5 + sum(n1D) + 2 * sum(n2D)) and _same(vec, want.vec)
    rcam, integ = mrf.restated_camera(cam), pr.UseProbesIntegrator(film.grid.data)
    Ls = np.array([prt.sample_Li(s.restated, integ, rcam, int(px), int(py), v, prt.dr.RNG(prt.rr.counter_key(SEED, int(kk), 0, prt.rr.LI_KIND)))[0].tuple()
                   for kk, (px, py), v in zip(k, xy, vec)], np.float32)
    ref = fr.reference_from_samples(fl, xy, 1, vec[:, 0], vec[:, 1], Ls, serial=False)
    got = r.render(s.scene).film
    assert np.array_equal(got[..., 3].astype(np.float64), ref.sum[..., 3])
    err, lim = np.abs(got.astype(np.float64) - ref.sum), fr.bound(ref.S, ref.n)
    print("halton: max |device - f64 sum| / bound = %.3g" % float((err[..., :3] / np.maximum(lim[..., :3], 1e-300)).max()))
    assert (err <= lim).all() and np.isfinite(got).all() and got[..., :3].max() > 0


# ---- 5. a known answer that does not come from the restatement ----
def _xyz_of(rgb):
    r, g, b = rgb   # RGBToXYZ (spectrum.dart): the film holds XYZ
    return np.array([0.412453 * r + 0.357580 * g + 0.180423 * b, 0.212671 * r + 0.715160 * g + 0.072169 * b, 0.019334 * r + 0.119193 * g + 0.950227 * b])


def test_an_open_plane_under_a_constant_sky_tends_to_kd_times_l(gpu):
    """An open matte plane (Kd 0.5, 0.25, 0.125) under a map-less infinite light L = 1 with 64 samples, probes baked in a slab above it (lmax 2):
    the irradiance of a unit sky on an upward normal is pi, so Li -> Kd / pi * pi = Kd * L.  The projection is Monte Carlo and the lookup
    interpolates, so the allowed deviation is twice the restatement's own largest relative deviation over the same samples; both are printed and
    DESIGN.md 2.18 records them."""
    kd = (0.5, 0.25, 0.125)
    plane = _quad((-40.0, 0.0, -40.0), (-40.0, 0.0, 40.0), (40.0, 0.0, 40.0), (40.0, 0.0, -40.0), kd=kd)
    s = Setup([plane], core.InfiniteAreaLight(None, (1.0, 1.0, 1.0), 64, None), eye=(0.0, 6.0, 0.5), look=(0.0, 0.0, 0.6))
    bounds = (-4.0, 0.25, -4.0, 4.0, 1.25, 4.0)
    grid = s.r.create_probes(s.scene, 2, 4.0, bounds, npoints=NPOINTS)
    assert grid.nProbes == (2, 1, 2)
    sampler = lambda: core.LowDiscrepancySampler(s.camera, 1, SEED)
    r = core.SamplerRenderer(sampler(), s.camera, core.UseProbesIntegrator(grid), core.EmissionIntegrator())
    pixels = r.pixels()
    vec = r.generate_samples(s.scene, pixels)
    want = prt.render(s.restated, pr.UseProbesIntegrator(grid.data), mrf.restated_camera(s.camera), s.camera.film, 1, pixels, vec,
                      prt.keyed_rng(SEED, prt.rr.sample_extent(s.camera.film)))
    got = r.render(s.scene).film
    rel = lambda f: float(np.abs(f[..., :3] / f[..., 3:4] / _xyz_of(kd) - 1.0).max())
    own = rel(want)
    print("known answer: restatement's largest relative deviation from Kd * L = %.4g, allowed = %.4g, device = %.4g" % (own, 2.0 * own, rel(got)))
    assert (got[..., 3] > 0).all() and own < 0.25 and rel(got) <= 2.0 * own


# ---- 6. refusals ----
def test_refusals_by_name_leave_the_scene_usable(film):
    s, lib = film.s, _abi.lib()
    out = np.zeros((8, 8, 4), np.float32)

    def refused(code, needle, integ, mutate=None):
        r = core.SamplerRenderer(_ld(film), s.camera, integ, core.EmissionIntegrator())
        integ.bind(s.scene)
        d, keep = r.describe()
        if mutate:
            mutate(d)
        rc = lib.dr_render(s.scene._device().handle, C.byref(d), out.ctypes.data, None)
        assert rc == code and needle in lib.dr_last_error().decode(), (rc, lib.dr_last_error())

    refused(-1, "use probes: no probe grid is set on the scene", core.UseProbesIntegrator(None))
    nodirect = film.grid.data.copy()
    nodirect[1] = 0.0
    refused(-4, "use probes: a grid with includeDirect 0 is not supported", core.UseProbesIntegrator(nodirect))

    def adaptive(d):
        d.sampler_mode, d.spp, d.strat_xsamples = _abi.DR_SAMPLER_ADAPTIVE, 8, 2
    refused(-4, "use probes: the adaptive sampler is not supported", core.UseProbesIntegrator(film.grid), adaptive)
    for lmax in (0, 9):
        bad = film.grid.data.copy()
        bad[0] = lmax
        with pytest.raises(_abi.DartRayHipError, match="use probes: lmax of the grid is outside 1 .. 8"):
            core.UseProbesIntegrator(bad).bind(s.scene)
    with pytest.raises(_abi.DartRayHipError, match="create probes: indirectlighting is not supported"):
        s.r.create_probes(s.scene, 2, 2.5, npoints=NPOINTS, indirectlighting=True)
    # the scene is still usable: the film of section 4 again, and another integrator
    want = film.restated(film.grid, _ld(film, 1), ("grid", "ld", 1))[0]
    assert _same(film.renderer(film.grid, _ld(film, 1)).render(s.scene).film, want)
    assert np.isfinite(core.SamplerRenderer(_ld(film), s.camera, core.AmbientOcclusionIntegrator(8), core.EmissionIntegrator()).render(s.scene).film).all()


def test_an_unsupported_material_is_refused_by_name(gpu):
    prims = _prims() + [core.GeometricPrimitive(core.TriangleMesh(np.array([[0, 1, 2]], np.uint32), np.array([(-1, 0.1, -1), (-1, 0.1, -2), (-2, 0.1, -1)], np.float32)),
                                                core.MirrorMaterial((0.9, 0.9, 0.9)), None)]
    accel = core.BVHAccel(prims)
    scene = core.Scene(accel, [core.PointLight(T.Translate(1.6, 2.5, -1.0).m, (30.0, 26.0, 22.0))])
    cam = core.PerspectiveCamera.lookAt((-1.5, 1.5, -2.5), (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), 70.0, core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5)))
    r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 1, SEED), cam, core.UseProbesIntegrator(), core.EmissionIntegrator())
    r.surfaceIntegrator = core.UseProbesIntegrator(r.create_probes(scene, 1, 3.0, npoints=NPOINTS))   # (the bake reads no material)
    with pytest.raises(_abi.DartRayHipError, match="use probes: material mirror .*is not supported"):
        r.render(scene)
