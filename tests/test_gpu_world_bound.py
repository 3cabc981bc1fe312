"""The scene's world bound (DScene::rootBox, dr_scene_create) where no sibling-pair records are built.  Diffuse and glossy PRT project the lights'
direct radiance at its centre (dr_prt_incident), the probe bake walks inside its bounding sphere and lays its default grid over it; the traversal
kernels read it only with the pair records.  A scene that cannot take the pair layout -- one with a quadric, a leaf of more than 31 primitives,
a box that is not the union of its children's -- must have the same world bound as any other: node 0's box.  Everything is compared bit for
bit with the Python restatements (tests/prt_restatement.py, tests/glossy_prt_restatement.py, tests/probes_restatement.py) through the sibling
test modules' own scaffolds, under both scene preparations.  The scenes lie well away from the origin, and every case asserts on the CPU that
the restated result at the origin -- what six zeros give -- is not the restated result at the centre.  Restated results are computed once per
configuration and shared.  Nothing is started after a failed call: every call's return code raises."""
import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt

import probes_restatement as pr
import prt_restatement as prt
import test_gpu_glossy_prt as tg
import test_gpu_probes as tb
import test_gpu_prt as tp
from test_gpu_prt import _cin_array, _quad, _same
from test_gpu_scene_prep import _pairs

pytestmark = pytest.mark.gpu

SEED = 5489
T = pbrt.Transform
PREPS = [None, b"host"]
PAIRLESS, CONTROLS = ["sphere", "disk", "bigleaf", "notunion"], ["plain", "oneleaf"]
LIGHTS = ["point", "spot", "area", "together"]

# the plain quads: x in [1, 7], y in [0.5, 2], z in [2, 9] -- the origin lies outside the bound, below and behind it
FLOOR = ((1.0, 0.5, 2.0), (1.0, 0.5, 9.0), (7.0, 0.5, 9.0), (7.0, 0.5, 2.0))
BLOCKER = ((3.0, 2.0, 4.0), (5.0, 2.0, 4.0), (5.0, 2.0, 6.0), (3.0, 2.0, 6.0))
EMITTER = ((0.0, 5.0, 6.0), (2.0, 5.0, 6.0), (2.0, 5.0, 8.0), (0.0, 5.0, 8.0))     # faces down; beside and above the centre: seen obliquely
STEP = ((5.5, 1.0, 7.0), (6.5, 1.0, 7.0), (6.5, 1.0, 8.0), (5.5, 1.0, 8.0))         # notunion, plain: a third leaf, so one interior node is not the root
SHARD = ((2.0, 1.0, 3.0), (3.0, 1.0, 3.0), (2.0, 1.75, 4.0))                       # bigleaf: forty copies of this triangle
# oneleaf: the bound's centre (2, 2, 3.5) lies off the triangle's plane, on the side its normal faces (the side an emitter lights)
LONE = ((1.0, 1.0, 3.0), (1.0, 3.0, 4.0), (3.0, 1.0, 4.0))
BALL_C, BALL_R = (6.0, 3.0, 8.0), 1.5                                              # raises the bound's pMax to (7.5, 4.5, 9.5)
DISK_C, DISK_R = (2.0, 3.5, 3.0), 1.5                                              # in the plane z = 3: pMin.x 0.5, pMax.y 5


def _tri(p, light=None):
    mesh = core.TriangleMesh(np.array([[0, 1, 2]], np.uint32), np.array(p, np.float32))
    if light is not None:
        light = core.DiffuseAreaLight(light[0], light[1], mesh)
    return core.GeometricPrimitive(mesh, core.MatteMaterial((0.5, 0.5, 0.5)), light)


def _ball():
    at = T.Translate(*BALL_C)
    return core.GeometricPrimitive(core.Sphere(at.m, at.mInv, False, BALL_R), core.MatteMaterial((0.4, 0.5, 0.6)), None)


def _prims(cls, emitter=0):
    """The geometry of one scene class; emitter: the sample count of its area light (0: none).  oneleaf's one triangle is its own emitter."""
    if cls == "oneleaf":
        return [_tri(LONE, light=((6.0, 5.0, 4.0), emitter) if emitter else None)]
    p = [_quad(*FLOOR), _quad(*BLOCKER)]
    if cls == "sphere":
        p.append(_ball())
    elif cls == "disk":
        at = T.Translate(*DISK_C)
        p.append(core.GeometricPrimitive(core.Disk(at.m, at.mInv, False, 0.0, DISK_R), core.MatteMaterial((0.4, 0.5, 0.6)), None))
    elif cls == "bigleaf":
        mesh = core.TriangleMesh(np.arange(120, dtype=np.uint32).reshape(40, 3), np.array(SHARD * 40, np.float32))
        p.append(core.GeometricPrimitive(mesh, core.MatteMaterial((0.5, 0.5, 0.5)), None))
    else:
        assert cls in ("notunion", "plain")
        p.append(_quad(*STEP))
    if emitter:
        p.append(_quad(*EMITTER, light=((6.0, 5.0, 4.0), emitter)))
    return p


def _accel(cls, prims):
    """The aggregate the device gets: bigleaf's with leaves of up to 255 primitives, notunion's with one inner box enlarged (the mutation of
    tests/test_gpu_scene_prep.py); the root box stays what the builder gave, so the restatement's centre is the device's."""
    if cls == "bigleaf":
        acc = core.BVHAccel(prims, 255)
        assert (acc.nodes["nprims"] > 31).any()
    elif cls == "notunion":
        acc = core.BVHAccel(prims)                                   # (a quad's two triangles share their bound's centroid: one leaf per quad)
        inner = np.flatnonzero(acc.nodes["nprims"] == 0)
        assert len(inner) >= 2 and inner[0] == 0
        acc.nodes[int(inner[1])]["bmax"][0] += 1.0
    else:
        acc = core.BVHAccel(prims)
    if cls == "oneleaf":
        assert len(acc.nodes) == 1
    if cls in ("sphere", "disk"):
        assert len(acc.quadrics) == 1
    else:
        assert len(acc.quadrics) == 0
    return acc


def _lights(name):
    """(emitter's sample count, the infinite light or None, the delta lights).  `together`: tests/test_gpu_prt.py's mix -- an area light of four
    samples (three draws of the shared RNG), a map-less infinite light, a point light (no draws) and a spot light (the next three draws)."""
    pt, sp = T.Translate(2.0, 4.0, 3.0), T.Translate(5.0, 6.0, 7.0) * T.Rotate(90.0, 1.0, 0.0, 0.0)   # (the spot light shines down)
    point, spot = lambda: core.PointLight(pt.m, (30.0, 26.0, 22.0)), lambda: core.SpotLight(sp.m, (50.0, 60.0, 70.0), 60.0, 25.0, sp.mInv)
    if name == "point":
        return 0, None, [point()]
    if name == "spot":
        return 0, None, [spot()]
    if name == "area":
        return 4, None, []
    assert name == "together"
    return 4, core.InfiniteAreaLight(None, (0.8, 0.9, 1.0), 1, None), [point(), spot()]


def _created_under(prep, scene):
    """Creates the scene's device scene under one scene preparation (the option is read by dr_scene_create) -> its number of pair records."""
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(b"SCENE_PREP", prep))
        return len(_pairs(scene._device())[0])
    finally:
        lib.dr_set_option(b"SCENE_PREP", None)


_restated = {}


def _restated_case(cls, light):
    """The restated side of one (scene class, light) case, built once: a tests/test_gpu_prt.py Setup (its restated scene and lights; its own
    device scene is never made) with the restated c_in at the centre and at the origin per lmax."""
    if (cls, light) not in _restated:
        emitter, env, delta = _lights(light)
        s = tp.Setup(_prims(cls, emitter), env, delta)
        s.at_origin = {}
        _restated[(cls, light)] = s
    return _restated[(cls, light)]


_env_projection = {}


class _env_projected_once:
    """While active, prt.shProject_infinite answers a repeated question from memory: the restated projection of an infinite light reads neither the
    point nor the scene (infinite_area_light.dart:207-281 without light visibility), only the light -- its radiance, its transform, its map -- and
    lmax, and this module's one map-less light is asked for it at two points of six scenes."""

    def __enter__(self):
        self.inner = inner = prt.shProject_infinite

        def remembered(light, p, lmax):
            mp = light.radianceMap
            key = (light.L.tuple(), tuple(float(v) for v in light.lightToWorld), mp.width, mp.height, tuple(c.tuple() for c in mp.pyramid[0][2]), lmax)
            if key not in _env_projection:
                _env_projection[key] = inner(light, p, lmax)
            return list(_env_projection[key])
        prt.shProject_infinite = remembered

    def __exit__(self, *exc):
        prt.shProject_infinite = self.inner


def _cin_at_centre(s, lmax):
    with _env_projected_once():
        return s.restated_cin(lmax)


def _cin_at_origin(s, lmax):
    if lmax not in s.at_origin:
        with _env_projected_once():
            s.at_origin[lmax] = prt.ProjectIncidentDirectRadiance(prt.Vec(0.0, 0.0, 0.0), 0.0, s.restated.lights, lmax, prt.dr.RNG())
    return s.at_origin[lmax]


def _differs(a, b):
    """Non-vacuity: some coefficient differs by more than 1e-3 of the largest |c_in|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.abs(a - b).max() > 1.0e-3 * np.abs(a).max())


def _device_scene(cls, light, prep):
    """A fresh aggregate and Scene of the case, its device scene created under the given preparation; the class it names is asserted."""
    emitter, env, delta = _lights(light)
    acc = _accel(cls, _prims(cls, emitter))
    scene = core.Scene(acc, acc.lights() + ([env] if env is not None else []) + list(delta))
    records = _created_under(prep, scene)
    if cls in PAIRLESS:
        assert records == 0
    elif cls == "plain":
        assert records > 0
    else:   # one leaf: the pair layout holds (the root reference is the leaf), but a record is an interior node's and there is none
        assert records == 0 and len(acc.nodes) == 1
    return acc, scene


# ---- 1. the incident light ----
@pytest.mark.parametrize("prep", PREPS, ids=["device", "host"])
@pytest.mark.parametrize("light", LIGHTS)
@pytest.mark.parametrize("cls", PAIRLESS + CONTROLS)
def test_incident_light_is_projected_at_the_world_centre(gpu, cls, light, prep):
    """dr_prt_incident through both integrators, lmax 2 and 4, against ProjectIncidentDirectRadiance at world_centre(scene), by bit equality.

    Why the suite missed the unset bound, confirmed on the CPU with prt_restatement alone: the one PRT scene with a quadric, yard_sphere of
    tests/test_gpu_prt.py, has the world centre (0, 1.5, 0.95000005) in the plane y = 1.5 of its only area light, which faces up, and the origin
    below that light's back; its infinite light has no map.  Its restated c_in at Vec(0, 0, 0) equals the one at the centre bit for bit at
    lmax 2 and 4 (largest |c_in| 3.5447514, the infinite light's band 0), so its film could not tell the two points apart."""
    s = _restated_case(cls, light)
    acc, scene = _device_scene(cls, light, prep)
    root = s.restated.bvh.nodes[0]
    assert _same(root[0], acc.nodes[0]["bmin"]) and _same(root[1], acc.nodes[0]["bmax"])   # the restated bound is the device's
    c = prt.world_centre(s.restated)
    assert min(abs(c.x), abs(c.y), abs(c.z)) > 1.0
    for lmax in (2, 4):
        want, origin = _cin_array(_cin_at_centre(s, lmax)), _cin_array(_cin_at_origin(s, lmax))
        assert np.isfinite(want).all() and _differs(want, origin)
        for name, integ in (("diffuse", core.DiffusePRTIntegrator(lmax, 1)), ("glossy", core.GlossyPRTIntegrator(tg.KD, tg.KS, tg.ROUGH, lmax, 1))):
            got = integ.incident(scene)
            print("%s %s lmax %d %s: max |device - restatement| = %.3g, |origin - centre| = %.3g, of %.3g" % (
                cls, light, lmax, name, float(np.abs(got - want).max()), float(np.abs(origin - want).max()), float(np.abs(want).max())))
            assert got.shape == want.shape == ((lmax + 1) ** 2, 3) and _same(got, want)


# ---- 2. the films of the sphere class ----
EYE, LOOK = (2.0, 6.0, 0.0), (5.0, 1.5, 7.0)


def _film_camera():
    return core.PerspectiveCamera.lookAt(EYE, LOOK, (0.0, 1.0, 0.0), 55.0, core.ImageFilm(8, 8, core.BoxFilter(0.5, 0.5)))


def _film_point():
    return core.PointLight(T.Translate(2.0, 4.0, 3.0).m, (30.0, 26.0, 22.0))


@pytest.fixture(scope="module")
def diffuse_film(gpu):
    """The sphere class under a point light, seen from above and in front: the film test tests/test_gpu_prt.py's yard_sphere was meant to be."""
    s = tp.Setup(_prims("sphere"), None, [_film_point()])
    s.camera = _film_camera()
    return s


@pytest.fixture(scope="module")
def glossy_film(gpu):
    """The same under tests/test_gpu_glossy_prt.py's Setup (which adds its map-less infinite light); the point light follows it on both sides."""
    s = tg.Setup(_prims("sphere"))
    point = _film_point()
    s.scene = core.Scene(s.scene.aggregate, s.scene.lights + [point])
    s.restated.lights = list(s.restated.lights) + [tp._restated_delta(point)]
    s.camera = _film_camera()
    return s


def _check_film(s, prep, cin_at_centre):
    want, pixels, vec = s.restated_film((2, 8), tp._ld(s), "ld")
    origin = prt.ProjectIncidentDirectRadiance(prt.Vec(0.0, 0.0, 0.0), 0.0, s.restated.lights, 2, prt.dr.RNG())
    assert _differs(_cin_array(cin_at_centre), _cin_array(origin))
    hits = tp._camera_hits(s, pixels, vec)
    on = [sum(h is not None and isinstance(h.prim.shape, prt.dr.Sphere) for h in hits), sum(h is not None and type(h.prim.shape) is prt.dr.Triangle for h in hits)]
    print("camera hits: %d on the sphere, %d on plain triangles, %d misses" % (on[0], on[1], sum(h is None for h in hits)))
    assert min(on) >= 2
    acc = core.BVHAccel(s.scene.aggregate.prims_in)               # a fresh aggregate: its device scene is created under this preparation
    scene = core.Scene(acc, s.scene.lights)
    assert _created_under(prep, scene) == 0
    got = s.renderer((2, 8), tp._ld(s)).render(scene).film
    print("max |device - restatement| = %.3g of %.3g" % (float(np.abs(got - want).max()), float(np.abs(want).max())))
    assert np.isfinite(got).all() and got[..., :3].max() > 0.0 and _same(got, want)


@pytest.mark.parametrize("prep", PREPS, ids=["device", "host"])
def test_diffuse_prt_film_of_a_scene_with_a_sphere(diffuse_film, prep):
    _check_film(diffuse_film, prep, diffuse_film.restated_cin(2))


@pytest.mark.parametrize("prep", PREPS, ids=["device", "host"])
def test_glossy_prt_film_of_a_scene_with_a_sphere(glossy_film, prep):
    _check_film(glossy_film, prep, glossy_film.preprocess(2)[0])


# ---- 3. the probe bake of the sphere class ----
NPOINTS, SPACING = 128, 4.0
PROBE_EYE, PROBE_LOOK = (6.0, 1.0, 5.5), (6.0, 3.0, 8.0)   # the walks start above the floor beside the blocker, below the sphere


class Bake:
    """tests/test_gpu_probes.py's Setup of the sphere class with one light; the restated walks are made once, with every scene intersection
    they ask for recorded."""

    def __init__(self, light):
        emitter, env, delta = _lights(light)
        self.s = tb.Setup(_prims("sphere", emitter), env, delta, eye=PROBE_EYE, look=PROBE_LOOK)
        bvh, self.asked = self.s.restated.bvh, []
        inner = bvh.intersect

        def recording(ray):
            isect = inner(ray)
            self.asked.append(None if isect is None else isect.prim.shape)
            return isect
        bvh.intersect = recording
        try:
            self.pts, self.walks = pr.surface_points(self.s.restated, self.s.eye, NPOINTS)
        finally:
            del bvh.intersect
        self.grid = pr.make_grid(self.s.restated, SPACING)

    def device_scene(self, prep):
        acc = core.BVHAccel(self.s.scene.aggregate.prims_in)
        scene = core.Scene(acc, self.s.scene.lights)
        assert _created_under(prep, scene) == 0
        return scene


@pytest.fixture(scope="module")
def bake_point(gpu):
    return Bake("point")


@pytest.fixture(scope="module")
def bake_area(gpu):
    return Bake("area")


@pytest.mark.parametrize("prep", PREPS, ids=["device", "host"])
def test_surface_points_of_a_scene_with_a_sphere(bake_point, prep):
    """The walks of k_walk_step on a scene with a quadric: its quadric branch (rec.isQuad, ray_epsilon(true, t)) is taken by every walk step
    that lands on the scene's sphere, the other branch by the steps that leave the scene and land on the bounding sphere of the world bound."""
    b = bake_point
    on_ball = sum(isinstance(shape, prt.dr.Sphere) for shape in b.asked)
    on_scene = sum(shape is not None for shape in b.asked)
    on_bound = sum(b.walks) - on_scene                       # points the walks deposited without a scene hit: on the bounding sphere
    print("%d walks, %d points: %d on the scene's sphere, %d on triangles, %d on the bounding sphere" % (
        len(b.walks), len(b.pts), on_ball, on_scene - on_ball, on_bound))
    assert on_ball >= 2 and on_scene - on_ball >= 2 and on_bound >= 1
    assert len(b.pts) == 1 + sum(b.walks) >= NPOINTS
    got = b.s.r.probes_surface_points(b.device_scene(prep), NPOINTS)
    assert got.shape == (len(b.pts), 3) and _same(got, tb._pts_array(b.pts))


@pytest.mark.parametrize("prep", PREPS, ids=["device", "host"])
def test_default_grid_and_candidates_of_a_scene_with_a_sphere(bake_point, prep):
    b = bake_point
    n, bounds = b.grid
    cells = n[0] * n[1] * n[2]
    root = b.s.restated.bvh.nodes[0]
    assert 2 <= cells <= 12 and _same(bounds, list(root[0]) + list(root[1])) and bounds[3] == BALL_C[0] + BALL_R   # the sphere's own bound
    scene = b.device_scene(prep)
    gn, gb = b.s.r.probes_grid(scene, SPACING)
    assert list(gn) == n and _same(gb, bounds)
    want = [pr.accept(b.s.restated, n, bounds, c, b.pts) for c in range(cells)]
    nfound, acc = b.s.r.probes_candidates(scene, tb._pts_array(b.pts), SPACING)
    for c in range(cells):
        assert nfound[c] == len(want[c][0]) and list(acc[c][:nfound[c]]) == want[c][0] and (acc[c][nfound[c]:] == -1).all()


@pytest.mark.parametrize("prep", PREPS, ids=["device", "host"])
@pytest.mark.parametrize("light", ["point", "area"])
def test_bake_of_a_scene_with_a_sphere_equals_the_restatement(bake_point, bake_area, light, prep):
    """The whole bake over the default grid, as tests/test_gpu_probes.py's _check_bake compares it."""
    b = bake_point if light == "point" else bake_area
    if not hasattr(b, "baked"):
        b.baked = pr.bake(b.s.restated, b.s.eye, 2, SPACING, None, NPOINTS)
    want = b.baked
    n = b.grid[0]
    got = b.s.r.create_probes(b.device_scene(prep), 2, SPACING, npoints=NPOINTS)
    assert got.data.shape == want.shape == (15 + n[0] * n[1] * n[2] * 27,) and np.isfinite(got.data).all()
    print("%s: max |device - restatement| = %.3g of %.3g" % (light, float(np.abs(got.data - want).max()), float(np.abs(want[12:]).max())))
    assert _same(got.data[:12], want[:12]) and (got.data[-3:] == 0).all() and np.abs(want[12:]).max() > 0.0
    assert _same(got.data, want)


# ---- 4. the refusal that remains ----
def test_the_bake_still_refuses_a_scene_without_nodes(gpu):
    scene = core.Scene(core.BVHAccel([]), [_film_point()])
    cam = _film_camera()
    r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 1, SEED), cam, core.UseProbesIntegrator(), core.EmissionIntegrator())
    for prep in PREPS:
        fresh = core.Scene(core.BVHAccel([]), scene.lights)
        assert _created_under(prep, fresh) == 0
        with pytest.raises(_abi.DartRayHipError, match="create probes: the scene's world bound is empty or not finite"):
            r.probes_surface_points(fresh, NPOINTS)
        with pytest.raises(_abi.DartRayHipError, match="create probes: the scene's world bound is empty or not finite"):
            r.create_probes(fresh, 2, SPACING, (1.0, 0.5, 2.0, 7.0, 2.0, 9.0), npoints=NPOINTS)
