"""The first-hit feature integrator on the host (no GPU): the slot table through the real library, the class, the plugin, what
it marshals and where, its refusals by name, and the Python restatement (tests/feature_restatement.py) against answers derived by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dartray_amd import _abi, core, pbrt, scenes

import feature_restatement as fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = {
    "lowdiscrepancy": lambda cam: core.LowDiscrepancySampler(cam, 2, 5489),
    "stratified": lambda cam: core.StratifiedSampler(cam, 2, 1, True, 5489),
    "halton": lambda cam: core.HaltonSampler(cam, 2, 5489),
    "random": lambda cam: core.RandomSampler(cam, 2, 5489),
}


@pytest.fixture(autouse=True)
def host_builder(monkeypatch):
    monkeypatch.setenv("DARTRAY_BVH_BUILDER", "host")


def _renderer(sampler, cam, channel="depth"):
    return core.SamplerRenderer(sampler, cam, core.FeatureIntegrator(channel), core.EmissionIntegrator())


# ---- the slot table ----
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
def test_the_c_table_and_the_python_class_count_the_same_slots(sampler):
    """kIntegratorTraits' row through dr_sample_floats against requestSamples through sampler.slot_counts, as tests/test_integrator_slots.py
    does for the other kinds: 5 camera floats and the volume integrator's two 1-D slots, whatever the lights."""
    cam = scenes.cornell_camera(2, 2)
    r = _renderer(SAMPLERS[sampler](cam), cam)
    assert core.FeatureIntegrator.kind == _abi.DR_INTEGRATOR_FEATURE == 5
    for nlights in (0, 1, 3):
        accel = core.BVHAccel([scenes.floor_quad()])
        scene = core.Scene(accel, [core.PointLight(None, (1.0 + i, 1.0, 1.0)) for i in range(nlights)])
        n1D, n2D = r.sampler.slot_counts(r, scene)
        got = _abi.lib().dr_sample_floats(r.surfaceIntegrator.kind, nlights)
        assert got == 5 + sum(n1D) + 2 * sum(n2D) == 7, (sampler, nlights, n1D, n2D)
        assert (n1D, n2D) == ([1, 1], [])
    # an integrator the table does not know counts as DirectLighting "all": 5 + (2n + 2) + 2 * 2n
    assert _abi.lib().dr_sample_floats(6, 3) == 25


# ---- the class and the plugin ----
def test_plugin_creates_it_and_the_channels_map_to_the_constants():
    make = core.Plugin.get("surfaceIntegrator", "feature")
    assert make is not None
    assert isinstance(make(), core.FeatureIntegrator) and make().channel == "ng"
    want = {"ng": _abi.DR_FEATURE_NG, "ns": _abi.DR_FEATURE_NS, "depth": _abi.DR_FEATURE_DEPTH, "uv": _abi.DR_FEATURE_UV, "id": _abi.DR_FEATURE_ID}
    assert want == {"ng": 0, "ns": 1, "depth": 2, "uv": 3, "id": 4} == fe.CHANNELS
    cam = scenes.cornell_camera(4, 4)
    for name, const in want.items():
        integ = make({"channel": name})
        assert integ.channel == name and integ.li_draws_recorded is False and integ.requestSamples(None, None) == ([], [])
        d, keep = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, integ, core.EmissionIntegrator()).describe()
        assert (d.integrator, d.feature_channel, d.max_depth) == (5, const, 0)
    for bad in ("position", "albedo", "NG", ""):
        with pytest.raises(ValueError) as e:
            make({"channel": bad})
        assert all(n in str(e.value) for n in ("ng", "ns", "depth", "uv", "id")) and str(e.value).startswith("feature integrator: channel")


def test_the_adaptive_sampler_is_refused_and_a_replay_needs_no_seed():
    cam = scenes.cornell_camera(8, 8)
    with pytest.raises(ValueError) as e:
        _renderer(core.AdaptiveSampler(cam, 2, 8, "contrast", 5489), cam).describe()
    assert str(e.value) == "feature integrator: the adaptive sampler is not supported"
    d, keep = _renderer(core.HostBufferSampler(cam, 2, [(0, 0)], np.zeros((2, 7), np.float32)), cam, "uv").describe()
    assert (d.integrator, d.feature_channel, d.sampler_mode, d.tail) == (5, _abi.DR_FEATURE_UV, _abi.DR_SAMPLER_HOST_BUFFER, None)


def test_dr_feature_check_names_its_refusals():
    """The rule dr_render* apply to their scene, asked without one: an index + 1 is exact in f32 below 2^24 primitives."""
    lib = _abi.lib()
    for ch in range(5):
        assert lib.dr_feature_check(ch, 20) == 0 and lib.dr_feature_check(ch, (1 << 24) - 1) == 0
    for ch in (-1, 5, 99):
        assert lib.dr_feature_check(ch, 20) == -1
        assert "feature integrator: unknown channel" in lib.dr_last_error().decode()
    for n in (1 << 24, (1 << 24) + 1, 1 << 40):
        assert lib.dr_feature_check(_abi.DR_FEATURE_ID, n) == -4
        assert "feature integrator: the id channel needs a scene of fewer than 2^24 primitives" in lib.dr_last_error().decode()
        for ch in (_abi.DR_FEATURE_NG, _abi.DR_FEATURE_NS, _abi.DR_FEATURE_DEPTH, _abi.DR_FEATURE_UV):
            assert lib.dr_feature_check(ch, n) == 0                # this channel only
    assert int(np.float32((1 << 24) - 1)) == (1 << 24) - 1 and int(np.float32((1 << 24) + 1)) != (1 << 24) + 1


# ---- the ABI ----
def test_the_channel_sits_in_the_former_padding_and_nothing_moved():
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    off = int(re.search(r"^DR_ABI_OFFSET\(DrRenderDesc, feature_channel, (\d+)\);", header, flags=re.M).group(1))
    D = _abi.DrRenderDesc
    assert off == D.feature_channel.offset == 1340 == D.max_tail.offset + 4 and D.tail_offsets.offset == 1344
    assert C.sizeof(D) == 1352 and "DR_ABI_SIZE(DrRenderDesc, 1352);" in header
    assert "#define DR_INTEGRATOR_FEATURE 5" in header and "#define DR_ABI_VERSION 9" in header and _abi.DR_ABI_VERSION == 9
    for name, v in (("NG", 0), ("NS", 1), ("DEPTH", 2), ("UV", 3), ("ID", 4)):
        assert re.search(r"^#define DR_FEATURE_%s %d\b" % (name, v), header, flags=re.M)
    # the overlay writes those four bytes and no others
    d = D()
    d.max_tail, d.feature_channel = 0x11111111, 3
    assert bytes(d)[1336:1344] == bytes([0x11] * 4 + [3, 0, 0, 0]) and not any(bytes(d)[:1336]) and not any(bytes(d)[1344:])
    # every other integrator's descriptor leaves the word zero
    cam = scenes.cornell_camera(4, 4)
    d, keep = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 2, 5489), cam, core.PathIntegrator(5), core.EmissionIntegrator()).describe()
    assert d.feature_channel == 0
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    assert "const int OFF_DrRenderDesc_feature_channel = 1340;" in dart and "const int DR_INTEGRATOR_FEATURE = 5;" in dart
    assert "DR_FEATURE_NG = 0, DR_FEATURE_NS = 1, DR_FEATURE_DEPTH = 2, DR_FEATURE_UV = 3, DR_FEATURE_ID = 4" in dart
    assert "class FeatureIntegrator extends SurfaceIntegrator" in dart and "rd.i32(OFF_DrRenderDesc_feature_channel, feat.channel);" in dart


def test_the_loader_still_refuses_it():
    with pytest.raises(pbrt.UnsupportedFeature) as e:
        pbrt.loads('SurfaceIntegrator "feature"\nWorldBegin\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                   '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nWorldEnd\n')
    assert "SurfaceIntegrator" in str(e.value) and "feature" in str(e.value)


# ---- the restatement's known answers ----
def _flat(prims):
    """core.BVHAccel's arrays -- what dr_scene_create receives -- handed to the restatement."""
    acc = core.BVHAccel(prims)
    quads = [("sphere" if isinstance(q, core.Sphere) else "disk", q.objectToWorld.reshape(-1), q.worldToObject.reshape(-1), q.reverseOrientation) + tuple(q.params)
             for q in acc.quadrics]
    nodes = [(tuple(float(v) for v in n["bmin"]), tuple(float(v) for v in n["bmax"]), int(n["offset"]), int(n["nprims"]), int(n["axis"])) for n in acc.nodes]
    sh = acc.has_shading
    return fe.build_scene(acc.tri_idx, acc.verts, acc.tri_reverse, acc.tri_material, nodes, quads, acc.tri_shading, acc.tri_xform,
                          acc.vert_normals if sh else None, acc.vert_tangents if sh else None, acc.vert_uvs if sh else None,
                          [(a.reshape(-1), b.reshape(-1)) for a, b in acc.mesh_xforms])


def _ortho(res=4):
    """An orthographic camera at the origin looking down -z over the window [-1, 1]^2: raster (X, Y) -> camera (2 X / res - 1, 1 - 2 Y / res, 0),
    camera -> world a half turn about y.  Every entry is a dyadic rational, so the rays are exact."""
    s = 2.0 / res
    r2c = [s, 0.0, 0.0, -1.0, 0.0, -s, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    c2w = [-1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    return fe.OrthographicCamera(r2c, c2w)


def _unit_quad(ccw_from_camera):
    """The unit quad [-1/2, 1/2]^2 in the plane z = -2, listed counter-clockwise as the camera (looking down -z from the origin) sees it, or
    clockwise."""
    P = [(-0.5, -0.5, -2.0), (0.5, -0.5, -2.0), (0.5, 0.5, -2.0), (-0.5, 0.5, -2.0)]
    if not ccw_from_camera:
        P = P[::-1]
    return core.GeometricPrimitive(core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array(P, np.float32)), core.MatteMaterial((0.5, 0.5, 0.5)), None)


@pytest.mark.parametrize("ccw,blue", [(True, 1.0), (False, 0.0)])
def test_a_unit_quad_before_an_orthographic_camera(ccw, blue):
    """Depth: every ray starts in the plane z = 0 and runs along (0, 0, -1), so t = 2 exactly (the hit test's products are dyadic).
    Normal: with the default uvs (0,0) (1,0) (1,1), du1 = -1, du2 = 0, dv1 = dv2 = -1 (triangle.dart:107-110), the determinant is 1 and
    dpdu = p2 - p1, dpdv = p3 - p2 (:129-131), so nn = normalize((p2 - p1) x (p3 - p2)).  Listed counter-clockwise for a viewer on +z -- where
    the camera is -- that is (1,0,0) x (0,1,0) = (0,0,1) for the triangle (0, 1, 2) and (1,1,0) x (-1,0,0) = (0,0,1) for (0, 2, 3): towards the
    camera, 0.5 * (n + 1) = (0.5, 0.5, 1.0).  The reversed list gives (0,0,-1): (0.5, 0.5, 0.0)."""
    scene, cam = _flat([_unit_quad(ccw)]), _ortho(4)
    pixels = [(1, 1), (2, 1), (1, 2), (2, 2)]                       # the four centre pixels: |x|, |y| < 1/2
    vec = np.array([[0.25, 0.25, 0, 0, 0, 0, 0], [0.75, 0.5, 0, 0, 0, 0, 0]] * 4, np.float32)
    box = [1.0] * 256
    for ch, want in ((fe.DEPTH, (2.0, 2.0, 2.0)), (fe.NG, (0.5, 0.5, blue)), (fe.NS, (0.5, 0.5, blue))):
        Ls, hit, film, rgb = fe.render(scene, ch, cam, 4, 4, 0.5, 0.5, box, 2, pixels, vec)
        assert hit.all() and (Ls == np.array(want, np.float32)).all(), (ch, Ls)
        assert (film[1:3, 1:3, 3] == 2.0).all() and film[0, 0, 3] == 0.0
    # outside the quad: a miss, black, and still a sample of the film
    Ls, hit, film, rgb = fe.render(scene, fe.DEPTH, cam, 4, 4, 0.5, 0.5, box, 2, [(0, 0)], vec[:2])
    assert not hit.any() and (Ls == 0.0).all() and film[0, 0, 3] == 2.0 and (film[0, 0, :3] == 0.0).all()
    # ids: one mesh, material 0, primitives 0 and 1 -> (1 or 2, 1, 1); uv of the default parameterisation stays in the unit square
    Ls, hit, film, rgb = fe.render(scene, fe.ID, cam, 4, 4, 0.5, 0.5, box, 2, pixels, vec)
    assert set(Ls[:, 0]) <= {1.0, 2.0} and len(set(Ls[:, 0])) == 2 and (Ls[:, 1:] == 1.0).all()
    Ls, hit, film, rgb = fe.render(scene, fe.UV, cam, 4, 4, 0.5, 0.5, box, 2, pixels, vec)
    assert (Ls[:, :2] >= 0.0).all() and (Ls[:, :2] <= 1.0).all() and (Ls[:, 2] == 0.0).all() and len(set(Ls[:, 0])) > 1


def test_a_unit_sphere_seen_head_on():
    """A sphere of radius 1 centred d = 5 in front of a perspective camera: the centre ray meets it at d - 1 = 4, where the outward normal
    points back at the camera."""
    at = pbrt.Transform.Translate(0.0, 0.0, 5.0)
    ball = core.GeometricPrimitive(core.Sphere(at.m, at.mInv, False, 1.0), core.MatteMaterial((0.5, 0.5, 0.5)), None)
    scene = _flat([ball])
    ray = lambda: fe.Ray(fe.Vec(0.0, 0.0, 0.0), fe.Vec(0.0, 0.0, 1.0))
    r = ray()
    isect = scene.bvh.intersect(r)
    assert fe.Li(fe.DEPTH, r, isect).tuple() == (4.0, 4.0, 4.0)
    n = fe.Li(fe.NG, r, isect).tuple()
    assert abs(n[0] - 0.5) < 1e-5 and abs(n[1] - 0.5) < 1e-5 and n[2] == 0.0   # (the pole fix-up moves x by 1e-5)
    assert fe.Li(fe.NS, r, isect).tuple() == n                      # a quadric's shading geometry is a copy
    u, v, z = fe.Li(fe.UV, r, isect).tuple()
    assert u == 0.0 and v == 0.0 and z == 0.0                       # phi = atan2(0, 1e-5) = 0; theta = acos(-1) = thetaMin = pi
    assert fe.Li(fe.ID, r, isect).tuple() == (1.0, 1.0, 1.0)
    # reverseOrientation turns the geometric normal and nothing else
    ball2 = core.GeometricPrimitive(core.Sphere(at.m, at.mInv, True, 1.0), core.MatteMaterial((0.5, 0.5, 0.5)), None)
    r = ray()
    isect = _flat([ball2]).bvh.intersect(r)
    assert fe.Li(fe.NG, r, isect).tuple()[2] == 1.0 and fe.Li(fe.DEPTH, r, isect).tuple() == (4.0, 4.0, 4.0)


def test_per_vertex_normals_and_uvs_reach_the_shading_normal_and_uv():
    """A quad in the plane z = 0 whose four vertex normals all lean the same way: the shading normal is that direction, normalised, wherever the
    ray lands; the geometric one stays (0, 0, +-1); and uv is the mesh's own bilinear map."""
    P = np.array([(0, 0, 0), (2, 0, 0), (2, 2, 0), (0, 2, 0)], np.float32)
    N = np.array([(0.0, 0.6, 0.8)] * 4, np.float32)
    uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), P, n=N, uvs=uv)
    scene = _flat([core.GeometricPrimitive(mesh, core.MatteMaterial((0.5, 0.5, 0.5)), None)])
    for x, y in ((0.5, 0.25), (1.5, 1.75), (0.25, 1.0)):
        r = fe.Ray(fe.Vec(x, y, 3.0), fe.Vec(0.0, 0.0, -1.0))
        isect = scene.bvh.intersect(r)
        assert fe.Li(fe.UV, r, isect).tuple() == (fe.f32(x / 2), fe.f32(y / 2), 0.0)
        assert fe.Li(fe.NG, r, isect).tuple() == (0.5, 0.5, 1.0)
        ns = fe.Li(fe.NS, r, isect).tuple()
        assert np.allclose(ns, (0.5, 0.8, 0.9), atol=1e-6) and ns != (0.5, 0.5, 1.0)
        assert fe.Li(fe.DEPTH, r, isect).tuple() == (3.0, 3.0, 3.0)
