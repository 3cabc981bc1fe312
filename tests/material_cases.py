"""What the material integrator's tests share (tests/test_material_integrator.py on the host, tests/test_gpu_material.py on the device): a
core aggregate and light list handed to tests/material_restatement.py as the flat arrays dr_scene_create receives, and the scenes."""
import numpy as np

from dartray_amd import core, pbrt
from dartray_amd.core.accel import _tri_light

import feature_restatement as fe
import material_restatement as me

T = pbrt.Transform
GREY = (0.5, 0.5, 0.5)
KINDS = {"MatteMaterial": "matte", "PlasticMaterial": "plastic", "MirrorMaterial": "mirror", "GlassMaterial": "glass"}


def flat(acc):
    """fe.build_scene of a core.BVHAccel's arrays."""
    quads = [("sphere" if isinstance(q, core.Sphere) else "disk", q.objectToWorld.reshape(-1), q.worldToObject.reshape(-1), q.reverseOrientation) + tuple(q.params)
             for q in acc.quadrics]
    nodes = [(tuple(float(v) for v in n["bmin"]), tuple(float(v) for v in n["bmax"]), int(n["offset"]), int(n["nprims"]), int(n["axis"])) for n in acc.nodes]
    sh = acc.has_shading
    return fe.build_scene(acc.tri_idx, acc.verts, acc.tri_reverse, acc.tri_material, nodes, quads, acc.tri_shading, acc.tri_xform,
                          acc.vert_normals if sh else None, acc.vert_tangents if sh else None, acc.vert_uvs if sh else None,
                          [(a.reshape(-1), b.reshape(-1)) for a, b in acc.mesh_xforms])


def restated(acc, lights):
    """me.build_scene of the aggregate under `lights` (core light objects, Scene.lights' order)."""
    mats = [(KINDS[type(m).__name__], tuple(float(v) for v in getattr(m, "Kd", (0.0, 0.0, 0.0))),
             tuple(float(v) for v in (m.Kr if KINDS[type(m).__name__] in ("mirror", "glass") else (0.0, 0.0, 0.0)))) for m in acc.materials]
    ls = []
    for l in lights:
        if isinstance(l, core.DiffuseAreaLight):
            ls.append(("area", l.Lemit))
        elif isinstance(l, core.InfiniteAreaLight):
            h, w = l.texels.shape[:2]
            ls.append(("infinite", l.lightToWorld.reshape(-1), l.worldToLight.reshape(-1), l.L, l.texels.reshape(-1, 3), w, h))
        else:
            ls.append(("area", (0.0, 0.0, 0.0)))                   # a delta light: Le(ray) is 0 and no primitive carries it
    return me.build_scene(flat(acc), mats, _tri_light(acc, list(lights)), ls)


def mesh(P, material, idx=((0, 1, 2), (0, 2, 3)), light=None, **kw):
    return core.GeometricPrimitive(core.TriangleMesh(np.array(idx, np.uint32), np.array(P, np.float32), **kw), material, light)


def yard_prims():
    """Eleven shapes before the camera of tests/test_gpu_feature.py: a floor quad, a quad with per-vertex N, a reverseOrientation quad, a
    mirror, a plastic and a glass quad, a sphere, a triangle emitter facing the camera, a disk emitter seen from behind and one seen from the
    front, and a reversed emitter quad whose listed normal points away but whose reversed one faces the camera.  The camera also sees past
    the floor's far edge: misses."""
    n = np.array([(0.3, 0.9, -0.1), (-0.2, 0.8, -0.4), (-0.3, 0.7, -0.6), (0.4, 0.9, -0.2)], np.float32)
    prims = [mesh([(-4.0, 0.0, -2.0), (-4.0, 0.0, 5.0), (4.0, 0.0, 5.0), (4.0, 0.0, -2.0)], core.MatteMaterial((0.7, 0.6, 0.5))),
             mesh([(-3.0, 0.5, 2.5), (-0.5, 0.5, 2.5), (-0.5, 2.5, 3.5), (-3.0, 2.5, 3.5)], core.MatteMaterial((0.2, 0.3, 0.4)), n=n),
             mesh([(0.5, 0.2, 1.0), (2.5, 0.2, 1.0), (2.5, 1.8, 2.0), (0.5, 1.8, 2.0)], core.MatteMaterial((0.1, 0.8, 0.1)), reverseOrientation=True),
             mesh([(-3.6, 0.1, 0.4), (-2.4, 0.1, 0.4), (-2.4, 1.2, 0.9), (-3.6, 1.2, 0.9)], core.MirrorMaterial((0.9, 0.85, 0.8))),
             mesh([(-2.2, 0.1, 0.2), (-1.2, 0.1, 0.2), (-1.2, 1.0, 0.6), (-2.2, 1.0, 0.6)], core.PlasticMaterial((0.3, 0.2, 0.6), (0.5, 0.5, 0.5), 0.05)),
             mesh([(2.6, 0.1, 0.2), (3.6, 0.1, 0.2), (3.6, 1.0, 0.6), (2.6, 1.0, 0.6)], core.GlassMaterial((0.95, 0.9, 1.0), (0.4, 0.4, 0.4), 1.5))]
    at = T.Translate(1.6, 2.6, 3.0)
    prims.append(core.GeometricPrimitive(core.Sphere(at.m, at.mInv, False, 0.9), core.MatteMaterial((0.6, 0.1, 0.1)), None))
    # a triangle emitter: listed so that normalize((p2 - p1) x (p3 - p1)) has z < 0, towards a camera that looks along +z
    prims.append(mesh([(-1.0, 0.1, 0.2), (-0.2, 1.2, 0.6), (0.6, 0.1, 0.0)], core.MatteMaterial(GREY), idx=((0, 1, 2),),
                      light=core.DiffuseAreaLight((5.0, 4.0, 3.0), 1)))
    # two disks with the same tilt: the disk's normal is its object-space +z; one turned to face the camera, one away from it
    back = T.Translate(-2.0, 3.2, 3.0) * T.Rotate(60.0, 1.0, 0.0, 0.0)
    front = T.Translate(0.0, 3.4, 3.0) * T.Rotate(-120.0, 1.0, 0.0, 0.0)
    prims.append(core.GeometricPrimitive(core.Disk(back.m, back.mInv, False, 0.0, 0.8, 0.2), core.MatteMaterial(GREY), core.DiffuseAreaLight((2.0, 7.0, 1.0), 1)))
    prims.append(core.GeometricPrimitive(core.Disk(front.m, front.mInv, False, 0.0, 0.6, 0.0), core.MatteMaterial(GREY), core.DiffuseAreaLight((1.0, 2.0, 9.0), 1)))
    prims.append(mesh([(2.8, 2.0, 2.0), (3.8, 2.0, 2.0), (3.8, 3.0, 2.4), (2.8, 3.0, 2.4)], core.MatteMaterial(GREY), reverseOrientation=True,
                      light=core.DiffuseAreaLight((8.0, 8.0, 2.0), 1)))
    return prims


def sky():
    """A 4 x 2 radiance map that differs texel by texel, under a factor that differs per channel, turned about x."""
    tex = np.array([[(0.1, 0.2, 0.3), (0.4, 0.5, 0.6), (0.7, 0.8, 0.9), (1.0, 1.1, 1.2)],
                    [(2.0, 1.5, 1.0), (0.5, 0.25, 0.125), (3.0, 0.0, 1.0), (0.0, 2.0, 0.5)]], np.float32)
    return core.InfiniteAreaLight(T.Rotate(30.0, 1.0, 0.0, 0.0).m, (0.5, 1.0, 2.0), 1, tex)
