"""The first-hit feature integrator restated in plain Python -- the test side's own reading of the reference text the section
cites, on top of the vector, transform, BVH, triangle / sphere / disk hit tests, camera and film of tests/golden/dart_restatement.py (imported,
not copied).  What that file leaves out because no integrator before this one read it is restated here line by line: (u, v) of every shape,
Triangle.getUVs with a mesh's own uvs, and Triangle.getShadingGeometry for meshes with per-vertex N / S.  Cited by file.dart:line of the
reference.  Shares no code with the library: the scene arrives as the flat arrays dr_scene_create receives (`build_scene`)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import dart_restatement as dr  # noqa: E402
from dart_restatement import INFINITY, RGB, Cross, CoordinateSystem, Normalize, Ray, Vec, clamp, f32, transformNormal, transformVector  # noqa: E402,F401

NG, NS, DEPTH, UV, ID = range(5)                                   # DR_FEATURE_* (include/dartray_hip.h)
CHANNELS = {"ng": NG, "ns": NS, "depth": DEPTH, "uv": UV, "id": ID}
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]


class DG(dr.DG):                                                   # differential_geometry.dart:77-102 with the u, v it also stores
    __slots__ = ("u", "v")


def SolveLinearSystem2x2(A, B):                                    # common.dart:170-185 -> (x0, x1) or None
    det = A[0] * A[3] - A[1] * A[2]
    if abs(det) < 1.0e-10:
        return None
    x0 = (A[3] * B[0] - A[1] * B[1]) / det
    x1 = (A[0] * B[1] - A[2] * B[0]) / det
    if math.isnan(x0) or math.isnan(x1):
        return None
    return x0, x1


class Triangle(dr.Triangle):
    """shapes/triangle.dart with the mesh data the golden restatement's Triangle does without: uvs (three (u, v) pairs or None), n and s
    (three object-space Vec each or None) and the mesh's objectToWorld / worldToObject (sixteen f32 values each)."""

    def __init__(self, p1, p2, p3, reverse=False, uvs=None, n=None, s=None, o2w=IDENTITY, w2o=IDENTITY):
        super().__init__(p1, p2, p3, reverse)
        self.uvs, self.n, self.s, self.o2w, self.w2o = uvs, n, s, o2w, w2o

    def getUVs(self):                                              # triangle.dart:247-263
        if self.uvs is not None:
            return [self.uvs[0][0], self.uvs[0][1], self.uvs[1][0], self.uvs[1][1], self.uvs[2][0], self.uvs[2][1]]
        return [0.0, 0.0, 1.0, 0.0, 1.0, 1.0]

    def intersect(self, ray):
        """triangle.dart:44-160 -> (t, rayEpsilon, dg) or None, dg with u and v."""
        p1, p2, p3 = self.p1, self.p2, self.p3
        e1x = p2.x - p1.x; e1y = p2.y - p1.y; e1z = p2.z - p1.z       # :52-57
        e2x = p3.x - p1.x; e2y = p3.y - p1.y; e2z = p3.z - p1.z
        d = ray.d
        s1x = (d.y * e2z) - (d.z * e2y)
        s1y = (d.z * e2x) - (d.x * e2z)
        s1z = (d.x * e2y) - (d.y * e2x)
        divisor = (s1x * e1x) + (s1y * e1y) + (s1z * e1z)
        if divisor == 0.0:
            return None
        invDivisor = 1.0 / divisor
        sx = ray.o.x - p1.x; sy = ray.o.y - p1.y; sz = ray.o.z - p1.z
        b1 = (sx * s1x + sy * s1y + sz * s1z) * invDivisor
        if b1 < 0.0 or b1 > 1.0:
            return None
        s2x = (sy * e1z) - (sz * e1y)
        s2y = (sz * e1x) - (sx * e1z)
        s2z = (sx * e1y) - (sy * e1x)
        b2 = ((d.x * s2x) + (d.y * s2y) + (d.z * s2z)) * invDivisor
        if b2 < 0.0 or b1 + b2 > 1.0:
            return None
        t = (e2x * s2x + e2y * s2y + e2z * s2z) * invDivisor
        if t < ray.mint or t > ray.maxt:
            return None
        uvs = self.getUVs()                                        # :104
        du1 = uvs[0] - uvs[4]; du2 = uvs[2] - uvs[4]; dv1 = uvs[1] - uvs[5]; dv2 = uvs[3] - uvs[5]   # :107-110
        dp1 = p1 - p3
        dp2 = p2 - p3
        determinant = du1 * dv2 - dv1 * du2
        if determinant == 0.0:                                     # :115-127
            e3x = (e2y * e1z) - (e2z * e1y)
            e3y = (e2z * e1x) - (e2x * e1z)
            e3z = (e2x * e1y) - (e2y * e1x)
            ln = math.sqrt(e3x * e3x + e3y * e3y + e3z * e3z)
            dpdu, dpdv = CoordinateSystem(Vec(e3x / ln, e3y / ln, e3z / ln))
        else:
            invdet = 1.0 / determinant
            dpdu = (dp1 * dv2 - dp2 * dv1) * invdet
            dpdv = (dp1 * -du2 + dp2 * du1) * invdet
        b0 = 1.0 - b1 - b2                                         # :135-137
        tu = b0 * uvs[0] + b1 * uvs[2] + b2 * uvs[4]
        tv = b0 * uvs[1] + b1 * uvs[3] + b2 * uvs[5]
        dg = DG().set(ray.pointAt(t), dpdu, dpdv, self.reverse)    # :154
        dg.u, dg.v = tu, tv
        return t, 1.0e-3 * t, dg

    def getShadingGeometry(self, dg):
        """triangle.dart:271-364 (dndu / dndv left out: nothing here reads them) -> dgShading."""
        if self.n is None and self.s is None:                      # :273-276
            return dg
        uv = self.getUVs()
        A = [uv[2] - uv[0], uv[4] - uv[0], uv[3] - uv[1], uv[5] - uv[1]]
        C = [dg.u - uv[0], dg.v - uv[1]]
        sol = SolveLinearSystem2x2(A, C)
        if sol is None:
            bx = by = bz = 1.0 / 3.0
        else:
            by, bz = sol
            bx = 1.0 - by - bz
        if self.n is not None:                                     # :303-309 (obj2world.transformNormal: the transpose of its inverse)
            ns = Normalize(transformNormal(self.w2o, self.n[0] * bx + self.n[1] * by + self.n[2] * bz))
        else:
            ns = dg.nn
        if self.s is not None:                                     # :311-317
            ss = Normalize(transformVector(self.o2w, self.s[0] * bx + self.s[1] * by + self.s[2] * bz))
        else:
            ss = Normalize(dg.dpdu)
        ts = Cross(ss, ns)                                         # :319-325
        if ts.lengthSquared() > 0.0:
            ts = Normalize(ts)
            ss = Cross(ts, ns)
        else:
            ss, ts = CoordinateSystem(ns)
        out = DG().set(dg.p, ss, ts, self.reverse)                 # :353-356
        out.u, out.v = dg.u, dg.v
        return out


class Sphere(dr.Sphere):
    def intersect(self, r):                                        # sphere.dart:117-120 beside the golden restatement's dpdu / dpdv
        h = self._hit(r)
        if h is None:
            return None
        thit, eps, dg0 = dr.Sphere.intersect(self, r)
        _, phit, phi = h
        dg = DG().set(dg0.p, dg0.dpdu, dg0.dpdv, self.reverse)
        dg.u = phi / self.phiMax
        theta = math.acos(clamp(phit.z / self.radius, -1.0, 1.0))
        dg.v = (theta - self.thetaMin) / (self.thetaMax - self.thetaMin)
        return thit, eps, dg

    def getShadingGeometry(self, dg):                              # shape.dart: dgShading.copy(dg)
        return dg


class Disk(dr.Disk):
    def intersect(self, r):                                        # disk.dart:69-75
        h = self._hit(r)
        if h is None:
            return None
        thit, eps, dg0 = dr.Disk.intersect(self, r)
        _, phit, dist2, phi = h
        dg = DG().set(dg0.p, dg0.dpdu, dg0.dpdv, self.reverse)
        dg.u = phi / self.phiMax
        oneMinusV = (math.sqrt(dist2) - self.innerRadius) / (self.radius - self.innerRadius)
        dg.v = 1.0 - oneMinusV
        return thit, eps, dg

    def getShadingGeometry(self, dg):
        return dg


class OrthographicCamera(dr.PerspectiveCamera):
    """cameras/orthographic_camera.dart:53-82 without a lens: the origin is the raster point in camera space, the direction (0, 0, 1)."""

    def generateRay(self, imageX, imageY, lensU=0.0, lensV=0.0):
        assert self.lensRadius == 0.0
        Pcamera = self._point(self.r2c, Vec(imageX, imageY, 0.0))
        return Ray(self._point(self.c2w, Pcamera), self._vector(self.c2w, Vec(0.0, 0.0, 1.0)), 0.0, INFINITY, 0)


class FlatScene:
    """bvh: a dr.BVH over dr.Prim whose .ids = (index in the primitive array, index in the material array)."""

    def __init__(self, bvh):
        self.bvh = bvh


def build_scene(tri_idx, verts, tri_reverse, tri_material, nodes, quadrics=(), tri_shading=None, tri_xform=None, vert_n=None, vert_s=None,
                vert_uv=None, xforms=()):
    """The arrays of a scene description in BVHAccel.primitives order.  tri_idx[i] = (a, b, c), or (0xFFFFFFFF, q, 0): quadric q of
    `quadrics`, each ("sphere" | "disk", objectToWorld, worldToObject, reverseOrientation, constructor arguments...).  tri_shading[i]: bit 0 N,
    bit 1 S, bit 2 uv; xforms[tri_xform[i]] = (objectToWorld, worldToObject).  nodes: (bmin, bmax, offset, nprims, axis)."""
    pt = lambda a, i: Vec(float(a[i][0]), float(a[i][1]), float(a[i][2]))
    prims = []
    for i in range(len(tri_idx)):
        a, b, c = (int(v) for v in tri_idx[i])
        if a == 0xFFFFFFFF:
            kind, o2w, w2o, ro = quadrics[b][:4]
            shape = (Sphere if kind == "sphere" else Disk)([float(v) for v in o2w], [float(v) for v in w2o], bool(ro), *quadrics[b][4:])
        else:
            f = int(tri_shading[i]) if tri_shading is not None else 0
            o2w, w2o = ([float(v) for v in m] for m in xforms[int(tri_xform[i])]) if f & 3 else (IDENTITY, IDENTITY)
            shape = Triangle(pt(verts, a), pt(verts, b), pt(verts, c), bool(tri_reverse[i]),
                             uvs=[(float(vert_uv[k][0]), float(vert_uv[k][1])) for k in (a, b, c)] if f & 4 else None,
                             n=[pt(vert_n, k) for k in (a, b, c)] if f & 1 else None,
                             s=[pt(vert_s, k) for k in (a, b, c)] if f & 2 else None, o2w=o2w, w2o=w2o)
        p = dr.Prim(shape, (0.5, 0.5, 0.5))
        p.ids = (i, int(tri_material[i]))
        prims.append(p)
    return FlatScene(dr.BVH(list(nodes), prims))


def Li(channel, ray, isect):
    """DESIGN.md 2.14, "Arithmetic": f64 from the Intersection, one rounding to the f32 of a Spectrum (RGB stores three f32)."""
    if channel == NG:
        n = isect.dg.nn                                            # intersection.dart: dg as Shape.intersect set it
        return RGB(0.5 * (n.x + 1.0), 0.5 * (n.y + 1.0), 0.5 * (n.z + 1.0))
    if channel == NS:
        n = isect.prim.shape.getShadingGeometry(isect.dg).nn       # Intersection.getBSDF -> GeometricPrimitive.getBSDF (:63-68)
        return RGB(0.5 * (n.x + 1.0), 0.5 * (n.y + 1.0), 0.5 * (n.z + 1.0))
    if channel == DEPTH:
        return RGB(ray.maxt, ray.maxt, ray.maxt)                   # geometric_primitive.dart:47-61 shrank it to the hit
    if channel == UV:
        return RGB(isect.dg.u, isect.dg.v, 0.0)
    assert channel == ID
    return RGB(isect.prim.ids[0] + 1.0, isect.prim.ids[1] + 1.0, 1.0)


def sample_Li(scene, channel, camera, px, py, sv):
    """One camera sample: generateRay, scene.intersect, Li at a hit and 0 at a miss, T * Li + Lv with T = 1 and Lv = 0, * rayWeight, the
    guards (sampler_renderer.dart:67-98,160-193) -> (Ls, imageX, imageY, hit)."""
    imageX = px + float(sv[0])
    imageY = py + float(sv[1])
    ray = camera.generateRay(imageX, imageY, float(sv[2]), float(sv[3]))
    isect = scene.bvh.intersect(ray)
    L = Li(channel, ray, isect) if isect is not None else RGB(0.0)
    Ls = (RGB(1.0) * L + RGB(0.0)) * 1.0
    if Ls.hasNaNs():
        Ls = RGB(0.0)
    elif Ls.luminance() < -1e-5:
        Ls = RGB(0.0)
    elif math.isinf(Ls.luminance()):
        Ls = RGB(0.0)
    return Ls, imageX, imageY, isect is not None


def render(scene, channel, camera, xres, yres, xWidth, yWidth, filterTable, spp, pixels, vectors):
    """The samples `vectors` ([len(pixels) * spp][nFloats], a pixel's samples adjacent) of the raster pixels `pixels`, in that order; a
    pixel's samples reach the film after all of them were traced (sampler_renderer.dart:199-203).
    -> (Ls [n][3] f32, hit [n] bool, film [H][W][4] f32: X, Y, Z, weightSum, rgb [H][W][3] f32: ImageFilm.writeImage)."""
    film = dr.ImageFilm(xres, yres, xWidth, yWidth, filterTable)
    Ls, hits = [], []
    for k, (px, py) in enumerate(np.asarray(pixels).reshape(-1, 2)):
        pending = []
        for i in range(spp):
            L, ix, iy, hit = sample_Li(scene, channel, camera, int(px), int(py), vectors[k * spp + i])
            pending.append((ix, iy, L))
            Ls.append(L.tuple())
            hits.append(hit)
        for a in pending:
            film.addSample(*a)
    lx = np.array(film.Lxyz, np.float32).reshape(yres, xres, 3)
    out = np.concatenate([lx, np.array(film.weightSum, np.float32).reshape(yres, xres, 1)], axis=2)
    return np.array(Ls, np.float32), np.array(hits, bool), out, np.array(film.writeImage(), np.float32).reshape(yres, xres, 3)
