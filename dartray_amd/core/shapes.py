"""lib/shapes/.  A quadric's to_abi(rec) fills its DrQuadric; a mesh crosses the C ABI as BVHAccel's flattened tables."""
import ctypes as C
import os

import numpy as np

from .. import _abi
from .transform import _bbox_transform, _inv, transform_points


class TriangleMesh:
    """shapes/triangle_mesh.dart:23-36.  P is already in world space (the
    reference pre-transforms vertices to world space, f32).  Optional per-vertex shading data: `n` (normals)
    and `s` (tangents) stay in OBJECT space and are transformed by objectToWorld at shading time
    (triangle.dart:303-317), so a mesh that has them also carries its transform; `uvs` [nverts,2] replace the
    default (0,0),(1,0),(1,1) parametrisation (triangle.dart:247-263)."""

    def __init__(self, vertexIndex, P, reverseOrientation=False, n=None, s=None, uvs=None, objectToWorld=None,
                 worldToObject=None):
        self.vertexIndex = np.ascontiguousarray(vertexIndex, dtype=np.uint32).reshape(-1, 3)
        self.P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
        self.reverseOrientation = bool(reverseOrientation)
        nv = len(self.P)
        self.n = None if n is None else np.ascontiguousarray(n, dtype=np.float32).reshape(nv, 3)
        self.s = None if s is None else np.ascontiguousarray(s, dtype=np.float32).reshape(nv, 3)
        self.uvs = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1)[:2 * nv].reshape(nv, 2)
        eye = np.eye(4, dtype=np.float32)
        self.objectToWorld = eye if objectToWorld is None else np.ascontiguousarray(np.asarray(objectToWorld, np.float32).reshape(4, 4))
        self.worldToObject = (eye if objectToWorld is None else _inv(self.objectToWorld)) if worldToObject is None else \
            np.ascontiguousarray(np.asarray(worldToObject, np.float32).reshape(4, 4))
        if self.vertexIndex.size and int(self.vertexIndex.max()) >= len(self.P):
            raise ValueError("TriangleMesh has out of-bounds vertex index")  # triangle_mesh.dart:160-166

    @property
    def ntris(self):
        return len(self.vertexIndex)

    def canIntersect(self):
        return False  # triangle_mesh.dart:79-81

    def refine(self):
        """Triangle order after Primitive.fullyRefine / ShapeSet: the todo list
        is a LIFO stack, so triangles come out reversed (primitive.dart:71-84,
        shape_set.dart:25-35)."""
        return np.arange(self.ntris - 1, -1, -1, dtype=np.int64)

    def light_rows(self, ctx):
        """(v0, v1, v2, flags) of every triangle, as an area light's ShapeSet holds them: refine() order, aggregate vertex numbers."""
        flags = (1 if self.reverseOrientation else 0) | (2 if self.uvs is not None else 0)
        rows = []
        for t in self.refine():
            v = self.vertexIndex[t] + ctx.base_of[id(self)]
            rows.append((int(v[0]), int(v[1]), int(v[2]), flags))
        return rows


class _Quadric:
    """Common part of the quadric shapes: they keep objectToWorld and transform the ray per test
    (shape.dart:24-39) instead of pre-transforming geometry, and are intersectable as they are."""

    kind = 0

    def __init__(self, o2w, w2o, reverseOrientation):
        self.objectToWorld = np.ascontiguousarray(np.asarray(o2w, np.float32).reshape(4, 4))
        self.worldToObject = np.ascontiguousarray(np.asarray(w2o, np.float32).reshape(4, 4))
        self.reverseOrientation = bool(reverseOrientation)

    def canIntersect(self):
        return True

    def worldBound(self):  # shape.dart:37-39
        lo, hi = self.objectBound()
        return _bbox_transform(self.objectToWorld, lo, hi)

    def to_abi(self, rec):
        rec.kind = self.kind
        rec.object_to_world[:] = [float(v) for v in self.objectToWorld.reshape(-1)]
        rec.world_to_object[:] = [float(v) for v in self.worldToObject.reshape(-1)]
        rec.params[:] = [float(v) for v in self.params]

    def light_rows(self, ctx):
        """ShapeSet keeps an intersectable shape whole (shape_set.dart:25-35): one row naming the quadric."""
        return [(_abi.DR_PRIM_QUADRIC, ctx.quad_of[id(self)], 0, 1 if self.reverseOrientation else 0)]


class Sphere(_Quadric):
    """shapes/sphere.dart:23-38 (constructor arguments as in Sphere.Create :313-321; phiMax in degrees)."""

    kind = _abi.DR_QUADRIC_SPHERE

    def __init__(self, o2w, w2o, ro, radius=1.0, z0=None, z1=None, phiMax=360.0):
        super().__init__(o2w, w2o, ro)
        self.radius = float(radius)
        z0 = -self.radius if z0 is None else float(z0)
        z1 = self.radius if z1 is None else float(z1)
        self.params = (self.radius, z0, z1, float(phiMax))
        self.zmin = min(max(min(z0, z1), -self.radius), self.radius)
        self.zmax = min(max(max(z0, z1), -self.radius), self.radius)

    def objectBound(self):  # sphere.dart:35-38
        return (-self.radius, -self.radius, self.zmin), (self.radius, self.radius, self.zmax)


class Disk(_Quadric):
    """shapes/disk.dart:23-29 (arguments as in Disk.Create :157-165; phiMax in degrees)."""

    kind = _abi.DR_QUADRIC_DISK

    def __init__(self, o2w, w2o, ro, height=0.0, radius=1.0, innerRadius=0.0, phiMax=360.0):
        super().__init__(o2w, w2o, ro)
        self.height, self.radius, self.innerRadius = float(height), float(radius), float(innerRadius)
        self.params = (self.height, self.radius, self.innerRadius, float(phiMax))

    def objectBound(self):  # disk.dart:31-34
        return (-self.radius, -self.radius, self.height), (self.radius, self.radius, self.height)


def _choose_builder(builder):
    """Which of the two builders of the BVH / of the subdivision runs: the caller's, else the environment's DARTRAY_BVH_BUILDER, else
    the device builder whenever a GPU has been selected."""
    if builder is None:
        builder = os.environ.get("DARTRAY_BVH_BUILDER") or ("device" if _abi._initialised is not None else "host")
    if builder not in ("device", "host"):
        raise ValueError("builder must be 'device' or 'host'")
    return builder


def loop_subdivide(indices, P, nlevels, builder=None):
    """LoopSubdivision's constructor and refine() (loop_subdivision.dart:24-308) through the C ABI: (P, N, indices, builder that ran) of
    the TriangleMesh it creates, object space.  builder: "device" = dr_loop_subdivide_device (HIP; needs an initialised GPU), "host" =
    dr_loop_subdivide (serial C++); None = the environment's DARTRAY_BVH_BUILDER, else the device builder whenever a GPU has been
    selected -- the rule of build_bvh_arrays.  Both write the same bytes (tests/test_gpu_subdiv.py).  A mesh the reference would crash
    or loop on raises DartRayHipError with the refusal's name."""
    builder = _choose_builder(builder)
    lib = _abi.lib()
    fn = lib.dr_loop_subdivide_device if builder == "device" else lib.dr_loop_subdivide
    idx = np.ascontiguousarray(np.asarray(indices).astype(np.uint32, copy=False).reshape(-1))
    idx = idx[:3 * (len(idx) // 3)]  # vi.length ~/ 3 faces (:370)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    nv, nf = C.c_uint64(0), C.c_uint64(0)
    args = (idx.ctypes.data, len(idx) // 3, P.ctypes.data, len(P), int(nlevels))
    _abi.check(fn(*args, None, None, None, 0, 0, C.byref(nv), C.byref(nf)))  # the size query
    Pout = np.empty((nv.value, 3), np.float32)
    Nout = np.empty((nv.value, 3), np.float32)
    iout = np.empty((nf.value, 3), np.uint32)
    _abi.check(fn(*args, Pout.ctypes.data, Nout.ctypes.data, iout.ctypes.data, nv.value, nf.value, C.byref(nv), C.byref(nf)))
    return Pout, Nout, iout, builder


class LoopSubdivision:
    """shapes/loop_subdivision.dart:23-93: Shape 'loopsubdiv'.  Not intersectable; refine() gives ONE TriangleMesh with per-vertex normals
    (:285-307).  indices / P are the control mesh in object space; the constructor's topology (and the refusal of every mesh it cannot
    handle) happens in refine(), inside the library."""

    def __init__(self, o2w, w2o, reverseOrientation, indices, P, nlevels=1):
        self.objectToWorld = np.ascontiguousarray(np.asarray(o2w, np.float32).reshape(4, 4))
        self.worldToObject = np.ascontiguousarray(np.asarray(w2o, np.float32).reshape(4, 4))
        self.reverseOrientation = bool(reverseOrientation)
        self.indices = np.asarray(indices).reshape(-1)
        self.P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
        self.nLevels = int(nlevels)
        self.builder = None  # the builder the last refine() ran

    def canIntersect(self):
        return False  # :95-97

    def objectBound(self):  # :310-316
        return self.P.min(0), self.P.max(0)

    def worldBound(self):  # :318-324
        pts = transform_points(self.objectToWorld, self.P)
        return pts.min(0), pts.max(0)

    def refine(self, builder=None):
        """TriangleMesh.Create(objectToWorld, worldToObject, reverseOrientation, {indices, P: Plimit, N}) (:301-307): the positions
        go to world space like any mesh's (triangle_mesh.dart:29-36), the normals stay in object space with the transform."""
        P, N, idx, self.builder = loop_subdivide(self.indices, self.P, self.nLevels, builder)
        return TriangleMesh(idx, transform_points(self.objectToWorld, P), self.reverseOrientation, n=N,
                            objectToWorld=self.objectToWorld, worldToObject=self.worldToObject)


def nurbs_dice(nu, uorder, uknots, u0, u1, nv, vorder, vknots, v0, v1, P=None, Pw=None, diceu=30, dicev=30, builder=None):
    """Nurbs.refine (nurbs.dart:76-154) through the C ABI: (P, N, uv, indices, builder that ran) of the TriangleMesh it creates, object
    space.  P: nu * nv points [., 3], or else Pw: homogeneous points [., 4]; both u fastest.  Everything crosses as f32.  builder as for
    loop_subdivide: "device" = dr_nurbs_dice_device (HIP; needs an initialised GPU), "host" = dr_nurbs_dice, None = _choose_builder's
    rule.  Both write the same bytes, a NaN's sign and payload aside (tests/test_gpu_nurbs.py).  An input on which the evaluation
    would index outside a list raises DartRayHipError with the refusal's name; two index expressions of the reference's text are repaired
    (DESIGN.md 2.21)."""
    builder = _choose_builder(builder)
    lib = _abi.lib()
    fn = lib.dr_nurbs_dice_device if builder == "device" else lib.dr_nurbs_dice
    if (P is None) == (Pw is None):
        raise ValueError("nurbs_dice needs exactly one of P and Pw")
    uk = np.ascontiguousarray(uknots, dtype=np.float32).reshape(-1)
    vk = np.ascontiguousarray(vknots, dtype=np.float32).reshape(-1)
    cp = np.ascontiguousarray(P if Pw is None else Pw, dtype=np.float32).reshape(-1)
    nu, uorder, nv, vorder = int(nu), int(uorder), int(nv), int(vorder)
    if len(uk) != nu + uorder or len(vk) != nv + vorder:
        raise ValueError("nurbs_dice needs nu + uorder uknots and nv + vorder vknots")
    if len(cp) != nu * nv * (3 if Pw is None else 4):
        raise ValueError("nurbs_dice needs nu * nv control points")
    patch = _abi.DrNurbsPatch(nu, uorder, uk.ctypes.data, float(u0), float(u1), nv, vorder, vk.ctypes.data, float(v0), float(v1),
                              cp.ctypes.data, 0 if Pw is None else 1, int(diceu), int(dicev), 0)
    nverts, ntris = C.c_uint64(0), C.c_uint64(0)
    _abi.check(fn(C.byref(patch), None, None, None, None, 0, 0, C.byref(nverts), C.byref(ntris)))  # the size query
    Pout = np.empty((nverts.value, 3), np.float32)
    Nout = np.empty((nverts.value, 3), np.float32)
    uv = np.empty((nverts.value, 2), np.float32)
    idx = np.empty((ntris.value, 3), np.uint32)
    _abi.check(fn(C.byref(patch), Pout.ctypes.data, Nout.ctypes.data, uv.ctypes.data, idx.ctypes.data, nverts.value, ntris.value,
                  C.byref(nverts), C.byref(ntris)))
    return Pout, Nout, uv, idx, builder


class Nurbs:
    """shapes/nurbs.dart:23-74: Shape 'nurbs'.  Not intersectable; refine() gives ONE TriangleMesh with per-vertex normals and uvs
    (:144-153).  P: nu * nv control points, u fastest, [., 3] or -- isHomogeneous -- [., 4].  The refusals happen in refine(), inside the
    library."""

    def __init__(self, o2w, w2o, reverseOrientation, nu, uorder, uknot, umin, umax, nv, vorder, vknot, vmin, vmax, P, isHomogeneous,
                 diceu=30, dicev=30):
        self.objectToWorld = np.ascontiguousarray(np.asarray(o2w, np.float32).reshape(4, 4))
        self.worldToObject = np.ascontiguousarray(np.asarray(w2o, np.float32).reshape(4, 4))
        self.reverseOrientation = bool(reverseOrientation)
        self.nu, self.uorder, self.nv, self.vorder = int(nu), int(uorder), int(nv), int(vorder)
        self.uknot = np.ascontiguousarray(uknot, dtype=np.float32).reshape(-1)
        self.vknot = np.ascontiguousarray(vknot, dtype=np.float32).reshape(-1)
        self.umin, self.umax, self.vmin, self.vmax = float(umin), float(umax), float(vmin), float(vmax)
        self.isHomogeneous = bool(isHomogeneous)
        self.P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 4 if self.isHomogeneous else 3)
        self.diceu, self.dicev = int(diceu), int(dicev)
        self.builder = None  # the builder the last refine() ran

    def canIntersect(self):
        return False  # :72-74

    def _points(self):
        """The Points both bounds walk: P as it stands, or x / w, y / w, z / w in f64 stored f32 (:42-44, :63-65)."""
        P = self.P[:self.nu * self.nv]
        if not self.isHomogeneous:
            return P
        P64 = P.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (P64[:, :3] / P64[:, 3:4]).astype(np.float32)

    def objectBound(self):  # :30-48
        pts = self._points()
        return pts.min(0), pts.max(0)

    def worldBound(self):  # :50-70
        pts = transform_points(self.objectToWorld, self._points())
        return pts.min(0), pts.max(0)

    def refine(self, builder=None):
        """TriangleMesh.Create(objectToWorld, worldToObject, reverseOrientation, {indices, P, uv, N}) (:146-153): the positions go to
        world space like any mesh's, the normals stay in object space with the transform."""
        kw = {"Pw" if self.isHomogeneous else "P": self.P}
        P, N, uv, idx, self.builder = nurbs_dice(self.nu, self.uorder, self.uknot, self.umin, self.umax, self.nv, self.vorder, self.vknot,
                                                 self.vmin, self.vmax, diceu=self.diceu, dicev=self.dicev, builder=builder, **kw)
        return TriangleMesh(idx, transform_points(self.objectToWorld, P), self.reverseOrientation, n=N, uvs=uv,
                            objectToWorld=self.objectToWorld, worldToObject=self.worldToObject)
