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
