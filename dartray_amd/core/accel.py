"""lib/accelerators/ with core/primitive/, core/ray.dart and core/scene.dart: the aggregate, the scene over it, and their way across the
C ABI -- describe_scene() fills a DrSceneDesc on the host, _DeviceScene hands it to dr_scene_create."""
import ctypes as C
import collections
import math
import time

import numpy as np

from .. import _abi
from .lights import LightContext
from .shapes import _Quadric, _choose_builder


class GeometricPrimitive:
    """core/primitive/geometric_primitive.dart:27-29."""

    def __init__(self, shape, material, areaLight=None):
        self.shape = shape
        self.material = material
        self.areaLight = areaLight
        if areaLight is not None and areaLight.shape is None:
            areaLight.shape = shape

    def getAreaLight(self):
        return self.areaLight


class Ray:
    """Batch of core/ray.dart rays (o, d f32; minDistance/maxDistance f64)."""

    def __init__(self, origin, direction, minDistance=0.0, maxDistance=math.inf):
        self.origin = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1, 3)
        self.direction = np.ascontiguousarray(direction, dtype=np.float32).reshape(-1, 3)
        n = len(self.origin)
        self.minDistance = np.broadcast_to(np.asarray(minDistance, dtype=np.float64), (n,)).copy()
        self.maxDistance = np.broadcast_to(np.asarray(maxDistance, dtype=np.float64), (n,)).copy()

    def __len__(self):
        return len(self.origin)

    def to_abi(self):
        arr = (_abi.DrRay * len(self))()
        buf = np.frombuffer(arr, dtype=np.dtype([("o", "<f4", 3), ("d", "<f4", 3), ("tmin", "<f8"), ("tmax", "<f8")]))
        buf["o"] = self.origin
        buf["d"] = self.direction
        buf["tmin"] = self.minDistance
        buf["tmax"] = self.maxDistance
        return arr


HIT_DTYPE = np.dtype([("prim", "<i4"), ("pad", "<i4"), ("t", "<f8"), ("b1", "<f8"), ("b2", "<f8")])
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("offset", "<u4"), ("nprims", "<u2"),
                       ("axis", "u1"), ("pad", "u1")])


# ---------------------------------------------------------------------------
# BVHAccel (lib/accelerators/bvh_accel.dart) -- the Aggregate of the scene
# ---------------------------------------------------------------------------
def build_bvh_arrays(verts, refined, quadric_bounds, nquadrics, max_prims, builder=None):
    """BVHAccel's constructor (bvh_accel.dart:41-91,228-437) through the C ABI: (nodes, order, nnodes, depth, builder that ran).
    builder: "device" = dr_bvh_build_device (HIP; needs an initialised GPU), "host" = dr_bvh_build_mixed (C++ threads);
    None = the environment's DARTRAY_BVH_BUILDER, else the device builder whenever a GPU has been selected.  Both write
    the same bytes (tests/test_gpu_bvh_device.py)."""
    n = len(refined)
    builder = _choose_builder(builder)
    lib = _abi.lib()
    nodes = np.zeros(max(2 * n - 1, 1), dtype=NODE_DTYPE)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    nn = C.c_uint64(0)
    depth = C.c_uint32(0)
    fn = lib.dr_bvh_build_device if builder == "device" else lib.dr_bvh_build_mixed
    _abi.check(fn(verts.ctypes.data, len(verts), refined.ctypes.data, n, quadric_bounds.ctypes.data, nquadrics, max_prims,
                  nodes.ctypes.data, C.byref(nn), order.ctypes.data, C.byref(depth)))
    return nodes, order, int(nn.value), int(depth.value), builder


class BVHAccel:
    """Aggregate 'bvh' (accelerators/bvh_accel.dart:36-91).

    The constructor refines the primitives, runs the SAH build (host C++ behind
    dr_bvh_build) and keeps the flattened arrays a Dart-side shim would marshal:
    `nodes` (32-byte _LinearBVHNode records) and the per-primitive tables in
    `primitives` order."""

    def __init__(self, p, maxPrims=4, splitMethod="sah", builder=None):
        if splitMethod != "sah":
            raise NotImplementedError("only the default 'sah' split method is on the path")
        self.maxPrimsInNode = min(255, int(maxPrims))
        self.prims_in = list(p)
        self.mesh_xforms = []
        self.materials = []
        self._lights = []  # DiffuseAreaLight objects in first-seen order
        self.quadrics = []  # Sphere / Disk shapes: intersectable, so fullyRefine keeps them whole (primitive.dart:71-84)
        cols = self._gather()
        self.verts = _cat(cols["verts"], (0, 3), np.float32)
        refined = _cat(cols["tri"], (0, 3), np.uint32)
        per_prim = {k: _cat(cols[k], 0, t) for k, t in (("material", np.uint32), ("light", np.int32), ("reverse", np.uint8),
                                                        ("shading", np.uint8), ("xform", np.uint32))}
        self.has_shading = bool(per_prim["shading"].any())
        if self.has_shading:
            self.vert_normals = _cat(cols["n"], (0, 3), np.float32)
            self.vert_tangents = _cat(cols["s"], (0, 3), np.float32)
            self.vert_uvs = _cat(cols["uvs"], (0, 2), np.float32)
        n = len(refined)
        qb = np.zeros((max(len(self.quadrics), 1), 6), dtype=np.float32)
        for i, q in enumerate(self.quadrics):
            lo, hi = q.worldBound()
            qb[i, :3], qb[i, 3:] = lo, hi
        t0 = time.perf_counter()
        nodes, order, nn, depth, self.builder = build_bvh_arrays(self.verts, refined, qb, len(self.quadrics), self.maxPrimsInNode, builder)
        self.build_ms = (time.perf_counter() - t0) * 1e3  # the constructor proper (host pointers in and out)
        order = order[:n]
        self.nodes = nodes[:nn] if n else None  # bvh_accel.dart:50-53
        self.depth = int(depth)
        self.order = order
        # BVHAccel.primitives (orderedPrims, bvh_accel.dart:69-76)
        self.tri_idx = np.ascontiguousarray(refined[order])
        self.tri_material = np.ascontiguousarray(per_prim["material"][order])
        self.tri_light = np.ascontiguousarray(per_prim["light"][order])
        self.tri_reverse = np.ascontiguousarray(per_prim["reverse"][order])
        self.tri_shading = np.ascontiguousarray(per_prim["shading"][order])
        self.tri_xform = np.ascontiguousarray(per_prim["xform"][order])
        self._scene = None
        self._scene_key = None

    def _gather(self):
        """Refines every primitive (primitive.dart:71-84) and returns, per column, the pieces each primitive contributes in input
        order: "verts" / "n" / "s" / "uvs" per vertex (triangle_mesh.dart:195-203; zeros where a mesh has none), "tri" and the
        five per-primitive columns per refined primitive.  Fills materials, _lights, quadrics and mesh_xforms on the way."""
        cols = collections.defaultdict(list)
        base = 0
        for gp in self.prims_in:
            mesh = gp.shape
            mid = len(self.materials)
            self.materials.append(gp.material)
            li = -1
            if gp.areaLight is not None:
                if gp.areaLight not in self._lights:
                    self._lights.append(gp.areaLight)
                li = self._lights.index(gp.areaLight)
            sflags, xf = 0, 0
            if isinstance(mesh, _Quadric):
                cols["tri"].append(np.array([[_abi.DR_PRIM_QUADRIC, len(self.quadrics), 0]], dtype=np.uint32))
                self.quadrics.append(mesh)
                nprim = 1
            else:
                order = mesh.refine()
                cols["verts"].append(mesh.P)
                cols["tri"].append(mesh.vertexIndex[order].astype(np.uint32) + np.uint32(base))
                base += len(mesh.P)
                nprim = len(order)
                for attr, flag, width in (("n", _abi.DR_SHADING_N, 3), ("s", _abi.DR_SHADING_S, 3), ("uvs", _abi.DR_SHADING_UV, 2)):
                    a = getattr(mesh, attr, None)
                    sflags |= flag if a is not None else 0
                    cols[attr].append(a if a is not None else np.zeros((len(mesh.P), width), np.float32))
                if sflags & (_abi.DR_SHADING_N | _abi.DR_SHADING_S):
                    xf = len(self.mesh_xforms)
                    self.mesh_xforms.append((mesh.objectToWorld, mesh.worldToObject))
            for col, value, dtype in (("shading", sflags, np.uint8), ("xform", xf, np.uint32), ("material", mid, np.uint32),
                                      ("light", li, np.int32), ("reverse", 1 if mesh.reverseOrientation else 0, np.uint8)):
                cols[col].append(np.full(nprim, value, dtype=dtype))
        return cols

    @staticmethod
    def Create(prims, ps=None):  # bvh_accel.dart:474-482
        ps = ps or {}
        return BVHAccel(prims, ps.get("maxnodeprims", 4), ps.get("splitmethod", "sah"))

    @property
    def primitives(self):
        return self.tri_idx

    def canIntersect(self):
        return True

    def worldBound(self):  # bvh_accel.dart:93-95
        if self.nodes is None:
            return (np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32))
        return (self.nodes[0]["bmin"].copy(), self.nodes[0]["bmax"].copy())

    def lights(self):
        """One DiffuseAreaLight per emissive shape (dartray.dart:398-401)."""
        return list(self._lights)

    # --- device scene (created lazily, shared with Scene) ---
    def _device_scene(self, lights=None):
        """The uploaded DrScene of this aggregate + light list.  One aggregate can serve several Scenes whose light
        lists differ (e.g. with and without an InfiniteAreaLight): the cache is keyed on the list's identity."""
        want = self._lights if lights is None else lights
        key = tuple(id(l) for l in want)
        cache = self.__dict__.setdefault("_scenes", collections.OrderedDict())
        if key in cache:
            cache.move_to_end(key)
        else:
            # a few light lists keep their own upload (alternating callers do not evict each other), but not without
            # bound: every entry holds the whole geometry in HBM (C4: 1.1 GB), so the least recently used one goes first
            while len(cache) >= self._SCENE_CACHE:
                cache.popitem(last=False)[1].destroy()
            cache[key] = _DeviceScene(self, want)
        self._scene, self._scene_key = cache[key], key
        return cache[key]

    _SCENE_CACHE = 3

    def intersect(self, ray):
        """Aggregate.intersect (bvh_accel.dart:101-165) on a batch: returns a
        structured array (prim, t, b1, b2); prim == -1 is a miss."""
        return self._device_scene().intersect(ray, any_hit=False)

    def intersectP(self, ray):
        """Aggregate.intersectP (bvh_accel.dart:167-226): bool per ray."""
        return self._device_scene().intersect(ray, any_hit=True)["prim"] >= 0

    def stats(self):
        return self._device_scene().stats()


def _cat(pieces, empty_shape, dtype):
    """The pieces of one table end to end, contiguous; no piece at all gives the empty table of that row shape."""
    return np.ascontiguousarray(np.concatenate(pieces) if pieces else np.zeros(empty_shape, dtype), dtype)


def _records(struct, items, fill):
    """A C array of max(len(items), 1) `struct` records, record i filled by fill(items[i], record)."""
    arr = (struct * max(len(items), 1))()
    for i, item in enumerate(items):
        fill(item, arr[i])
    return arr


def _tri_light(accel, lights):
    """Per-primitive area-light index = position of the primitive's DiffuseAreaLight in Scene.lights (-1: not emissive)."""
    pos = np.full(len(accel._lights) + 1, -1, dtype=np.int32)
    for i, al in enumerate(accel._lights):
        if al not in lights:
            raise ValueError("an emissive primitive's area light is missing from Scene.lights")
        pos[i] = lights.index(al)
    return np.ascontiguousarray(np.where(accel.tri_light >= 0, pos[accel.tri_light], -1).astype(np.int32))


def describe_scene(accel, lights):
    """(DrSceneDesc of the aggregate under this light list, the arrays it points into, general) -- host work only: nothing here
    touches the library or a device.  general: the general shading kernels (not the plain-triangle matte ones) run this scene
    (dr_api.hip's `general`).  Every class writes its own record (to_abi); the lists grow in the lights' order."""
    lights = list(lights)
    general = bool(accel.quadrics) or accel.has_shading or any(L.general for L in lights) or any(m.general for m in accel.materials)
    base_of, base = {}, 0
    for gp in accel.prims_in:
        if isinstance(gp.shape, _Quadric):
            continue
        base_of[id(gp.shape)] = base
        base += len(gp.shape.P)
    ctx = LightContext(base_of, {id(q): i for i, q in enumerate(accel.quadrics)})
    mats = _records(_abi.DrMaterial, accel.materials, lambda m, rec: m.to_abi(rec))
    dl = _records(_abi.DrAreaLight, lights, lambda L, rec: L.to_abi(rec, ctx))
    lt = (_abi.DrLightTri * max(len(ctx.light_tris), 1))()
    for i, t in enumerate(ctx.light_tris):
        lt[i].v[:] = t[:3]
        lt[i].reverse_orientation = t[3]
    env_arr = (_abi.DrEnvMap * max(len(ctx.env_maps), 1))(*ctx.env_maps)
    qa = _records(_abi.DrQuadric, accel.quadrics, lambda q, rec: q.to_abi(rec))
    xa = (_abi.DrMeshXform * max(len(accel.mesh_xforms), 1))()
    tri_light = _tri_light(accel, lights)
    d = _abi.DrSceneDesc()
    d.env_maps, d.nenv_maps = C.cast(env_arr, C.c_void_p), len(ctx.env_maps)
    d.quadrics, d.nquadrics = C.cast(qa, C.c_void_p), len(accel.quadrics)
    if accel.has_shading:
        for i, (o2w, w2o) in enumerate(accel.mesh_xforms):
            xa[i].object_to_world[:] = [float(v) for v in np.asarray(o2w, np.float32).reshape(-1)]
            xa[i].world_to_object[:] = [float(v) for v in np.asarray(w2o, np.float32).reshape(-1)]
        d.vert_normals = accel.vert_normals.ctypes.data
        d.vert_tangents = accel.vert_tangents.ctypes.data
        d.vert_uvs = accel.vert_uvs.ctypes.data
        d.tri_shading = accel.tri_shading.ctypes.data
        d.tri_xform = accel.tri_xform.ctypes.data
        d.mesh_xforms, d.nmesh_xforms = C.cast(xa, C.c_void_p), len(accel.mesh_xforms)
    d.nodes = accel.nodes.ctypes.data if accel.nodes is not None else None
    d.nnodes = len(accel.nodes) if accel.nodes is not None else 0
    d.verts, d.nverts = accel.verts.ctypes.data, len(accel.verts)
    d.tri_idx, d.ntris = accel.tri_idx.ctypes.data, len(accel.tri_idx)
    d.tri_material = accel.tri_material.ctypes.data
    d.tri_light = tri_light.ctypes.data
    d.tri_reverse = accel.tri_reverse.ctypes.data
    d.materials, d.nmaterials = C.cast(mats, C.c_void_p), len(accel.materials)
    d.lights, d.nlights = C.cast(dl, C.c_void_p), len(lights)
    d.light_tris, d.nlight_tris = C.cast(lt, C.c_void_p), len(ctx.light_tris)
    d.bvh_depth = accel.depth
    return d, (mats, dl, lt, env_arr, qa, xa, tri_light), general


class _DeviceScene:
    """Owns the DrScene handle (scene arrays resident in HBM)."""

    def __init__(self, accel, lights):
        self.lights = list(lights)  # (no reference back to the aggregate: the cache there would make it a cycle)
        d, self._keep, self.general = describe_scene(accel, self.lights)
        _abi.init(_abi._initialised if _abi._initialised is not None else 0)
        h = C.c_void_p()
        _abi.check(_abi.lib().dr_scene_create(C.byref(d), C.byref(h)))
        self.handle = h

    def destroy(self):
        """dr_scene_destroy now (an evicted cache entry must not wait for a garbage collection)."""
        if getattr(self, "handle", None):
            _abi.lib().dr_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def intersect(self, ray, any_hit):
        n = len(ray)
        out = np.zeros(n, dtype=HIT_DTYPE)
        if n:
            arr = ray.to_abi()
            _abi.check(_abi.lib().dr_intersect(self.handle, C.cast(arr, C.c_void_p), n, out.ctypes.data, 1 if any_hit else 0))
        return out

    def stats(self):
        s = _abi.DrRenderStats()
        _abi.check(_abi.lib().dr_get_stats(self.handle, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _abi.DrRenderStats._fields_}

    def reset_stats(self):
        _abi.check(_abi.lib().dr_reset_stats(self.handle))

    def state_layout(self, layout=None):
        """Get (layout, alive share at the second bounce) of this scene's path renders (0 = not measured yet), or store a
        layout (64 / 4; 0 makes the next big render measure again)."""
        if layout is not None:
            _abi.check(_abi.lib().dr_scene_set_state_layout(self.handle, int(layout)))
        lay, dens = C.c_int32(0), C.c_float(0.0)
        _abi.check(_abi.lib().dr_scene_get_state_layout(self.handle, C.byref(lay), C.byref(dens)))
        return int(lay.value), float(dens.value)

    def trace_kernels(self, kernels=None):
        """Get (closest, any-hit) traversal kernels of this scene (0 = not measured yet), or set them (2 / 3, closest-hit also 5,
        any-hit also 6 / 7 = 2 / 3 with the far child first; (0, 0) makes the next big render measure again)."""
        arr = (C.c_uint32 * 2)(*(kernels or (0, 0)))
        if kernels is not None:
            _abi.check(_abi.lib().dr_scene_set_trace_kernels(self.handle, C.byref(arr)))
        _abi.check(_abi.lib().dr_scene_get_trace_kernels(self.handle, C.byref(arr)))
        return int(arr[0]), int(arr[1])

    def last_render_info(self):
        """What the last render_device call ran with (dr_scene_last_render_info)."""
        arr = (C.c_int32 * 8)()
        _abi.check(_abi.lib().dr_scene_last_render_info(self.handle, C.byref(arr)))
        return {"state_layout": int(arr[0]), "closest_kernel": int(arr[1]), "any_hit_kernel": int(arr[2]),
                "pilot_batches": int(arr[4]), "batches": int(arr[5]), "trace_wg_per_cu": int(arr[6]), "overlap_any": int(arr[7]) & 1,
                "coherent_camera": (int(arr[7]) >> 1) & 1, "lazy_gen": (int(arr[7]) >> 3) & 1,
                # arr[3]: -1, or after a WhittedIntegrator / AmbientOcclusionIntegrator / FeatureIntegrator / DiffusePRTIntegrator / GlossyPRTIntegrator render the integrator and its shading kernels
                "integrator": None if arr[3] < 0 else {_abi.DR_INTEGRATOR_WHITTED: "whitted", _abi.DR_INTEGRATOR_AO: "ambientocclusion",
                                                       _abi.DR_INTEGRATOR_FEATURE: "feature", _abi.DR_INTEGRATOR_DIFFUSE_PRT: "diffuseprt",
                                                       _abi.DR_INTEGRATOR_GLOSSY_PRT: "glossyprt", _abi.DR_INTEGRATOR_USE_PROBES: "useprobes",
                                                       _abi.DR_INTEGRATOR_MATERIAL: "material"}.get(int(arr[3]) & 255),
                "shade_kernels": [] if arr[3] < 0 else [k for bit, k in ((8, "k_shade_whitted"), (9, "k_shade_spec"), (10, "k_shade_ao"),
                                                                         (11, "k_shade_feature"), (15, "k_shade_prt"), (16, "k_shade_gprt"), (16, "k_gprt_finish"), (17, "k_shade_probes"), (18, "k_shade_material")) if (int(arr[3]) >> bit) & 1],
                "feature_channel": (int(arr[3]) >> 12) & 7 if arr[3] >= 0 and (int(arr[3]) >> 11) & 1 else None,
                "material_channel": (int(arr[3]) >> 19) & 1 if arr[3] >= 0 and (int(arr[3]) >> 18) & 1 else None}

    def adaptive_pixels(self):
        """Raster pixels ([n, 2] int32, no particular order) the last render of this scene supersampled (dr_scene_get_adaptive_pixels:
        an AdaptiveSampler's pixels traced at maxSamples; empty after any other sampler's render)."""
        n = C.c_uint64(0)
        _abi.check(_abi.lib().dr_scene_get_adaptive_pixels(self.handle, None, 0, C.byref(n)))
        out = np.zeros((n.value, 2), dtype=np.int32)
        if n.value:
            _abi.check(_abi.lib().dr_scene_get_adaptive_pixels(self.handle, out.ctypes.data, n.value, C.byref(n)))
        return out

    def workspace_bytes(self):
        """Device memory the scene's path-state workspace holds right now (dr_scene_workspace_bytes)."""
        n = C.c_uint64(0)
        _abi.check(_abi.lib().dr_scene_workspace_bytes(self.handle, C.byref(n)))
        return int(n.value)

    def table_counts(self):
        """What the shading kernels' light and material tables hold (dr_scene_get_table_counts): their byte sizes decide whether the
        kernels read them from LDS or from global memory."""
        arr = (C.c_uint32 * 6)()
        _abi.check(_abi.lib().dr_scene_get_table_counts(self.handle, C.byref(arr)))
        return {"nlights": int(arr[0]), "nltris": int(arr[1]), "ncdf": int(arr[2]), "nmats": int(arr[3]),
                "sizeof_DLight": int(arr[4]), "sizeof_DLightTri": int(arr[5])}

    def coherent_stats(self):
        """The part of stats()' closest-hit totals that k_trace_pk (coherent waves: the camera rays) traced."""
        arr = (C.c_double * 5)()
        _abi.check(_abi.lib().dr_scene_get_coherent_stats(self.handle, C.byref(arr)))
        return {"rays": int(arr[0]), "nodes": int(arr[1]), "tris": int(arr[2]), "launches": int(arr[3]), "ms": float(arr[4])}

    def sampler_stats(self):
        """(pixel, LD block) pairs the device sampler generated / that the integrator's reads name (lazy generation: fewer where paths end early)."""
        arr = (C.c_double * 2)()
        _abi.check(_abi.lib().dr_scene_get_sampler_stats(self.handle, C.byref(arr)))
        return {"generated": int(arr[0]), "named": int(arr[1])}

    def pilot(self):
        """What the traversal pilot measured, ms per algorithmic GB: {"closest": {2: .., 3: .., 5: ..}, "any_hit": {2: .., 3: ..}}
        (0.0 = that candidate was not timed)."""
        arr = (C.c_float * 6)()
        _abi.check(_abi.lib().dr_scene_get_pilot(self.handle, C.byref(arr)))
        return {"closest": {2: float(arr[0]), 3: float(arr[1]), 5: float(arr[2])}, "any_hit": {2: float(arr[3]), 3: float(arr[4])},
                "far_first": float(arr[5])}  # any-hit rays: far child first over the reference order, time per ray (0 = not measured)


class Scene:
    """core/scene.dart:26-45."""

    def __init__(self, aggregate, lights, volumeRegion=None):
        if volumeRegion is not None:
            raise NotImplementedError("participating media are not on the path")
        self.aggregate = aggregate
        self.lights = list(lights)
        self.volumeRegion = None
        self.worldBound = aggregate.worldBound()

    def _device(self):
        return self.aggregate._device_scene(self.lights)

    def intersect(self, ray):  # scene.dart:51-56 (through this Scene's own device scene: one upload per Scene)
        return self._device().intersect(ray, any_hit=False)

    def intersectP(self, ray):  # scene.dart:63-68
        return self._device().intersect(ray, any_hit=True)["prim"] >= 0
