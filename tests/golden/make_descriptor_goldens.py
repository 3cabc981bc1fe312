"""Records what the host classes write into the C ABI's descriptors: tests/golden/descriptors.json.

    python tests/golden/make_descriptor_goldens.py

Every case below is built on the host alone.  _abi.init becomes a no-op and the object _abi.lib() returns is wrapped so
that dr_scene_create and dr_render keep the descriptor they are handed and report success without calling the library;
every other symbol (the host BVH and subdivision builders) is the library's own.  A descriptor's canonical form takes
each _fields_ entry in turn: a value field is its bytes, a pointer field the bytes of the array it addresses (POINTERS
below says how long that is), an embedded struct its fields under dotted names, an array of records the records'
canonical forms one after the other.  The file keeps one sha256 per (case, field), the `general` flag of every scene
case, and the names dartray_amd.core and dartray_amd expose.  tests/test_descriptors.py recomputes all of it through
describe_scene / SamplerRenderer.describe.
"""
import ctypes as C
import glob
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

import dartray_amd
from dartray_amd import _abi, core


def public_names():
    """What `from dartray_amd import *` binds, less the package's own submodules (which of those are loaded depends on
    what else the process imported)."""
    own = {m.split(".")[1] for m in sys.modules if m.startswith("dartray_amd.") and m.count(".") == 1}
    return sorted(n for n in dir(dartray_amd) if not n.startswith("_") and n not in own)


NAMES = {"core": sorted(dir(core)), "dartray_amd": public_names()}  # before anything below imports more of the package

from dartray_amd import pbrt, scenes

OUT = os.path.join(HERE, "descriptors.json")

# (struct, pointer field) -> (record: a struct or a size in bytes, count: a field's name or a function of the struct)
_S, _R, _E = _abi.DrSceneDesc, _abi.DrRenderDesc, _abi.DrEnvMap
POINTERS = {
    (_S, "nodes"): (_abi.DrBvhNode, "nnodes"), (_S, "verts"): (12, "nverts"), (_S, "tri_idx"): (12, "ntris"),
    (_S, "tri_material"): (4, "ntris"), (_S, "tri_light"): (4, "ntris"), (_S, "tri_reverse"): (1, "ntris"),
    (_S, "materials"): (_abi.DrMaterial, "nmaterials"), (_S, "lights"): (_abi.DrAreaLight, "nlights"),
    (_S, "light_tris"): (_abi.DrLightTri, "nlight_tris"), (_S, "env_maps"): (_E, "nenv_maps"),
    (_S, "quadrics"): (_abi.DrQuadric, "nquadrics"), (_S, "vert_normals"): (12, "nverts"), (_S, "vert_tangents"): (12, "nverts"),
    (_S, "vert_uvs"): (8, "nverts"), (_S, "tri_shading"): (1, "ntris"), (_S, "tri_xform"): (4, "ntris"),
    (_S, "mesh_xforms"): (_abi.DrMeshXform, "nmesh_xforms"),
    (_E, "texels"): (12, lambda e: e.width * e.height),
    (_R, "pixel_xy"): (8, lambda d: d.nsamples // d.spp), (_R, "sample_vec"): (4, lambda d: d.nsamples * d.sample_stride),
    (_R, "tail_offsets"): (8, lambda d: d.nsamples + 1),
    # packed: as many values as the last offset says; otherwise max_tail per sample
    (_R, "tail"): (8, lambda d: int(C.cast(d.tail_offsets, C.POINTER(C.c_uint64))[d.nsamples]) if d.tail_offsets else d.nsamples * d.max_tail),
}


def _fields(s, prefix=""):
    """[(dotted field name, canonical bytes)] of the ctypes struct s."""
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if issubclass(typ, C.Structure):
            out += _fields(v, prefix + name + ".")
        elif typ is C.c_void_p:
            record, count = POINTERS[(type(s), name)]
            n = 0 if not v else (getattr(s, count) if isinstance(count, str) else count(s))
            if isinstance(record, int):
                data = C.string_at(v, n * record) if n else b""
            else:
                arr = C.cast(v, C.POINTER(record))
                data = b"".join(b for i in range(n) for _, b in _fields(arr[i]))
            out.append((prefix + name, (b"set:" if v else b"null:") + data))
        else:
            out.append((prefix + name, bytes(v if isinstance(v, C.Array) else typ(v))))
    return out


def canonical(desc):
    """{field: sha256 of its canonical bytes, the first 64 bits in hex (the file stays small; a change still shows)} of a
    DrSceneDesc / DrRenderDesc."""
    return {k: hashlib.sha256(b).hexdigest()[:16] for k, b in _fields(desc)}


# ---------------------------------------------------------------------------------------------------------------------
# scene cases: name -> function returning [Scene, ...] (several Scenes of one case share the aggregate)
# ---------------------------------------------------------------------------------------------------------------------
def _translate(x, y, z):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = (x, y, z)
    return m


def _scenes_config(name, **kw):
    def make():
        prims, mk = scenes.config(name, xres=8, yres=8, spp=2, **kw)
        r = mk()
        accel = core.BVHAccel(prims, builder="host")
        return [core.Scene(accel, accel.lights() + ([r.env] if r.env is not None else []))]
    return make


def _mixed():
    """What scenes.py lacks: every material, both quadrics, per-vertex n / s / uvs, a loopsubdiv mesh, every light kind, and a
    second light list over the same aggregate."""
    tri = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1))
    tan = np.tile(np.array([[1, 0, 0]], np.float32), (4, 1))
    uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    o2w = _translate(0.5, -1.0, 2.0)
    tet_idx, tet_P = [0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2], [[1, 1, 1], [-1, -1, 1], [-1, 1, -1], [1, -1, -1]]
    sub = core.LoopSubdivision(_translate(3, 0, 0), _translate(-3, 0, 0), False, tet_idx, tet_P, 1).refine("host")
    ball_light, glass_light = core.DiffuseAreaLight((5, 4, 3), 2), core.DiffuseAreaLight((1, 2, 3), 1)
    prims = [
        core.GeometricPrimitive(core.TriangleMesh(tri, quad + 2, n=nrm, s=tan, uvs=uvs, objectToWorld=o2w), core.MatteMaterial((0.2, 0.3, 0.4), 20.0)),
        core.GeometricPrimitive(core.TriangleMesh(tri[:1], quad - 2, True), core.MirrorMaterial((0.8, 0.7, 0.6))),
        core.GeometricPrimitive(core.TriangleMesh(tri, quad * 2, uvs=uvs), core.GlassMaterial((0.9, 1, 1), (1, 0.9, 1), 1.33), glass_light),
        core.GeometricPrimitive(core.TriangleMesh(tri, quad - 5, n=nrm, objectToWorld=o2w), core.PlasticMaterial((0.1, 0.2, 0.3), (0.4, 0.5, 0.6), 0.07)),
        core.GeometricPrimitive(core.Sphere(_translate(0, 4, 0), _translate(0, -4, 0), True, 1.5, -1.0, 1.2, 270.0), core.MatteMaterial(), ball_light),
        core.GeometricPrimitive(core.Disk(_translate(0, -4, 0), _translate(0, 4, 0), False, 0.5, 2.0, 0.25, 180.0), core.MirrorMaterial()),
        core.GeometricPrimitive(sub, core.MatteMaterial((0.5, 0.5, 0.5))),
    ]
    accel = core.BVHAccel(prims, maxPrims=2, builder="host")
    spot_cos = core.SpotLight(_translate(0, 8, 0), (3, 3, 3), 40.0, 35.0)
    spot_cos.marshal_cosines = True
    texels = np.arange(3 * 2 * 3, dtype=np.float32).reshape(2, 3, 3) / 7.0
    lights = [core.PointLight(_translate(1, 2, 3), (9, 8, 7)), core.SpotLight(_translate(0, 8, 0), (3, 2, 1), 30.0, 25.0), spot_cos,
              core.InfiniteAreaLight(scenes.SKY_TO_WORLD, (0.5, 0.6, 0.7), 3, texels), core.DistantLight(None, (2, 2, 2), (0.0, -1.0, 0.5))]
    area = accel.lights()
    return [core.Scene(accel, lights[:3] + area + lights[3:]), core.Scene(accel, area[::-1])]


def _empty():
    return [core.Scene(core.BVHAccel([], builder="host"), []),
            core.Scene(core.BVHAccel([], builder="host"), [core.PointLight(None, (1, 1, 1))])]


def _pbrt(path):
    return lambda: [pbrt.load(path, render=False).scene]


def scene_cases():
    cases = {"C1": _scenes_config("C1"), "C2": _scenes_config("C2", blob=(3, 2)), "C4": _scenes_config("C4", hair=(2, 2)),
             "C5": _scenes_config("C5", yard=(1, 1), env_res=(4, 2)), "mixed": _mixed, "empty": _empty}
    for path in sorted(glob.glob(os.path.join(ROOT, "examples", "*.pbrt"))):
        cases["pbrt:" + os.path.basename(path)] = _pbrt(path)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# render cases: name -> function returning a SamplerRenderer
# ---------------------------------------------------------------------------------------------------------------------
def render_cases():
    eye, look, up = (0.0, 1.0, -9.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0)
    film = lambda flt=None, crop=(0.0, 1.0, 0.0, 1.0): core.ImageFilm(12, 8, flt, crop)
    persp = lambda f=None: core.PerspectiveCamera.lookAt(eye, look, up, 40.0, f or film(), lensradius=0.25, focaldistance=7.0)
    path, emission = core.PathIntegrator(5), core.EmissionIntegrator()
    cases = {}

    def add(name, sampler_of, cam=None, integ=path, **kw):
        def make():
            c = cam() if cam else persp()
            return core.SamplerRenderer(sampler_of(c), c, integ, emission, **kw)
        cases[name] = make

    ld = lambda c: core.LowDiscrepancySampler(c, 3, 77)
    add("sampler:lowdiscrepancy", ld)
    add("sampler:stratified", lambda c: core.StratifiedSampler(c, 4, 2, True, 11))
    add("sampler:stratified-nojitter", lambda c: core.StratifiedSampler(c, 2, 2, False, 12))
    add("sampler:adaptive", lambda c: core.AdaptiveSampler(c, 3, 20, "contrast", 13))
    add("sampler:halton", lambda c: core.HaltonSampler(c, 3, 14))
    xy = np.array([[1, 2], [3, 4]], np.int32)
    vec = (np.arange(4 * 7, dtype=np.float32).reshape(4, 7) + 0.5) / 32.0
    tail = (np.arange(4 * 3, dtype=np.float64).reshape(4, 3) + 0.25) / 16.0
    add("sampler:hostbuffer", lambda c: core.HostBufferSampler(c, 2, xy, vec))
    add("sampler:hostbuffer-tail", lambda c: core.HostBufferSampler(c, 2, xy, vec, tail))
    add("sampler:hostbuffer-packed", lambda c: core.HostBufferSampler(c, 2, xy, vec, tail, [0, 3, 1, 2]))
    add("sampler:hostbuffer-packed-empty", lambda c: core.HostBufferSampler(c, 2, xy, vec, tail, [0, 0, 0, 0]))
    add("camera:orthographic", ld, lambda: core.OrthographicCamera.lookAt(eye, look, up, film(), lensradius=0.1, focaldistance=5.0))
    add("camera:environment", ld, lambda: core.EnvironmentCamera.lookAt(eye, look, up, film(), 0.25, 0.75))
    for name, flt in (("box", core.BoxFilter(0.5, 0.75)), ("gaussian", core.GaussianFilter(2.0, 1.5, 1.0)), ("mitchell", core.MitchellFilter(0.25, 0.5, 2.0, 2.5)),
                      ("triangle", core.TriangleFilter(1.5, 2.0)), ("sinc", core.LanczosSincFilter(4.0, 3.0, 2.0))):
        add("filter:" + name, ld, lambda flt=flt: persp(film(flt, (0.25, 0.75, 0.1, 0.9))))
    add("integrator:direct-all", ld, integ=core.DirectLightingIntegrator(core.DirectLightingIntegrator.SAMPLE_ALL_UNIFORM, 3))
    add("integrator:direct-one", ld, integ=core.DirectLightingIntegrator(core.DirectLightingIntegrator.SAMPLE_ONE_UNIFORM, 4))
    add("tasks", ld, taskNum=1, taskCount=3)
    add("tiles", ld, tileRank=2, tileCount=4, tileSize=16)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
class _Capture:
    """The library with dr_scene_create / dr_render (and what a host-only render calls around them) replaced."""

    def __init__(self, lib):
        self._lib, self.scene_descs, self.render_descs = lib, [], []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def dr_scene_create(self, desc, handle):
        self.scene_descs.append(desc._obj)
        return _abi.DR_OK

    def dr_render(self, handle, desc, film, rgb):
        self.render_descs.append(desc._obj)
        return _abi.DR_OK

    def dr_scene_destroy(self, handle):
        pass

    def dr_reset_stats(self, handle):
        return _abi.DR_OK

    def dr_get_stats(self, handle, stats):
        return _abi.DR_OK


def main():
    os.environ.pop("DARTRAY_BVH_BUILDER", None)
    cap = _Capture(_abi.lib())
    _abi.init = lambda device=0: None
    _abi.lib = lambda: cap
    out = {"names": NAMES, "scenes": {}, "general": {}, "renders": {}}
    for name, make in scene_cases().items():
        for i, scene in enumerate(make()):
            dev = scene._device()
            out["scenes"]["%s/%d" % (name, i)] = canonical(cap.scene_descs[-1])
            out["general"]["%s/%d" % (name, i)] = bool(dev.general)
    target = scene_cases()["C1"]()[0]
    for name, make in render_cases().items():
        r = make()  # (alive until its descriptor is read: the sampler owns the arrays)
        r.render(target)
        out["renders"][name] = canonical(cap.render_descs[-1])
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d scene descriptors, %d render descriptors" % (OUT, len(out["scenes"]), len(out["renders"])))


if __name__ == "__main__":
    main()
