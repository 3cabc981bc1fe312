"""Where a scene's light and material tables live while a shading kernel runs ("Where the tables live"), restated
in plain Python, and scene builders whose tables have an exact size.

The launchers of k_shade_path, k_shade_direct (dr_kernels.hip) and k_shade_whitted (dr_shade_whitted.hip) pick one of two compiled forms
per scene from the byte sizes of its tables (light_table_bytes, mat_table_bytes, lightsInLds: dr_shade_common.h).  Nothing on the device
reports the choice, so a test that means to cover one form states it here from the scene's own counts (dr_scene_get_table_counts) and
asserts it: placement().  Every constant is read from the sources, none is retyped; tests/test_table_placement.py holds the restated
formulas against the worked numbers and the parsed text against the launchers' own lines."""
import collections
import os
import re

import numpy as np

from dartray_amd import core, scenes

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dartray_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _define(text, name):
    """The value of `#define name <integer expression>` (the first one: the #ifndef default)."""
    m = re.search(r"^#define %s\s+\(?([0-9 *+]+?)\)?\s*(?://.*)?$" % re.escape(name), text, flags=re.M)
    assert m, name
    return _product(m.group(1))


def _product(expr):
    out = 1
    for f in expr.split("*"):
        out *= int(f)
    return out


# The launch conditions as the three launchers write them (white space apart): what placement() restates.
LAUNCH_CONDITIONS = {
    "k_shade_path": ("dr_kernels.hip", "lightsInLds(sc) && push_stage_bytes(SHADE_BLOCK_OF(gen), envq ? 5 : 4) + x <= 160 * 1024"),
    "k_shade_direct": ("dr_kernels.hip", "lightsInLds(sc) && push_stage_bytes(SHADE_BLOCK_OF(gen)) + light_table_bytes(sc) + mat_table_bytes(sc) <= 160 * 1024"),
    "k_shade_whitted": ("dr_shade_whitted.hip", "lightsInLds(sc) && push_stage_bytes(SHADE_BLOCK_OF(true)) + x <= 160 * 1024"),
}


def parse_constants():
    """Every number the placement depends on, from the text of the headers and the launchers."""
    common, wave = _text("dr_shade_common.h"), _text("dr_wave.h")
    c = {"DR_LDS_LIGHT_BYTES": _define(common, "DR_LDS_LIGHT_BYTES"), "DR_LDS_MAT_BYTES": _define(common, "DR_LDS_MAT_BYTES"),
         "DR_SHADE_BLOCK": _define(common, "DR_SHADE_BLOCK"), "DR_SHADE_BLOCK_GEN": _define(common, "DR_SHADE_BLOCK_GEN"),
         "DR_PUSH_ITERS": _define(wave, "DR_PUSH_ITERS")}
    ltb = re.search(r"light_table_bytes\(const DScene& sc\) \{[^\n]*\n\s*return \(size_t\)sc\.nlights \* sizeof\(DLight\) \+ \(size_t\)sc\.nltris \* "
                    r"\(sizeof\(DLightTri\) \+ (\d+)\) \+ \(size_t\)sc\.ncdf \* (\d+);", common)
    assert ltb, "light_table_bytes no longer reads as restated here"
    c["EDGE_BYTES"], c["CDF_ENTRY_BYTES"] = int(ltb.group(1)), int(ltb.group(2))
    mtb = re.search(r"mat_table_bytes\(const DScene& sc\) \{\s*const size_t b = \(size_t\)sc\.nmats \* (\d+);\s*return b <= DR_LDS_MAT_BYTES \? b : 0;", common)
    assert mtb, "mat_table_bytes no longer reads as restated here"
    c["MAT_BYTES"] = int(mtb.group(1))
    assert re.search(r"lightsInLds\(const DScene& sc\) \{\s*return sc\.nlights > 0 && light_table_bytes\(sc\) <= DR_LDS_LIGHT_BYTES;", common), "lightsInLds"
    assert re.search(r"return sizeof\(PushStage\) \+ \(size_t\)nq \* \(size_t\)blockDimX \* DR_PUSH_ITERS \* sizeof\(uint32_t\);", wave), "push_stage_bytes"
    assert re.search(r"push_stage_bytes\(uint32_t blockDimX, int nq = 4\)", wave), "push_stage_bytes' default list count"
    limits, lists = set(), None
    for kernel, (unit, cond) in LAUNCH_CONDITIONS.items():
        flat = " ".join(_text(unit).split())
        assert "if (" + cond + ")" in flat, "the launch condition of %s no longer reads as restated here" % kernel
        limits.add(_product(re.search(r"<= ([0-9 *]+)$", cond).group(1)))
        m = re.search(r"envq \? (\d+) : (\d+)", cond)
        if m:
            lists = (int(m.group(1)), int(m.group(2)))
    assert len(limits) == 1 and lists
    c["LDS_BYTES"] = limits.pop()
    c["ENV_LISTS"], c["LISTS"] = lists
    c["SIZEOF_PUSHSTAGE"] = push_stage_size_from_text(wave)
    return c


def push_stage_size_from_text(wave=None):
    """sizeof(PushStage) from the struct's text (dr_wave.h) as built: the DR_SHADE_PROF member is not compiled in.  Every member is an
    array of a naturally aligned scalar, in an order that needs no padding (asserted)."""
    wave = wave if wave is not None else _text("dr_wave.h")
    body = re.search(r"struct PushStage \{(.*?)\n\};", wave, flags=re.S).group(1)
    body = re.sub(r"#ifdef DR_SHADE_PROF.*?#endif", "", body, flags=re.S)
    width = {"uint32_t": 4, "unsigned long long": 8}
    size, members = 0, 0
    for line in body.splitlines():
        line = line.split("//")[0].strip()
        if not line:
            continue
        m = re.fullmatch(r"(uint32_t|unsigned long long) \w+((?:\[\d+\])+);", line)
        assert m, "a member of PushStage this reader does not know: %r" % line
        n = _product("*".join(re.findall(r"\[(\d+)\]", m.group(2))))
        assert size % width[m.group(1)] == 0
        size += n * width[m.group(1)]
        members += 1
    assert members == 3 and size % 8 == 0
    return size


K = parse_constants()

# kernel variant -> (the kernel as the launcher names it, general shading kernels, staging lists per wave)
Variant = collections.namedtuple("Variant", "kernel general env lists")
VARIANTS = {
    "path": Variant("k_shade_path<false,false,*>", False, False, K["LISTS"]),
    "path_env": Variant("k_shade_path<true,false,*>", False, True, K["ENV_LISTS"]),
    "path_gen": Variant("k_shade_path<true,true,*>", True, False, K["LISTS"]),
    "direct": Variant("k_shade_direct<false,*>", False, False, K["LISTS"]),
    "direct_gen": Variant("k_shade_direct<true,*>", True, False, K["LISTS"]),
    "whitted": Variant("k_shade_whitted<*>", True, False, K["LISTS"]),
}


def push_stage_bytes(block, lists=None):
    return K["SIZEOF_PUSHSTAGE"] + (K["LISTS"] if lists is None else lists) * block * K["DR_PUSH_ITERS"] * 4


def stage_bytes(variant):
    v = VARIANTS[variant]
    return push_stage_bytes(K["DR_SHADE_BLOCK_GEN"] if v.general else K["DR_SHADE_BLOCK"], v.lists)


def light_table_bytes(c):
    return c["nlights"] * c["sizeof_DLight"] + c["nltris"] * (c["sizeof_DLightTri"] + K["EDGE_BYTES"]) + c["ncdf"] * K["CDF_ENTRY_BYTES"]


def mat_table_bytes(c):
    b = c["nmats"] * K["MAT_BYTES"]
    return b if b <= K["DR_LDS_MAT_BYTES"] else 0


def lights_in_lds(c):
    return c["nlights"] > 0 and light_table_bytes(c) <= K["DR_LDS_LIGHT_BYTES"]


def placement_of_counts(c, variant):
    """"lds": LdsLights with the material table beside the lights; "lds_lights_global_mats": LdsLights whose mat() reads global memory;
    "global": GlobalLights."""
    if lights_in_lds(c) and stage_bytes(variant) + light_table_bytes(c) + mat_table_bytes(c) <= K["LDS_BYTES"]:
        return "lds" if mat_table_bytes(c) else "lds_lights_global_mats"
    return "global"


def table_counts(scene):
    """The counts of a core.Scene's uploaded tables (dr_scene_get_table_counts)."""
    return scene._device().table_counts()


def host_counts(scene, sizeof_DLight, sizeof_DLightTri):
    """What table_counts() will say of a core.Scene, worked out on the host from its descriptor (no device): the upload keeps one light
    record per light, one light-triangle record per marshalled one, one material record per primitive, and a CDF of ntris + 1 entries per
    area light (a single entry where there is none).  The record sizes are the caller's (compiled_sizes)."""
    from dartray_amd import _abi
    d, keep, _ = core.describe_scene(scene.aggregate, scene.lights)
    lights = keep[1]
    ncdf = sum(lights[i].ntris + 1 for i in range(d.nlights) if lights[i].kind == _abi.DR_LIGHT_DIFFUSE_AREA)
    return {"nlights": int(d.nlights), "nltris": int(d.nlight_tris), "ncdf": max(ncdf, 1), "nmats": int(d.nmaterials),
            "sizeof_DLight": sizeof_DLight, "sizeof_DLightTri": sizeof_DLightTri}


def compiled_sizes(workdir):
    """sizeof(PushStage), sizeof(DLight), sizeof(DLightTri) as the host pass of the product's own compiler lays them out: a stand-alone
    program over dr_wave.h (which brings dr_device.h), built with the library's flags for the host only and run.  No device is touched."""
    import subprocess
    src, exe = os.path.join(str(workdir), "table_sizes.hip"), os.path.join(str(workdir), "table_sizes")
    with open(src, "w") as fh:
        fh.write('#include <cstdio>\n#include "dr_kernels.h"\n#include "dr_wave.h"\n'
                 'int main() { std::printf("%zu %zu %zu\\n", sizeof(PushStage), sizeof(DLight), sizeof(DLightTri)); return 0; }\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O0", "-std=c++17", "-Wno-unused-function", "-I", CSRC,
                           "-x", "hip", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    return {"PushStage": int(out[0]), "DLight": int(out[1]), "DLightTri": int(out[2])}


def placement(scene, kernel_variant):
    """Which form of `kernel_variant` (a key of VARIANTS) a render of `scene` launches, from the scene's own counts.  The scene must
    belong to the variant: general or plain shading kernels, with or without an infinite light."""
    v = VARIANTS[kernel_variant]
    dev = scene._device()
    has_env = any(isinstance(L, core.InfiniteAreaLight) for L in scene.lights)
    if kernel_variant != "whitted":   # (k_shade_whitted has one form for every scene)
        assert bool(dev.general) == v.general and has_env == v.env, (kernel_variant, dev.general, has_env)
    return placement_of_counts(dev.table_counts(), kernel_variant)


def with_fan(c, n, have):
    """The counts `c` of a scene that holds a fan of `have` triangles, with a fan of n in its place: a light triangle and a CDF entry
    more per triangle, the same lights and materials."""
    return dict(c, nltris=c["nltris"] + n - have, ncdf=c["ncdf"] + n - have)


def with_tiles(c, k, have):
    """The counts `c` of a scene whose floor is `have` tiles, with k tiles in their place: a material record per tile."""
    return dict(c, nmats=c["nmats"] + k - have)


def fan_sizes(c, variant, have, lo=2, hi=1000):
    """(largest n for which the scene of counts `c`, rebuilt with a fan of n triangles in place of its fan of `have`, is "lds"; smallest
    n for which it is "global"), by the restated formula alone."""
    where = [placement_of_counts(with_fan(c, n, have), variant) for n in range(lo, hi)]
    assert where[0] == "lds" and where[-1] == "global", (where[0], where[-1])
    first_global = where.index("global")
    assert all(w == "global" for w in where[first_global:]) and all(w == "lds" for w in where[:first_global])
    return lo + first_global - 1, lo + first_global


# ---- scene builders with exact table sizes ----
def fan_emitter(n, L=(36.0, 36.0, 36.0), nSamples=1, centre=(0.0, 0.0), half=3.0, y=9.9):
    """A flat emitter under the Cornell ceiling at the place and winding of scenes.emitter_quad (normal (0, -1, 0)), cut into exactly n
    triangles: a fan from the quad's first corner over its two far edges, ceil(n / 2) pieces on the first and the rest on the second.
    One TriangleMesh under one DiffuseAreaLight."""
    assert n >= 2
    cx, cz = centre
    p0, p1, p2, p3 = ((cx - half, y, cz - half), (cx + half, y, cz - half), (cx + half, y, cz + half), (cx - half, y, cz + half))
    n1 = (n + 1) // 2
    n2 = n - n1
    rim = [np.asarray(p1, np.float64) + (np.asarray(p2, np.float64) - np.asarray(p1, np.float64)) * (i / n1) for i in range(n1)]
    rim += [np.asarray(p2, np.float64) + (np.asarray(p3, np.float64) - np.asarray(p2, np.float64)) * (i / n2) for i in range(n2)]
    rim.append(np.asarray(p3, np.float64))
    P = np.array([p0] + rim, np.float32)
    assert len(np.unique(P, axis=0)) == n + 2   # no two rim points fall together in f32: no degenerate triangle
    idx = np.array([[0, i + 1, i + 2] for i in range(n)], np.uint32)
    return core.GeometricPrimitive(core.TriangleMesh(idx, P), core.MatteMaterial((0.5, 0.5, 0.5)), core.DiffuseAreaLight(L, nSamples))


def blob_emitter(segments, rows, L=(14.0, 12.0, 10.0), radius=1.5, centre=(3.5, 5.5, 2.0)):
    """A closed emissive scenes.blob_mesh inside the box (2 * segments * rows triangles): the segment from a shaded point to the sampled
    point crosses two of its triangles, so ShapeSet.sample's walk over every triangle -- the last hit in list order wins -- decides Ns."""
    mesh = scenes.blob_mesh(segments, rows, radius=radius, centre=centre)
    mesh.reverseOrientation = True   # blob_mesh winds its triangles inwards and an area light is one-sided: emit outwards
    return core.GeometricPrimitive(mesh, core.MatteMaterial((0.5, 0.5, 0.5)), core.DiffuseAreaLight(L, 1))


def tiled_floor(k):
    """The Cornell floor as k GeometricPrimitives -- strips along x, two triangles each, wound like scenes.floor_quad -- each with a
    MatteMaterial of its own Kd: k material records (the upload keeps one per primitive)."""
    assert k >= 1
    xs = np.linspace(-10.0, 10.0, k + 1)
    return [scenes._quad((xs[i], -10, -10), (xs[i + 1], -10, -10), (xs[i + 1], -10, 10), (xs[i], -10, 10),
                         (0.15 + 0.7 * i / k, 0.45 + 0.3 * ((i * 7) % 11) / 11.0, 0.85 - 0.7 * i / k)) for i in range(k)]


def box_prims(emitters, floor=None, extras=()):
    """The Cornell walls (the floor replaced by `floor`, a list of primitives, if given) around the small matte blob, the emitters, and
    whatever else the kernel variant needs."""
    walls = scenes.cornell_walls()
    return (list(floor) if floor is not None else walls[:1]) + walls[1:] + list(emitters) + [scenes.blob_prim(12, 6)] + list(extras)
