"""The shading kernels against the oracle on both sides of the table caps ("Where the tables live").

k_shade_path and k_shade_direct are compiled in two forms -- light tables in LDS (LdsLights, with or without the material table beside
them) or in global memory (GlobalLights) -- and the launcher picks one from the byte sizes of the scene's tables.  The forms run different
code (stage_lights' copy and its pre-evaluated f64 edges, lds_read_struct, the global read of mat() from inside the LDS view) and must
give the same bytes.  Every case here states the form it means to run, asserts it from the scene's own counts
(tests/table_placement.py::placement over dr_scene_get_table_counts) and then holds the render against the oracle like
tests/test_gpu_shading.py::_parity: film bit for bit (matte, mirror and glass only), the six traversal counters, a lit image.  Under the
environment light the film has tests/test_gpu_cameras.py's allowance for the device library's sin / cos, and only there.

Sizes are not written down here: each emitter's triangle count and each floor's tile count is found with the restated formula from the
counts of a probe scene (the same scene with a fan of two triangles over a floor of one tile), then asserted on the scene that renders.
Film 16 x 12, 4 samples per pixel; k_shade_whitted's cases are in tests/test_gpu_whitted.py."""
import numpy as np
import pytest

import table_placement as tp
from dartray_amd import core, pbrt, scenes
from util import rel_err_image

pytestmark = pytest.mark.gpu

K = tp.K


def _specular_extras():
    """A glass sphere and a mirror quad: the general shading kernels."""
    at = pbrt.Transform.Translate(6.5, -7.5, -4.0)
    sphere = core.GeometricPrimitive(core.Sphere(at.m, at.mInv, False, 2.0), core.GlassMaterial((1.0, 1.0, 1.0), (1.0, 0.95, 0.9), 1.5))
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                             np.array([(-9.0, -6.0, 8.0), (-9.0, 5.0, 8.0), (-6.5, 5.0, 1.0), (-6.5, -6.0, 1.0)], np.float32))
    return [sphere, core.GeometricPrimitive(mesh, core.MirrorMaterial((0.9, 0.85, 0.8)))]


# run -> (kernel variant of tests/table_placement.py, integrator, specular extras)
RUNS = {
    "path": ("path", lambda: core.PathIntegrator(4), False),
    "path_env": ("path_env", lambda: core.PathIntegrator(4), False),
    "path_gen": ("path_gen", lambda: core.PathIntegrator(5), True),
    "direct": ("direct", lambda: core.DirectLightingIntegrator(0, 5), False),
    "direct_gen": ("direct_gen", lambda: core.DirectLightingIntegrator(0, 5), True),
    "direct_gen_one": ("direct_gen", lambda: core.DirectLightingIntegrator(1, 5), True),   # SAMPLE_ONE_UNIFORM
}
CELLS = ["fan_largest-lds", "fan_smallest-global", "blob_300-global", "tiles_at_cap-lds", "tiles_over_cap-lds_lights_global_mats",
         "both_over-global"]
ENV_CELLS = ["together_just_fit-lds", "together_over-global"]

_env = {}
_probe = {}


def _sky():
    if "sky" not in _env:
        _env["sky"] = scenes.sky_env(32, 16)
    return _env["sky"]


def _scene(run, emitters, floor=None):
    variant, _, spec = RUNS[run]
    prims = tp.box_prims(emitters, floor, _specular_extras() if spec else ())
    env = _sky() if tp.VARIANTS[variant].env else None
    return prims, env, scenes.make_scene(prims, env)


def _probe_counts(run, nfans=1):
    """The counts of the run's scene with fans of two triangles over a floor of one tile: what the sizes are worked out from."""
    if (run, nfans) not in _probe:
        fans = [tp.fan_emitter(2, centre=(8.0 * i - 4.0 * (nfans - 1), 0.0), half=2.5) for i in range(nfans)]
        _probe[(run, nfans)] = tp.table_counts(_scene(run, fans)[2])
    return dict(_probe[(run, nfans)])


def _tiles_at_cap(c):
    """The largest tile count whose material table still goes to LDS, for a scene of counts c over one tile."""
    k = max(k for k in range(1, 1000) if tp.mat_table_bytes(tp.with_tiles(c, k, 1)))
    assert tp.with_tiles(c, k, 1)["nmats"] * K["MAT_BYTES"] == K["DR_LDS_MAT_BYTES"]   # exactly at the cap: the `<=`
    return k


def _parity(ob, run, prims, env, scene, want, counts=None):
    variant, integ, _ = RUNS[run]
    got = tp.table_counts(scene)
    print("%s: %s -> light tables %d B (cap %d), material table %d B (cap %d), staging %d B of %d" % (
        run, got, tp.light_table_bytes(got), K["DR_LDS_LIGHT_BYTES"], got["nmats"] * K["MAT_BYTES"], K["DR_LDS_MAT_BYTES"],
        tp.stage_bytes(variant), K["LDS_BYTES"]))
    if counts is not None:
        assert got == counts
    assert tp.placement(scene, variant) == want
    film = core.ImageFilm(16, 12)
    cam = core.PerspectiveCamera.lookAt((0, 0, -35), (0, 0, 0), (0, 1, 0), 35.0, film)
    r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 4), cam, integ(), core.EmissionIntegrator())
    out = r.render(scene)
    osc = ob.OracleScene(prims, env=env) if env is not None else ob.OracleScene(prims)
    osc.counters(reset=True)
    ref = osc.render(ob.render_desc(r, sampler_mode=1))
    assert rel_err_image(out.rgb, ref["rgb"]).max() <= 1e-4
    if env is None:
        assert np.array_equal(out.film, ref["film"])
    else:   # sin / cos of the device maths library: an ulp now and then (tests/test_gpu_cameras.py)
        assert np.allclose(out.film, ref["film"], rtol=2e-5, atol=1e-6)
    c, st = osc.counters(), r.last_stats
    for k in ("closest_rays", "any_rays", "closest_nodes", "any_nodes", "closest_tris", "any_tris"):
        assert st[k] == c[k], k
    assert out.rgb.mean() > 0.02 and (out.rgb.max(axis=2) > 0).mean() > 0.5
    return out


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("run", list(RUNS))
def test_both_sides_of_the_caps(ob, gpu, run, cell):
    variant = RUNS[run][0]
    what, want = cell.split("-")
    c = _probe_counts(run)
    n_lds, n_global = tp.fan_sizes(c, variant, 2)
    assert n_global == n_lds + 1
    k_cap = _tiles_at_cap(c)
    if what == "fan_largest":
        counts = tp.with_fan(c, n_lds, 2)
        # the `<=` edge, or as near below it as one more triangle allows
        assert K["DR_LDS_LIGHT_BYTES"] - tp.light_table_bytes(counts) < c["sizeof_DLightTri"] + K["EDGE_BYTES"] + K["CDF_ENTRY_BYTES"]
        emitters, floor = [tp.fan_emitter(n_lds)], None
    elif what == "fan_smallest":
        counts = tp.with_fan(c, n_global, 2)
        emitters, floor = [tp.fan_emitter(n_global)], None
    elif what == "blob_300":
        counts = None
        emitters, floor = [tp.blob_emitter(15, 10)], None
    elif what == "tiles_at_cap":
        counts = tp.with_tiles(c, k_cap, 1)
        emitters, floor = [tp.fan_emitter(2)], tp.tiled_floor(k_cap)
    elif what == "tiles_over_cap":
        counts = tp.with_tiles(c, k_cap + 1, 1)
        emitters, floor = [tp.fan_emitter(2)], tp.tiled_floor(k_cap + 1)
    else:
        counts = tp.with_tiles(tp.with_fan(c, n_global, 2), k_cap + 1, 1)
        emitters, floor = [tp.fan_emitter(n_global)], tp.tiled_floor(k_cap + 1)
    prims, env, scene = _scene(run, emitters, floor)
    if what == "blob_300":
        got = tp.table_counts(scene)
        assert got["nltris"] == 300 and not tp.lights_in_lds(got)
    _parity(ob, run, prims, env, scene, want, counts)


def _together(c):
    """(n, k): the fan and the floor for which the two tables, each under its own cap, fill what five staging lists leave as nearly as
    any pair with 140 to 180 emissive triangles does."""
    room = K["LDS_BYTES"] - tp.stage_bytes("path_env")
    best = None
    for n in range(140, 181):
        cn = tp.with_fan(c, n, 2)
        if not tp.lights_in_lds(cn):
            continue
        for k in range(1, _tiles_at_cap(c) + 1):
            cc = tp.with_tiles(cn, k, 1)
            used = tp.light_table_bytes(cc) + tp.mat_table_bytes(cc)
            if used <= room and (best is None or (used, -abs(n - 160)) > best[0]):
                best = ((used, -abs(n - 160)), n, k)
    return best[1], best[2], room - best[0][0]


@pytest.mark.parametrize("cell", ENV_CELLS)
def test_env_variant_where_the_two_tables_compete_for_the_room(ob, gpu, cell):
    """k_shade_path<true,false,*> stages five lists per wave at 768 threads: each table may pass its own cap and the two still not fit
    together beside them."""
    what, want = cell.split("-")
    c = _probe_counts("path_env")
    n, k, slack = _together(c)
    print("fan %d, tiles %d: %d B short of the room" % (n, k, slack))
    assert slack < K["MAT_BYTES"]
    if what == "together_over":
        k += 1   # one material record more: 64 B over, each table still under its own cap
    counts = tp.with_tiles(tp.with_fan(c, n, 2), k, 1)
    assert tp.lights_in_lds(counts) and tp.mat_table_bytes(counts)
    assert tp.placement_of_counts(counts, "path") == "lds"   # the four-list form would keep them
    prims, env, scene = _scene("path_env", [tp.fan_emitter(n)], tp.tiled_floor(k))
    _parity(ob, "path_env", prims, env, scene, want, counts)


@pytest.mark.parametrize("want", ["lds", "global"])
def test_two_emitters_whose_tables_cross_the_cap_together(ob, gpu, want):
    """The second emitter (nSamples 3) starts neither the triangle table nor the CDF: first_tri and cdf_off of a light that is not the
    first, in both views.  Neither emitter passes the cap alone."""
    run = "direct_gen"
    c = _probe_counts(run, nfans=2)
    t_lds, t_global = tp.fan_sizes(c, "direct_gen", 4, lo=4)
    total = t_lds if want == "lds" else t_global
    n1 = total // 2
    n2 = total - n1
    counts = tp.with_fan(c, total, 4)
    for n in (n1, n2):   # either one alone: a light, its material, its triangles and its CDF (n + 1 entries) less
        alone = dict(counts, nlights=counts["nlights"] - 1, nmats=counts["nmats"] - 1, nltris=n, ncdf=n + 1)
        assert tp.placement_of_counts(alone, "direct_gen") == "lds" and n > 50
    fans = [tp.fan_emitter(n1, centre=(-4.0, 0.0), half=2.5), tp.fan_emitter(n2, L=(10.0, 30.0, 50.0), nSamples=3, centre=(4.0, 0.0), half=2.5)]
    prims, env, scene = _scene(run, fans)
    assert [L.nSamples for L in scene.lights] == [1, 3]
    _parity(ob, run, prims, env, scene, want, counts)
