"""Every traversal kernel against the oracle, ray by ray, on rays built to land inside the band of the f32 slab filter
(tests/band_rays.py): hit records bit-exact, visit counters equal.  Caller rays (dr_intersect) reach k_intersect<0/1>,
k_intersect3<0> and k_intersect3a in either any-hit order; the state-array kernels (k_trace, k_trace3, k_trace3c, k_trace_pk) are
held through films and counters of a render of the same scene."""
import ctypes as C

import numpy as np
import pytest

import band_rays as br
from dartray_amd import _abi, core, scenes
from test_gpu_intersect import _compare
from test_oracle_bvh import SCENES

pytestmark = pytest.mark.gpu

CLOSEST = ("closest_rays", "closest_nodes", "closest_tris")
ANY = ("any_rays", "any_nodes", "any_tris")


def _npairs(dev):
    n = C.c_uint64(0)
    _abi.check(_abi.lib().dr_scene_get_pairs(dev.handle, None, 0, C.byref(n), None, None))
    return int(n.value)


class _own_kernels:
    """Hide an inherited DARTRAY_TRACE_IMPL (the suite is also run with it set): the scene's own kernel ids decide."""

    def __enter__(self):
        _abi.check(_abi.lib().dr_set_option(b"TRACE_IMPL", b""))

    def __exit__(self, *exc):
        _abi.check(_abi.lib().dr_set_option(b"TRACE_IMPL", None))


_scenes = {}


def _band_scene(scale):
    """The band scene on the device (one per scale for the whole module); its tree is the oracle's, byte for byte."""
    if scale not in _scenes:
        scene = scenes.make_scene(br.band_prims(scale))
        nodes, tri, _, _ = br.oracle_scene(scale).bvh()
        assert scene.aggregate.nodes.tobytes() == nodes.tobytes() and np.array_equal(scene.aggregate.tri_idx, tri)
        assert _npairs(scene._device()) > 0   # a pair layout exists: ids 3 / 7 do not fall back to k_intersect
        _scenes[scale] = scene
    return _scenes[scale]


@pytest.mark.parametrize("name", br.FAMILIES)
@pytest.mark.parametrize("kernels", [(2, 2), (3, 3), (2, 6), (3, 7)], ids=lambda k: "k%d-%d" % k)
def test_band_rays_ray_by_ray(ob, gpu, kernels, name):
    """20 000 rays of one family through one (closest, any-hit) kernel pair: prim, t, b1, b2 equal the oracle's bit for bit, the
    occlusion booleans too, and so do the closest-hit counters.  The any-hit counters equal the oracle's for ids 2 / 3; for 6 / 7
    (far child first) they equal the oracle's far-first walk of the same rays -- its order study runs inside intersectP, so it
    counts dr_intersect-style batches as well as renders."""
    r = br.family(name)
    scene = _band_scene(br.SCALES[name])
    dev = scene._device()
    rays = core.Ray(r["o"], r["d"], r["tmin"], r["tmax"])
    with _own_kernels():
        assert dev.trace_kernels(kernels) == kernels
        dev.reset_stats()
        h = scene.intersect(rays)
        st = dev.stats()
        for k in ("prim", "t", "b1", "b2"):
            assert np.array_equal(h[k], r["closest"][k]), k
        assert [st[k] for k in CLOSEST] == [r["counters"][k] for k in CLOSEST]
        assert [st[k] for k in ANY] == [0, 0, 0]
        dev.reset_stats()
        occluded = scene.intersectP(rays)
        st = dev.stats()
        assert np.array_equal(occluded, r["occluded"])
        assert [st[k] for k in CLOSEST] == [0, 0, 0]   # the closest-hit side is untouched
        c, study = r["any_counters"], r["far_first"]
        assert (study["rays"], study["nodes_all"], study["tris_all"]) == (c["any_rays"], c["any_nodes"], c["any_tris"])
        if kernels[1] in (2, 3):
            assert [st[k] for k in ANY] == [c[k] for k in ANY]
        else:
            assert st["any_rays"] == c["any_rays"]
            assert st["any_nodes"] == study["nodes_all"] - study["nodes_occ_ref"] + study["nodes_occ_far_first"]
            assert st["any_tris"] == study["tris_all"] - study["tris_occ_ref"] + study["tris_occ_far_first"]


@pytest.mark.parametrize("name", list(SCENES))
def test_hit_records_match_oracle_under_the_pair_kernels(ob, gpu, name):
    """tests/test_gpu_intersect.py::test_hit_records_match_oracle once more with k_intersect3<0> / k_intersect3a, for every entry of
    SCENES that has a pair layout (a default run of the suite otherwise compares only k_intersect<0/1> ray by ray)."""
    prims = SCENES[name]()
    if _npairs(scenes.make_scene(prims)._device()) == 0:
        pytest.skip("no pair layout: this scene runs k_intersect by design")
    with _own_kernels():
        h = _compare(ob, prims, 50000, seed=21, kernels=(3, 3))
    assert (h["prim"] >= 0).sum() > 100


def _render_case(ob, kernels, coherent):
    """24 x 20 pixels, 16 spp, path depth 3, a perspective camera off every axis looking at the shingle stack and the blob."""
    scene = _band_scene(1.0)
    dev = scene._device()
    film = core.ImageFilm(24, 20, core.BoxFilter(0.5, 0.5))
    cam = core.PerspectiveCamera.lookAt((-17.5, 1.75, 0.5), (-13.5, 0.0, 3.0), (0.0, 1.0, 0.0), 70.0, film)
    r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 16), cam, core.PathIntegrator(3), core.EmissionIntegrator())
    lib = _abi.lib()
    with _own_kernels():
        assert dev.trace_kernels(kernels) == kernels
        if coherent is not None:
            _abi.check(lib.dr_set_option(b"COHERENT_CAMERA", coherent))
        try:
            out = r.render(scene)
        finally:
            _abi.check(lib.dr_set_option(b"COHERENT_CAMERA", None))
        info, st = dev.last_render_info(), r.last_stats
    assert (info["closest_kernel"], info["any_hit_kernel"]) == kernels, info
    if coherent is not None:
        assert info["coherent_camera"] == int(coherent), info
        cs = dev.coherent_stats()
        assert (cs["rays"] > 0) == (coherent == b"1")
    osc = br.oracle_scene(1.0)
    osc.counters(reset=True)
    ref = osc.render(ob.render_desc(r, sampler_mode=1))
    c = osc.counters()
    assert np.array_equal(out.film, ref["film"])
    assert [st[k] for k in CLOSEST + ANY] == [c[k] for k in CLOSEST + ANY]
    assert out.film[..., :3].max() > 0 and c["closest_nodes"] > 10 * c["closest_rays"]


@pytest.mark.parametrize("kernels,coherent", [((2, 2), None), ((3, 3), None), ((5, 3), None),
                                              ((2, 2), b"1"), ((2, 2), b"0"), ((5, 3), b"1"), ((5, 3), b"0")],
                         ids=lambda v: "default" if v is None else ("k%d-%d" % v if isinstance(v, tuple) else "coherent" + v.decode()))
def test_state_array_kernels_render_the_band_scene(ob, gpu, kernels, coherent):
    """k_trace, k_trace3, k_trace3c (its brackets derived from one neighbouring float) and k_trace_pk (one stack per wave) cannot
    take caller rays: they render the band scene, whose coincident planes the camera and bounce rays meet, and film and all six
    visit counters must equal the oracle's; last_render_info says the requested kernels ran."""
    _render_case(ob, kernels, coherent)
