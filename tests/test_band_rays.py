"""The band rays of tests/band_rays.py, checked without a GPU: the restated filter never contradicts the restated literal test (the
constants 2^-21 and 1e-37 are sound), a filter a few bits too narrow WOULD contradict it on these rays (the inputs are sharp), the
rays sit in the band, and the oracle's accelerator agrees with exhaustive testing on them (so it is a fit reference for the
kernels, tests/test_gpu_traversal_band.py)."""
import numpy as np
import pytest

import band_rays as br

BAND = ("edge", "tmax", "tmin")


def _boxes(r, nodes):
    return nodes["bmin"][r["target"]], nodes["bmax"][r["target"]]


@pytest.fixture(scope="module")
def million(ob):
    """170 000 rays of every family (1.02 million), candidates as drawn; per family (rays, node array)."""
    out = {}
    for name in br.FAMILIES:
        osc = br.oracle_scene(br.SCALES[name])
        out[name] = (br.band_family(name, osc, 170000, seed=11, clean=False), osc.bvh()[0])
    return out


def _contradictions(r, bmin, bmax, **kw):
    hit = br.slab_f64(r["o"], r["d"], r["tmin"], r["tmax"], bmin, bmax)[0]
    sure_hit, sure_miss = br.slab_f32_sure(r["o"], r["d"], r["tmin"], r["tmax"], bmin, bmax, **kw)
    assert not (sure_hit & sure_miss).any()
    return int(((sure_hit & ~hit) | (sure_miss & hit)).sum())


def test_the_scene(ob):
    osc = br.oracle_scene(1.0)
    assert osc.depth > 32 and osc.nprims <= 3000
    assert len(br.shingle_mesh().vertexIndex) == 80   # 40 quads
    for name in br.FAMILIES:
        r = br.family(name)
        nd = br.oracle_scene(br.SCALES[name]).bvh()[0]
        assert len(r["o"]) == 20000 and np.all(np.isfinite(r["o"])) and np.all(np.isfinite(r["d"])) and np.all(r["d"] != 0)
        if name != "facehit":
            depth = br.node_depths(nd)[r["target"]]
            leaf = nd["nprims"][r["target"]] > 0
            assert 0.3 < leaf.mean() < 0.7 and len(np.unique(depth[leaf])) >= 4 and len(np.unique(depth[~leaf])) >= 8
            for k in range(3):  # both signs of every direction component
                assert 0.3 < (r["d"][:, k] > 0).mean() < 0.7
    r = br.family("tmin")
    assert (r["tmin"] < 0).sum() > 1000 and (r["tmax"] <= 0).sum() > 1000 and (r["tmax"] == 0).sum() > 100


def test_restated_slab_test_is_the_oracles(ob):
    """slab_f64 against the oracle's own slab function (orc_slab), on the rays' target boxes and on the root."""
    for name in br.FAMILIES:
        r = br.family(name)
        nodes = br.oracle_scene(br.SCALES[name]).bvh()[0]
        pick = np.arange(0, 20000, 40)
        for boxes in (_boxes(r, nodes), (nodes["bmin"][np.zeros(20000, int)], nodes["bmax"][np.zeros(20000, int)])):
            mine = br.slab_f64(r["o"], r["d"], r["tmin"], r["tmax"], *boxes)[0]
            for i in pick:
                bmin, bmax = np.ascontiguousarray(boxes[0][i]), np.ascontiguousarray(boxes[1][i])
                assert bool(ob.lib().orc_slab(bmin.ctypes.data, bmax.ctypes.data, r["rays"][i:i + 1].ctypes.data)) == bool(mine[i]), (name, i)


def test_filter_constants_are_sound(million):
    """On a million band rays the filter's sureHit / sureMiss never contradicts the literal test -- at the box each ray was built
    for, and at the root box."""
    total = 0
    for name, (r, nodes) in million.items():
        total += len(r["o"])
        assert _contradictions(r, *_boxes(r, nodes)) == 0, name
        root = np.zeros(len(r["o"]), int)
        assert _contradictions(r, nodes["bmin"][root], nodes["bmax"][root]) == 0, name
    assert total >= 10 ** 6


def test_inputs_are_sharp(million):
    """With R = 2^-25 and A = 0 (an enclosure narrower than the rounding error of the f32 products) the same rays DO catch the filter
    contradicting the literal test, in each of the three band families at either scale: a kernel whose band is a few bits too
    narrow cannot pass on them.  Likewise the 20 000 rays per family that the GPU tests trace."""
    for name in BAND + ("tiny", "huge"):
        r, nodes = million[name]
        assert _contradictions(r, *_boxes(r, nodes), R=2.0 ** -25, A=0.0) > 0, name
        r, nodes = br.family(name), br.oracle_scene(br.SCALES[name]).bvh()[0]
        assert _contradictions(r, *_boxes(r, nodes), R=2.0 ** -25, A=0.0) > 0, name


def test_coverage_floor(million):
    """At least half of the rays of every band family are ambiguous at the box they were built for (a condition on the inputs)."""
    for name in BAND:
        assert million[name][0]["ambiguous"].mean() >= 0.5, name
        assert br.family(name)["ambiguous"].mean() >= 0.5, name
    for name in ("tiny", "huge"):
        for r in (million[name][0], br.family(name)):
            for part in range(3):
                assert r["ambiguous"][r["part"] == part].mean() >= 0.5, (name, part)


@pytest.mark.parametrize("name", br.FAMILIES)
def test_oracle_equals_brute_force(ob, name):
    """BVHAccel.intersect / intersectP of the oracle against exhaustive testing on the 20 000 rays per family that the GPU tests
    trace.  Left out, by the criterion itself applied to the brute-force result: a triangle hit at exactly t == maxDistance or
    t == minDistance, which Triangle.intersect accepts and the strict leaf-box test loses (tests/test_gpu_intersect.py::
    test_edge_cases) -- under 1 % of a family."""
    r = br.family(name)
    osc = br.oracle_scene(br.SCALES[name])
    b = osc.intersect(r["rays"], brute=True)
    bp = osc.intersect(r["rays"], any_hit=True, brute=True)["prim"] >= 0
    out = (b["prim"] >= 0) & ((b["t"] == r["tmax"]) | (b["t"] == r["tmin"]))
    assert out.mean() < 0.01
    keep = ~out
    h = r["closest"]
    assert np.array_equal(h["prim"][keep], b["prim"][keep]) and np.array_equal(h["t"][keep], b["t"][keep])
    assert np.array_equal(r["occluded"][keep], bp[keep])
    assert (h["prim"] >= 0).sum() > 2000 and (h["prim"] < 0).sum() > 0 if name != "facehit" else (h["prim"] >= 0).all()
    if name != "tiny":   # (at 2^-100 Triangle.intersectP underflows and reports nothing: band_family)
        assert r["occluded"].sum() > 2000
    if br.SCALES[name] == 1.0:
        assert r["counters"]["max_stack"] > 32   # the rays reach the deep part of the tree
