"""tests/table_placement.py without a device: the constants it reads from the sources, its restated formulas against the worked numbers
of DESIGN.md section 3 ("Where the tables live"), the struct sizes against a host compile, the restated text against the launchers' own,
and the scene builders' exact table sizes."""
import os

import numpy as np
import pytest

import table_placement as tp
from dartray_amd import core, scenes

K = tp.K


@pytest.fixture(scope="module")
def sizes(tmp_path_factory):
    return tp.compiled_sizes(tmp_path_factory.mktemp("table_sizes"))


def _counts(sizes, nlights=1, nltris=2, ncdf=3, nmats=7):
    return {"nlights": nlights, "nltris": nltris, "ncdf": ncdf, "nmats": nmats, "sizeof_DLight": sizes["DLight"], "sizeof_DLightTri": sizes["DLightTri"]}


def test_the_parsed_constants_exist():
    for name in ("DR_LDS_LIGHT_BYTES", "DR_LDS_MAT_BYTES", "LDS_BYTES", "DR_PUSH_ITERS", "DR_SHADE_BLOCK", "DR_SHADE_BLOCK_GEN", "EDGE_BYTES",
                 "CDF_ENTRY_BYTES", "MAT_BYTES", "LISTS", "ENV_LISTS", "SIZEOF_PUSHSTAGE"):
        assert isinstance(K[name], int) and K[name] > 0, name
    assert K["DR_LDS_LIGHT_BYTES"] == K["DR_LDS_MAT_BYTES"] == 24 * 1024 and K["LDS_BYTES"] == 160 * 1024
    assert K["DR_SHADE_BLOCK"] > K["DR_SHADE_BLOCK_GEN"] and K["ENV_LISTS"] == K["LISTS"] + 1
    assert set(tp.LAUNCH_CONDITIONS) == {"k_shade_path", "k_shade_direct", "k_shade_whitted"}


def test_struct_sizes_against_a_host_compile(sizes):
    assert sizes["PushStage"] == K["SIZEOF_PUSHSTAGE"] == tp.push_stage_size_from_text()
    # stage_lights copies the records word by word and starts the f64 edges behind them: both must be 8-byte multiples
    assert sizes["DLight"] % 8 == 0 and sizes["DLightTri"] % 8 == 0


def test_the_worked_numbers(sizes):
    one, two = _counts(sizes, nltris=1, ncdf=2), _counts(sizes, nltris=2, ncdf=3)
    assert tp.light_table_bytes(two) - tp.light_table_bytes(one) == 124   # DLightTri + its edges + its CDF entry
    assert sizes["DLightTri"] + K["EDGE_BYTES"] + K["CDF_ENTRY_BYTES"] == 124
    assert tp.stage_bytes("path") == tp.stage_bytes("direct") == 99776
    assert tp.stage_bytes("path_env") == 124352
    assert tp.stage_bytes("path_gen") == tp.stage_bytes("direct_gen") == tp.stage_bytes("whitted") == 67008
    assert K["LDS_BYTES"] - tp.stage_bytes("path_env") == 39488   # "about 39 KiB is left for the tables"
    # the four-list forms always fit: both tables at their caps beside the larger staging block
    assert tp.stage_bytes("path") + K["DR_LDS_LIGHT_BYTES"] + K["DR_LDS_MAT_BYTES"] <= K["LDS_BYTES"]


def test_the_three_conditions_at_their_edges(sizes):
    per_tri = sizes["DLightTri"] + K["EDGE_BYTES"]
    # light tables exactly at the cap: one light, n triangles and the CDF entries that make up the rest
    n = (K["DR_LDS_LIGHT_BYTES"] - sizes["DLight"]) // (per_tri + 4)
    rest = K["DR_LDS_LIGHT_BYTES"] - sizes["DLight"] - n * per_tri
    at = _counts(sizes, nltris=n, ncdf=rest // 4)
    assert rest % 4 == 0 and tp.light_table_bytes(at) == K["DR_LDS_LIGHT_BYTES"]
    for v in tp.VARIANTS:
        assert tp.placement_of_counts(at, v) == "lds", v                                # `<=`: at the cap is inside
        assert tp.placement_of_counts(dict(at, ncdf=at["ncdf"] + 1), v) == "global", v  # four bytes more are outside
        assert tp.placement_of_counts(_counts(sizes, nlights=0, nltris=0, ncdf=1), v) == "global", v   # no light: nothing to stage
    cap = K["DR_LDS_MAT_BYTES"] // K["MAT_BYTES"]
    assert cap == 384
    for v in tp.VARIANTS:
        assert tp.placement_of_counts(_counts(sizes, nmats=cap), v) == "lds", v
        assert tp.placement_of_counts(_counts(sizes, nmats=cap + 1), v) == "lds_lights_global_mats", v
        assert tp.placement_of_counts(dict(at, ncdf=at["ncdf"] + 1, nmats=cap + 1), v) == "global", v
    # five staging lists: each table under its own cap, together over the room -- and only there
    room = K["LDS_BYTES"] - tp.stage_bytes("path_env")
    fit = dict(at, nmats=(room - K["DR_LDS_LIGHT_BYTES"]) // K["MAT_BYTES"])
    assert tp.light_table_bytes(fit) + tp.mat_table_bytes(fit) == room and tp.placement_of_counts(fit, "path_env") == "lds"
    over = dict(fit, nmats=fit["nmats"] + 1)
    assert tp.mat_table_bytes(over) and tp.placement_of_counts(over, "path_env") == "global"
    assert all(tp.placement_of_counts(over, v) == "lds" for v in tp.VARIANTS if v != "path_env")
    # a material table over its cap takes no room: the lights alone decide
    assert tp.placement_of_counts(dict(at, nmats=cap + 1), "path_env") == "lds_lights_global_mats"


def test_the_restated_blocks_are_the_ones_held_against_dr_kernels():
    """tests/test_whitted_integrator.py holds every block of dr_shade_common.h, word for word, against dr_kernels.hip; the functions restated
    here are in those blocks, and the blocks are in dr_kernels.hip -- so the text parse_constants() read is what both launch paths compile."""
    header, kernels = tp._text("dr_shade_common.h"), tp._text("dr_kernels.hip")
    body = header[header.index("#define DR_SHADE_COMMON_H") + len("#define DR_SHADE_COMMON_H"):header.rindex("#endif")]
    blocks = [b.strip() for b in body.split("\n\n") if b.strip()]
    code = lambda text: "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("//"))
    for name in ("DR_LDS_LIGHT_BYTES (", "DR_LDS_MAT_BYTES (", "DR_SHADE_BLOCK 768", "DR_SHADE_BLOCK_GEN 512", "inline size_t light_table_bytes(",
                 "inline size_t mat_table_bytes(", "static bool lightsInLds("):
        mine = [b for b in blocks if name in b]
        assert len(mine) == 1 and code(mine[0]) in code(kernels), name
    assert "dr_shade_common.h" in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_whitted_integrator.py")).read()


@pytest.mark.parametrize("n", [2, 3, 7, 197, 198, 300])
def test_fan_emitter_is_the_quad_in_exactly_n_triangles(n):
    fan, quad = tp.fan_emitter(n), scenes.emitter_quad()
    P, idx = fan.shape.P.astype(np.float64), fan.shape.vertexIndex
    assert len(idx) == n and fan.areaLight is not None and fan.areaLight.nSamples == 1
    assert np.array_equal(fan.areaLight.Lemit, quad.areaLight.Lemit)
    assert (P[:, 1] == np.float32(9.9)).all() and np.array_equal(P.min(axis=0), quad.shape.P.min(axis=0)) and np.array_equal(P.max(axis=0), quad.shape.P.max(axis=0))
    cross = np.cross(P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]])
    assert (cross[:, 1] < 0).all() and (cross[:, [0, 2]] == 0).all()   # every piece faces down like the quad, none is degenerate
    assert abs(0.5 * -cross[:, 1].sum() - 36.0) < 1e-4                  # together they are the 6 x 6 quad


def test_blob_emitter_and_tiled_floor():
    blob = tp.blob_emitter(15, 10)
    assert len(blob.shape.vertexIndex) == 300 and blob.areaLight is not None
    assert np.abs(blob.shape.P).max() < 10.0   # inside the box
    for k in (1, 5, 384):
        tiles = tp.tiled_floor(k)
        assert len(tiles) == k and len({tuple(t.material.Kd) for t in tiles}) == k and len({id(t.material) for t in tiles}) == k
        P = np.concatenate([t.shape.P for t in tiles])
        assert (P[:, 1] == -10).all() and P[:, 0].min() == -10 and P[:, 0].max() == 10 and all(len(t.shape.vertexIndex) == 2 for t in tiles)
        assert all(tiles[i].shape.P[:, 0].max() == tiles[i + 1].shape.P[:, 0].min() for i in range(k - 1))   # no gap, no overlap


def test_the_builders_straddle_the_caps_by_the_host_descriptor(sizes):
    """The sizes the GPU tests find from a probe scene's queried counts, here from the host descriptor's: the counts move by one light
    triangle and one CDF entry per fan triangle and by one material per tile, and the largest "lds" fan and the smallest "global" fan are
    neighbours on either side of the cap."""
    def counts(emitters, floor=None):
        return tp.host_counts(scenes.make_scene(tp.box_prims(emitters, floor)), sizes["DLight"], sizes["DLightTri"])
    probe = counts([tp.fan_emitter(2)])
    assert probe == _counts(sizes, nlights=1, nltris=2, ncdf=3, nmats=7)
    n_lds, n_global = tp.fan_sizes(probe, "path", 2)
    assert n_global == n_lds + 1
    a, b = counts([tp.fan_emitter(n_lds)]), counts([tp.fan_emitter(n_global)])
    assert a == tp.with_fan(probe, n_lds, 2) and b == tp.with_fan(probe, n_global, 2)
    assert tp.light_table_bytes(a) <= K["DR_LDS_LIGHT_BYTES"] < tp.light_table_bytes(b)
    k = K["DR_LDS_MAT_BYTES"] // K["MAT_BYTES"] - (probe["nmats"] - 1)
    at, over = counts([tp.fan_emitter(2)], tp.tiled_floor(k)), counts([tp.fan_emitter(2)], tp.tiled_floor(k + 1))
    assert at == tp.with_tiles(probe, k, 1) and over == tp.with_tiles(probe, k + 1, 1)
    assert at["nmats"] * K["MAT_BYTES"] == K["DR_LDS_MAT_BYTES"]
    assert tp.placement_of_counts(at, "path") == "lds" and tp.placement_of_counts(over, "path") == "lds_lights_global_mats"
    # two emitters: a light record, a material and a CDF end more
    two = counts([tp.fan_emitter(5, centre=(-4.0, 0.0), half=2.5), tp.fan_emitter(9, nSamples=3, centre=(4.0, 0.0), half=2.5)])
    assert two == _counts(sizes, nlights=2, nltris=14, ncdf=16, nmats=8)
