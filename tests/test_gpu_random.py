"""The random device sampler (DR_SAMPLER_RANDOM) on the GPU, bit for bit: the vectors (dr_generate_samples) against the
Python restatement (tests/random_restatement.py), and the films against the host-buffer replay of those restated vectors with the
matching kind-2 tails.  The arithmetic is integer generator steps and one exact conversion, so every comparison is equality of bit
patterns.  Nothing is started after a failed call: every call's return code raises."""
import ctypes as C

import numpy as np
import pytest

from dartray_amd import _abi, core, scenes

import random_restatement as rr

pytestmark = pytest.mark.gpu

PATH_SLOTS = rr.slot_counts(1, [1])  # PathIntegrator: SAMPLE_DEPTH = 3 requested bounces; from the fourth vertex on Li draws on kind 2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rand(r, spp, seed=5489):
    r.sampler = core.RandomSampler(r.camera, spp, seed)
    return r


def _block(x0, y0, w, h):
    return np.array([(x0 + x, y0 + y) for y in range(h) for x in range(w)], np.int32)


@pytest.fixture(scope="module")
def c2small(gpu):
    """The small Cornell box with the blob (tests/golden/make_golden.py's c2small): 16 x 16 film, path, maxdepth 5."""
    prims, mk = scenes.config("C2", xres=16, yres=16, spp=4, blob=(32, 16))
    return prims, mk, scenes.make_scene(prims)


def _dump(c2small, pixels, spp, seed):
    prims, mk, scene = c2small
    r = _rand(mk(), spp, seed)
    got = r.generate_samples(scene, pixels)
    want = rr.keyed_vectors(seed, rr.sample_extent(r.camera.film), pixels, spp, *PATH_SLOTS)
    return got, want


# ---- 1. the dump against the restatement ----
SHAPES = {"5x3x4_under_a_wave": (_block(2, 1, 5, 3), 4), "9x7x8_two_ragged_workgroups": (_block(4, 6, 9, 7), 8),
          "2x2x64_a_wave_per_pixel": (_block(15, 15, 2, 2), 64), "2x2x128_two_waves_per_pixel": (_block(0, 0, 2, 2), 128),
          "3x1x1_spp_1": (_block(7, 16, 3, 1), 1)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_generated_vectors_equal_the_restatement(c2small, shape):
    pixels, spp = SHAPES[shape]
    got, want = _dump(c2small, pixels, spp, 5489 if spp != 8 else 77)
    assert got.shape == want.shape == (len(pixels) * spp, 37)
    assert np.array_equal(_bits(got), _bits(want))


# ---- 2. slots of several entries under DirectLighting "all" ----
def test_multi_entry_slots_come_out_in_draw_order(gpu):
    prims = [scenes.floor_quad(), scenes.emitter_quad(), scenes.emitter_quad(L=(20.0, 20.0, 20.0), half=1.0, y=9.0)]
    lights = [gp.areaLight for gp in prims if gp.areaLight is not None]
    lights[0].nSamples, lights[1].nSamples = 4, 1
    cam = scenes.cornell_camera(16, 16)
    r = core.SamplerRenderer(core.RandomSampler(cam, 2, 31), cam, core.DirectLightingIntegrator(0, 5), core.EmissionIntegrator())
    scene = scenes.make_scene(prims)
    ns = [L.nSamples for L in scene.lights]
    assert sorted(ns) == [1, 4]
    n1D, n2D = rr.slot_counts(0, ns)
    pixels = _block(3, 5, 4, 4)
    got = r.generate_samples(scene, pixels)
    want = rr.keyed_vectors(31, rr.sample_extent(cam.film), pixels, 2, n1D, n2D)
    assert got.shape == want.shape == (32, 5 + 12 + 20)
    assert np.array_equal(_bits(got), _bits(want))
    out = r.render(scene)
    assert np.isfinite(out.film).all() and out.rgb.mean() > 0.01


# ---- 3. / 4. the render ----
@pytest.fixture(scope="module")
def whole_film(c2small):
    prims, mk, scene = c2small
    r = _rand(mk(), 4)
    out = r.render(scene)
    return out, scene._device().last_render_info(), r.last_stats


def test_render_equals_the_host_buffer_replay_of_the_restated_vectors(c2small, whole_film):
    prims, mk, scene = c2small
    out, info, stats = whole_film
    r = mk()
    pixels = r.pixels()
    assert len(pixels) == 17 * 17
    ext = rr.sample_extent(r.camera.film)
    vec = rr.keyed_vectors(5489, ext, pixels, 4, *PATH_SLOTS)
    mt = rr.need_tail(1, 5, len(scene.lights))
    assert mt == 32
    r.sampler = core.HostBufferSampler(r.camera, 4, pixels, vec, rr.li_stream_tail(5489, ext, pixels, 4, mt))
    replay = r.render(scene)
    assert np.array_equal(out.film, replay.film) and np.array_equal(out.rgb, replay.rgb)
    assert out.rgb.mean() > 0.01 and np.isfinite(out.film).all()
    # dr_scene_last_render_info and the stats speak of this render as of any pixel-bound mode's
    assert info["state_layout"] in (4, 64) and info["batches"] == 1 and info["lazy_gen"] == 0
    assert stats["camera_samples"] == 17 * 17 * 4
    # ... which is no other sampler's image
    assert not np.array_equal(out.film, mk().render(scene).film)


def test_any_split_traces_the_same_samples(c2small, whole_film):
    prims, mk, scene = c2small
    one = whole_film[0].film
    kw = dict(xres=16, yres=16, spp=4, blob=(32, 16))
    tasks = sum(_rand(scenes.config("C2", taskNum=k, taskCount=2, **kw)[1](), 4).render(scene).film for k in range(2))
    assert np.array_equal(tasks, one)
    tiles = sum(_rand(scenes.config("C2", tileRank=k, tileCount=2, tileSize=8, **kw)[1](), 4).render(scene).film for k in range(2))
    assert np.array_equal(tiles, one)


# ---- 5. the slow-draw switch ----
def test_slow_draws_switch_leaves_the_streams_alone(c2small):
    pixels, spp = SHAPES["9x7x8_two_ragged_workgroups"]
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(b"GEN_SLOW_DRAWS", b"1"))
        got, want = _dump(c2small, pixels, spp, 77)
    finally:
        lib.dr_set_option(b"GEN_SLOW_DRAWS", None)
    assert np.array_equal(_bits(got), _bits(want))


# ---- 6. it is not another sampler ----
def test_the_image_samples_are_not_one_per_stratum(c2small):
    prims, mk, scene = c2small
    pixels, spp = SHAPES["2x2x64_a_wave_per_pixel"]
    got, want = _dump(c2small, pixels, spp, 5489)
    r = mk()
    r.sampler = core.StratifiedSampler(r.camera, 8, 8, True, 5489)
    strat = r.generate_samples(scene, pixels)
    assert strat.shape == got.shape and not np.array_equal(_bits(strat), _bits(got))

    def cells(v):  # the 8 x 8 cell of every image sample, per pixel
        return (np.floor(v[:, 0].astype(np.float64) * 8) + 8 * np.floor(v[:, 1].astype(np.float64) * 8)).astype(int).reshape(len(pixels), spp)

    assert np.array_equal(cells(got), cells(want))
    # 64 uniform draws fill all 64 cells with probability 64! / 64^64 per pixel; the restatement says which cells repeat, the device agrees
    assert any(len(set(row)) < spp for row in cells(want))
    assert all(sorted(row) == list(range(spp)) for row in cells(strat))


# ---- 7. refusals through the device entry point ----
def test_limits_are_refused_by_name_and_leave_the_scene_usable(c2small, whole_film):
    prims, mk, scene = c2small
    lib = _abi.lib()
    film = np.zeros((16, 16, 4), np.float32)

    def refused(r, sc, needle, mutate=None):
        d, keep = r.describe()
        if mutate:
            mutate(d)
        rc = lib.dr_render(sc._device().handle, C.byref(d), film.ctypes.data, None)
        assert rc == -4, rc  # DR_ERR_UNSUPPORTED
        assert needle in lib.dr_last_error().decode(), lib.dr_last_error()

    for spp in (3, 8192, 0):
        refused(_rand(mk(), 4), scene, "random sampler: pixelsamples (spp) must be a power of two, at most 4096", lambda d: setattr(d, "spp", spp))
    assert np.array_equal(_rand(mk(), 4).render(scene).film, whole_film[0].film)  # the scene still renders
    # a light with nsamples = 3 under DirectLighting "all": roundSize is the identity, the scene's slot layout is the rounded one
    prims1, mk1 = scenes.config("C1", xres=16, yres=16, spp=4)
    next(gp for gp in prims1 if gp.areaLight is not None).areaLight.nSamples = 3
    scene1 = scenes.make_scene(prims1)
    refused(_rand(mk1(), 4), scene1, "random sampler: a light's nsamples must be a power of two (RandomSampler.roundSize is the identity")
    r = _rand(mk1(), 4)
    r.surfaceIntegrator = core.PathIntegrator(3)  # (the path integrator asks for one entry per slot whatever nsamples says)
    assert np.isfinite(r.render(scene1).film).all()
