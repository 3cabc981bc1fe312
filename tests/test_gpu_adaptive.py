"""The adaptive sampler (DR_SAMPLER_ADAPTIVE) on the GPU against the frozen oracle.  The oracle side of every case
(tests/adaptive_restatement.py: oracle_adaptive) records the radiances of a counter-mode render at minSamples, applies the
Python restatement of needsSupersampling, and composes the expected film from two more counter-mode renders: the
unflagged pixels at minSamples + the flagged pixels at maxSamples.  Each case asserts that the oracle's flagged set is
neither empty nor everything, that the device supersampled exactly that set, and -- box filter -- that film and rgb are
bit-equal; the gaussian case uses the tolerance of tests/test_gpu_filters.py (atomically added splats).
Every render's return code raises (core: _abi.check), so nothing is started after a failed call."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from dartray_amd import _abi, core, scenes

import adaptive_restatement as ar

pytestmark = pytest.mark.gpu


def _adaptive(r, mins, maxs, seed=5489):
    r.sampler = core.AdaptiveSampler(r.camera, mins, maxs, "contrast", seed)
    assert (r.sampler.minSamples, r.sampler.maxSamples) == (mins, maxs)
    return r


def _set(xy):
    return set(map(tuple, np.asarray(xy).reshape(-1, 2).tolist()))


def _case(ob, prims, r, mins, maxs, scene=None, exact=True):
    """One adaptive render against the oracle's composition.  Returns (scene, out, want)."""
    want = ar.oracle_adaptive(ob, ob.OracleScene(prims), r, mins, maxs)  # (asserts 0 < flagged < all)
    nfl, npix = len(want["flagged"]), len(want["pixels"])
    scene = scene or scenes.make_scene(prims)
    out = r.render(scene)
    got = r.supersampled_pixels(scene)
    print("adaptive (%d, %d): %d of %d pixels flagged on the oracle (%d black), %d on the device" % (mins, maxs, nfl, npix, int(want["black"].sum()), len(got)))
    assert len(got) == nfl and len(_set(got)) == len(got)
    assert _set(got) == want["flagged"]
    if exact:
        assert np.array_equal(out.film, want["film"])
        assert np.array_equal(out.rgb, want["rgb"])
    assert np.isfinite(out.film).all() and out.film[..., 3].sum() > 0
    st = r.last_stats
    assert st["camera_samples"] == mins * npix + maxs * nfl
    f = r.camera.film
    inside = lambda xy: sum(1 for x, y in xy if f.left <= x < f.left + f.width and f.top <= y < f.top + f.height)
    fl_in, all_in = inside(want["flagged"]), inside(_set(want["pixels"]))
    assert st["film_samples"] == mins * (all_in - fl_in) + maxs * fl_in
    return scene, out, want


def _c1(mins, maxs, integ=None, **kw):
    prims, mk = scenes.config("C1", xres=32, yres=24, spp=4, **kw)
    r = _adaptive(mk(), mins, maxs)
    if integ is not None:
        r.surfaceIntegrator = integ
    return prims, r


def _c2small(mins, maxs, **kw):
    prims, mk = scenes.config("C2", xres=16, yres=16, spp=4, blob=(32, 16), **kw)  # (tests/golden/make_golden.py's c2small), maxdepth 5
    return prims, _adaptive(mk(), mins, maxs)


# ---- 1. films ----
@pytest.mark.parametrize("mins,maxs", [(2, 4), (4, 32), (64, 256)])
def test_c1_direct_lighting(ob, gpu, mins, maxs):
    """(64, 256): the tiled shapes of k_adaptive_decide and k_film (16 pixels, 64 samples of each per pass; pass 2 walks four passes)."""
    prims, r = _c1(mins, maxs)
    scene, out, want = _case(ob, prims, r, mins, maxs)
    if (mins, maxs) == (4, 32):
        assert len(want["flagged"]) == 35 and int(want["black"].sum()) == 700
    if (mins, maxs) == (2, 4):
        assert len(want["flagged"]) == 25 and int(want["black"].sum()) == 702


def test_adaptive_film_is_neither_plain_film_and_equals_the_composition(ob, gpu):
    """Fails where the mode does not exist: the adaptive film differs from the plain minsamples and maxsamples films of the scene."""
    prims, r = _c1(4, 32)
    scene, out, want = _case(ob, prims, r, 4, 32)
    films = {}
    for spp in (4, 32):
        r.sampler = core.LowDiscrepancySampler(r.camera, spp, 5489)
        films[spp] = r.render(scene).film
        assert len(r.supersampled_pixels(scene)) == 0  # (the list is the LAST render's: another sampler leaves none)
    assert not np.array_equal(out.film, films[4]) and not np.array_equal(out.film, films[32])
    w = out.film[..., 3]
    assert np.array_equal(out.film[w == 4.0], films[4][w == 4.0]) and np.array_equal(out.film[w == 32.0], films[32][w == 32.0])
    assert set(np.unique(w).tolist()) == {4.0, 32.0}


def test_c1_path(ob, gpu):
    prims, r = _c1(4, 32, core.PathIntegrator(3))
    scene, out, want = _case(ob, prims, r, 4, 32)
    assert len(want["flagged"]) == 35


def test_small_c2_path(ob, gpu):
    prims, r = _c2small(4, 16)
    scene, out, want = _case(ob, prims, r, 4, 16)
    assert len(want["flagged"]) == 198 and len(want["pixels"]) == 289


def test_c1_path_at_64_with_lazy_generation(ob, gpu):
    """Path integrator from 64 samples on: both passes generate their sample blocks lazily, pass 2 at 512 spp with u16 indices."""
    prims, r = _c1(64, 512, core.PathIntegrator(3))
    scene, out, want = _case(ob, prims, r, 64, 512)
    assert scene._device().last_render_info()["lazy_gen"] == 1


# ---- 2. layouts, batches, shards ----
@pytest.mark.parametrize("layout", [64, 4])
def test_both_state_layouts(ob, gpu, layout):
    prims, r = _c2small(4, 16)
    scene = scenes.make_scene(prims)
    scene._device().state_layout(layout)
    _case(ob, prims, r, 4, 16, scene=scene)
    assert scene._device().last_render_info()["state_layout"] == layout


def test_several_first_pass_batches_and_the_pilot(ob, gpu):
    """BATCH_BITS = 16: 2^16 slots per batch at most.  C1 at 48 x 40 and (64, 256): 2009 pixels are 128576 first-pass slots (77 flagged
    and 1709 black on the oracle); the path integrator, so that a forced pilot has calibration batches to run."""
    prims, mk = scenes.config("C1", xres=48, yres=40, spp=4)
    r = _adaptive(mk(), 64, 256)
    r.surfaceIntegrator = core.PathIntegrator(3)
    lib = _abi.lib()
    one_scene, one, want = _case(ob, prims, r, 64, 256)
    try:
        _abi.check(lib.dr_set_option(b"BATCH_BITS", b"16"))
        scene = scenes.make_scene(prims)
        out = r.render(scene)
        got = r.supersampled_pixels(scene)
        batches = r.last_stats["batches"]
        _abi.check(lib.dr_set_option(b"PILOT", b"force"))
        scene_p = scenes.make_scene(prims)
        piloted = r.render(scene_p)
        got_p = r.supersampled_pixels(scene_p)
        pilot_batches = scene_p._device().last_render_info()["pilot_batches"]
    finally:
        lib.dr_set_option(b"BATCH_BITS", None)
        lib.dr_set_option(b"PILOT", None)
    nfl = len(want["flagged"])
    assert batches >= 2 + (nfl * 256 + 65535) // 65536 and batches > one_scene._device().last_render_info()["batches"]
    assert _set(got) == want["flagged"] and np.array_equal(out.film, want["film"]) and np.array_equal(out.rgb, want["rgb"])
    # calibration batches are part of pass 1: their pixels are decided like every other batch's
    assert pilot_batches >= 1
    assert _set(got_p) == want["flagged"] and np.array_equal(piloted.film, want["film"])


def test_two_tile_shares_sum_to_the_unsplit_film(ob, gpu):
    prims, mk = scenes.config("C1", xres=32, yres=24, spp=4)
    r = _adaptive(mk(), 4, 32)
    scene, one, want = _case(ob, prims, r, 4, 32)
    total, flagged = np.zeros_like(one.film), set()
    osc = ob.OracleScene(prims)
    for k in range(2):
        rk = _adaptive(scenes.config("C1", xres=32, yres=24, spp=4, tileRank=k, tileCount=2, tileSize=8)[1](), 4, 32)
        share = ar.oracle_adaptive(ob, osc, rk, 4, 32, pixels=rk.pixels())
        out = rk.render(scene)
        got = _set(rk.supersampled_pixels(scene))
        assert got == share["flagged"] and not (got & flagged)
        assert np.array_equal(out.film, share["film"])
        flagged |= got
        total += out.film
    assert flagged == want["flagged"]
    assert np.array_equal(total, one.film)


# ---- 3. a wide filter ----
def test_gaussian_filter(ob, gpu):
    """A retired pixel's first-pass samples must not splat into its neighbours either.  Own-pixel contributions are added in sample
    order, the others atomically: the tolerance of tests/test_gpu_filters.py."""
    prims = scenes.cornell_c1_prims()
    film = core.ImageFilm(32, 24, core.GaussianFilter(2.0, 2.0, 2.0))
    cam = core.PerspectiveCamera.lookAt((0, 0, -35), (0, 0, 0), (0, 1, 0), 35.0, film)
    r = core.SamplerRenderer(core.AdaptiveSampler(cam, 4, 32), cam, core.DirectLightingIntegrator(0, 5), core.EmissionIntegrator())
    scene, out, want = _case(ob, prims, r, 4, 32, exact=False)
    assert np.allclose(out.film, want["film"], rtol=2e-5, atol=2e-6)
    # ... and it would show: with the flagged pixels' first-pass samples left in, the film is further away than that
    lo = ob.render_desc(r, sampler_mode=1)
    lo.spp = 4
    leaked = ob.OracleScene(prims).render(lo)["film"] + want["high"]
    assert not np.allclose(leaked, want["film"], rtol=2e-5, atol=2e-6)


# ---- 4. the vectors, refusals ----
def test_generate_samples_dumps_the_min_pass(gpu):
    prims, r = _c2small(4, 16)
    scene = scenes.make_scene(prims)
    pixels = np.array([(0, 0), (3, 9), (16, 16)], np.int32)
    got = r.generate_samples(scene, pixels)
    r.sampler = core.LowDiscrepancySampler(r.camera, 4, 5489)
    assert got.shape == (12, 37) and np.array_equal(got.view(np.uint32), r.generate_samples(scene, pixels).view(np.uint32))


def test_bad_counts_are_refused_by_name_and_leave_the_scene_usable(gpu):
    lib = _abi.lib()
    prims, r = _c2small(4, 16)
    scene = scenes.make_scene(prims)
    film = np.zeros((16, 16, 4), np.float32)

    def refused(mins, maxs):
        d, keep = r.describe()
        d.strat_xsamples, d.spp = mins, maxs
        rc = lib.dr_render(scene._device().handle, C.byref(d), film.ctypes.data, None)
        assert rc in (-1, -4), rc  # DR_ERR_INVALID / DR_ERR_UNSUPPORTED
        msg = lib.dr_last_error().decode()
        assert "adaptive sampler" in msg and "minSamples" in msg and "maxSamples" in msg, msg

    for mins, maxs in [(1, 8), (0, 8), (3, 8), (4, 24), (8, 8), (16, 8), (4, 8192), (-4, 8)]:
        refused(mins, maxs)
    assert not film.any()
    n = C.c_uint64(99)
    _abi.check(lib.dr_scene_get_adaptive_pixels(scene._device().handle, None, 0, C.byref(n)))
    assert n.value == 0
    # the scene still renders: the LD golden of this very scene
    g = np.load(os.path.join(GOLDEN, "c2small_path_counter.npz"))
    r.sampler = core.LowDiscrepancySampler(r.camera, 8, 5489)
    out = r.render(scene)
    assert np.array_equal(out.film, g["film"]) and np.array_equal(out.rgb, g["rgb"])
    # a buffer smaller than the list is refused, the count is still written
    _adaptive(r, 4, 16).render(scene)
    h = scene._device().handle
    _abi.check(lib.dr_scene_get_adaptive_pixels(h, None, 0, C.byref(n)))
    assert n.value > 1
    small = np.zeros((1, 2), np.int32)
    m = C.c_uint64(0)
    assert lib.dr_scene_get_adaptive_pixels(h, small.ctypes.data, 1, C.byref(m)) == -1 and m.value == n.value
