"""The stratified device sampler (DR_SAMPLER_STRATIFIED / _NOJITTER) on the GPU, bit for bit against the frozen oracle:
the vectors (dr_generate_samples) against the Python restatement (tests/stratified_restatement.py), and the films
against the oracle's pricing of those restated vectors (orc_li_samples + orc_film_accumulate: oracle_film in
tests/test_stratified_sampler.py).  Every scene has the box filter, so films are compared with equality.  Nothing is
started after a failed render call: every call's return code raises."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from dartray_amd import _abi, core, scenes

import stratified_restatement as sr
from test_stratified_sampler import _c1, oracle_film, window_pixels

sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402

pytestmark = pytest.mark.gpu


def _strat(r, xs, ys, jitter=True, seed=5489):
    r.sampler = core.StratifiedSampler(r.camera, xs, ys, jitter, seed)
    return r


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 6. the vectors ----
@pytest.mark.parametrize("xs,ys,jitter,seed", [(2, 2, True, 5489), (4, 4, True, 5489), (8, 8, True, 77), (2, 8, True, 77),
                                                (2, 2, False, 77), (4, 4, False, 5489), (2, 8, False, 5489), (8, 8, False, 77)])
def test_generated_vectors_equal_the_restatement(gpu, xs, ys, jitter, seed):
    prims, r = _c1(xs, ys, jitter, seed)
    r.surfaceIntegrator = core.PathIntegrator(5)
    scene = scenes.make_scene(prims)
    pixels = np.array([(0, 0), (1, 0), (31, 23), (32, 24), (7, 11)] + [(x, 5) for x in range(8, 20)], np.int32)
    got = r.generate_samples(scene, pixels)
    n1D, n2D = sr.slot_counts(1, [1])
    want, _ = sr.keyed_vectors(r.camera.film, pixels, xs, ys, jitter, seed, n1D, n2D)
    assert got.shape == want.shape == (len(pixels) * xs * ys, 37)
    assert np.array_equal(_bits(got), _bits(want))


def test_generated_vectors_of_a_sub_window_are_keyed_by_the_full_extent(gpu):
    prims, mk = scenes.config("C1", xres=32, yres=24, spp=4, taskNum=2, taskCount=4)
    r = _strat(mk(), 2, 2)
    scene = scenes.make_scene(prims)
    pixels = r.pixels()
    assert len(pixels) < 33 * 25 and pixels.min(axis=0).max() > 0  # task 2 of 4: not the window's first pixel
    got = r.generate_samples(scene, pixels)
    n1D, n2D = sr.slot_counts(0, [L.nSamples for L in scene.lights])
    want, _ = sr.keyed_vectors(r.camera.film, pixels, 2, 2, True, 5489, n1D, n2D)
    assert np.array_equal(_bits(got), _bits(want))
    whole = _strat(scenes.config("C1", xres=32, yres=24, spp=4)[1](), 2, 2)
    assert np.array_equal(_bits(whole.generate_samples(scene, pixels)), _bits(got))


@pytest.mark.parametrize("spp", [4, 64])
def test_the_dump_reads_the_ld_sampler_as_a_render_does(ob, gpu, spp):
    """dr_generate_samples in DR_SAMPLER_COUNTER mode equals the oracle's LDPixelSampleCounter (both forms of the compact sampler)."""
    prims, mk = scenes.config("C2", xres=16, yres=16, spp=spp, blob=(32, 16))
    r = mk()
    scene = scenes.make_scene(prims)
    pixels = np.array([(0, 0), (3, 9), (16, 16)], np.int32)
    got = r.generate_samples(scene, pixels)
    n1D, n2D = np.ones(14, np.int32), np.ones(9, np.int32)
    for k, (px, py) in enumerate(pixels):
        want = np.zeros((spp, 37), np.float32)
        ob.lib().orc_ld_pixel_sample(1, r.sampler.seed, int(py) * 17 + int(px), spp, n1D.ctypes.data, 14, n2D.ctypes.data, 9, want.ctypes.data)
        assert np.array_equal(_bits(got[k * spp:(k + 1) * spp]), _bits(want)), k


# ---- 7. films ----
def _film_case(ob, prims, r, xs, ys, jitter=True, env=None):
    scene = scenes.make_scene(prims, env) if env is not None else scenes.make_scene(prims)
    out = r.render(scene)
    osc = ob.OracleScene(prims, env=env) if env is not None else ob.OracleScene(prims)
    film, rgb, _, _ = oracle_film(ob, osc, r, window_pixels(r), xs, ys, jitter, r.sampler.seed, [L.nSamples for L in scene.lights])
    assert np.array_equal(out.film, film)
    assert np.array_equal(out.rgb, rgb)
    assert out.film[..., 3].sum() > 0 and np.isfinite(out.film).all()
    return scene, out


@pytest.mark.parametrize("xs,ys,jitter", [(2, 2, True), (4, 4, True), (8, 8, True), (2, 2, False)])
def test_c1_film(ob, gpu, xs, ys, jitter):
    prims, r = _c1(xs, ys, jitter)
    _film_case(ob, prims, r, xs, ys, jitter)


def test_c1_path_film(ob, gpu):
    prims, r = _c1(2, 4)
    r.surfaceIntegrator = core.PathIntegrator(2)
    _film_case(ob, prims, r, 2, 4)


def test_small_c2_path_film_with_the_in_li_stream(ob, gpu):
    prims, mk = scenes.config("C2", xres=16, yres=16, spp=8, blob=(32, 16))  # (tests/golden/make_golden.py's c2small), maxdepth 5
    _film_case(ob, prims, _strat(mk(), 4, 2), 4, 2)


def test_direct_all_with_four_samples_per_light(ob, gpu):
    prims, mk = scenes.config("C1", xres=16, yres=16, spp=4)
    next(gp for gp in prims if gp.areaLight is not None).areaLight.nSamples = 4
    _film_case(ob, prims, _strat(mk(), 2, 2), 2, 2)


def test_direct_one_film(ob, gpu):
    prims, mk = mrf.dlone_case()
    _film_case(ob, prims, _strat(mk(), 2, 2), 2, 2)


def test_thin_lens_film(ob, gpu):
    prims, mk = mrf.lens_case()
    _film_case(ob, prims, _strat(mk(), 2, 2), 2, 2)


def test_environment_map_film(ob, gpu):
    prims, mk = mrf.env_case()
    r = _strat(mk(), 4, 2)
    _film_case(ob, prims, r, 4, 2, env=r.env)


# ---- 8. invariance ----
def test_shards_batches_and_the_pilot_leave_the_film_alone(gpu):
    prims, mk = scenes.config("C2", xres=48, yres=40, spp=64, blob=(32, 16))
    scene = scenes.make_scene(prims)
    one = _strat(mk(), 8, 8).render(scene)
    tiles = sum(_strat(scenes.config("C2", xres=48, yres=40, spp=64, blob=(32, 16), tileRank=k, tileCount=3, tileSize=8)[1](), 8, 8).render(scene).film
                for k in range(3))
    assert np.array_equal(tiles, one.film)
    tasks = sum(_strat(scenes.config("C2", xres=48, yres=40, spp=64, blob=(32, 16), taskNum=k, taskCount=4)[1](), 8, 8).render(scene).film
                for k in range(4))
    assert np.array_equal(tasks, one.film)
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(b"BATCH_BITS", b"16"))
        r = _strat(mk(), 8, 8)
        batched = r.render(scene)
        assert r.last_stats["batches"] > 1
        _abi.check(lib.dr_set_option(b"PILOT", b"force"))
        piloted = _strat(mk(), 8, 8).render(scenes.make_scene(prims))
    finally:
        lib.dr_set_option(b"BATCH_BITS", None)
        lib.dr_set_option(b"PILOT", None)
    assert np.array_equal(batched.film, one.film) and np.array_equal(batched.rgb, one.rgb)
    assert np.array_equal(piloted.film, one.film)


# ---- 9. the reference's serial stream through host buffers ----
def test_serial_stream_replay(ob, gpu):
    prims, r = _c1(2, 2)
    scene = scenes.make_scene(prims)
    hb = r.sampler.serial_samples(r, scene)
    n1D, n2D = sr.slot_counts(0, [1])
    vec, xy = sr.serial_vectors(hb.pixel_xy, 2, 2, True, n1D, n2D, sr.RNG(0))
    assert np.array_equal(_bits(hb.sample_vec), _bits(vec))
    r.sampler = hb
    out = r.render(scene)
    rd = ob.render_desc(r, sampler_mode=0)
    Ls = ob.OracleScene(prims).li_samples(rd, np.repeat(hb.pixel_xy, 4, axis=0), vec)
    film = np.zeros((24, 32, 4), np.float32)
    rgb = np.zeros((24, 32, 3), np.float32)
    xy = np.ascontiguousarray(xy)
    assert ob.lib().orc_film_accumulate(C.byref(rd), len(vec), xy.ctypes.data, Ls.ctypes.data, film.ctypes.data, rgb.ctypes.data) == 0
    assert np.array_equal(out.film, film) and np.array_equal(out.rgb, rgb)


# ---- 10. refusals ----
def test_limits_are_refused_by_name_and_leave_the_scene_usable(gpu):
    lib = _abi.lib()
    prims, mk = scenes.config("C2", xres=16, yres=16, spp=8, blob=(32, 16))
    scene = scenes.make_scene(prims)
    film = np.zeros((16, 16, 4), np.float32)

    def refused(r, needle, mutate=None):
        d, keep = r.describe()
        if mutate:
            mutate(d)
        rc = lib.dr_render(scene._device().handle, C.byref(d), film.ctypes.data, None)
        assert rc in (-1, -4), rc  # DR_ERR_INVALID / DR_ERR_UNSUPPORTED
        assert needle in lib.dr_last_error().decode(), lib.dr_last_error()

    refused(_strat(mk(), 3, 2), "power of two")
    refused(_strat(mk(), 2, 2), "strat_xsamples", lambda d: setattr(d, "strat_xsamples", 3))
    refused(_strat(mk(), 2, 2), "strat_xsamples", lambda d: setattr(d, "strat_xsamples", 0))
    # the scene still renders: the LD golden of this very scene
    g = np.load(os.path.join(GOLDEN, "c2small_path_counter.npz"))
    out = mk().render(scene)
    assert np.array_equal(out.film, g["film"]) and np.array_equal(out.rgb, g["rgb"])
    # a light with nsamples = 3 under DirectLighting "all": the scene's slot layout is the rounded one
    prims1, mk1 = scenes.config("C1", xres=16, yres=16, spp=4)
    next(gp for gp in prims1 if gp.areaLight is not None).areaLight.nSamples = 3
    scene = scenes.make_scene(prims1)
    refused(_strat(mk1(), 2, 2), "nsamples must be a power of two")
    assert np.isfinite(mk1().render(scene).film).all()  # the LD sampler rounds 3 up to 4 and renders


# ---- 11. the command line ----
def test_pbrt_command_line_renders_a_stratified_scene(gpu, tmp_path):
    from dartray_amd import pbrt
    text = open(os.path.join(ROOT, "examples", "cornell-specular.pbrt")).read()
    lines = text.splitlines()
    at = [i for i, l in enumerate(lines) if l.strip().startswith("Sampler")]
    assert len(at) == 1
    lines[at[0]] = 'Sampler "stratified" "integer xsamples" [4] "integer ysamples" [4]'
    scene_file = tmp_path / "cornell-stratified.pbrt"
    scene_file.write_text("\n".join(lines) + "\n")
    out_file = tmp_path / "out.npy"
    res = subprocess.run([sys.executable, "-m", "dartray_amd.pbrt", str(scene_file), "-o", str(out_file), "--xres", "32", "--yres", "32"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    api = pbrt.load(str(scene_file), overrides={"xresolution": 32, "yresolution": 32})
    s = api.rendererObject.sampler
    assert isinstance(s, core.StratifiedSampler) and (s.xPixelSamples, s.yPixelSamples) == (4, 4)
    direct = api.rendererObject.render(api.scene)
    assert np.array_equal(np.load(out_file), direct.rgb) and direct.rgb.max() > 0
