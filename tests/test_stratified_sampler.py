"""The stratified sampler off the GPU: the test side's restatement (tests/stratified_restatement.py), the host mirror
(core.StratifiedSampler: keyed and serial modes), the oracle composition the GPU tests compare films with, the PBRT
front end and the ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, pbrt, scenes

import stratified_restatement as sr


def _strata(v, n):
    return np.floor(np.asarray(v, np.float64) * n).astype(int)


def _c1(xs, ys, jitter=True, seed=5489, xres=32, yres=24, **kw):
    prims, mk = scenes.config("C1", xres=xres, yres=yres, spp=xs * ys, **kw)
    r = mk()
    r.sampler = core.StratifiedSampler(r.camera, xs, ys, jitter, seed)
    return prims, r


# ---- 1. the restatement's keyed vectors ----
@pytest.mark.parametrize("xs,ys", [(2, 2), (4, 4), (2, 8)])
def test_keyed_vectors_hit_every_stratum_once(xs, ys):
    prims, r = _c1(xs, ys)
    film, spp = r.camera.film, xs * ys
    pixels = [(0, 0), (5, 3), (31, 23), (32, 24)]
    vec, xy = sr.keyed_vectors(film, pixels, xs, ys, True, 77, [4, 1], [1, 4])
    assert vec.shape == (len(pixels) * spp, 5 + 5 + 10) and vec.dtype == np.float32
    assert (vec >= 0).all() and (vec[:, 2:] < 1).all() and (vec[:, :2] <= 1).all()
    for k, (px, py) in enumerate(pixels):
        v = vec[k * spp:(k + 1) * spp]
        # image: row-major strata (never shuffled); the stored fraction + the pixel is the reference's imageX / imageY
        assert np.array_equal(v[:, :2].astype(np.float64) + (px, py), xy[k * spp:(k + 1) * spp])
        cell = np.minimum(_strata(v[:, 0], xs), xs - 1) + xs * np.minimum(_strata(v[:, 1], ys), ys - 1)
        assert np.array_equal(cell, np.arange(spp)) or sorted(cell) == list(range(spp))
        lens = _strata(v[:, 2], xs) + xs * _strata(v[:, 3], ys)
        assert sorted(lens) == list(range(spp))
        assert sorted(_strata(v[:, 4], spp)) == list(range(spp))
        for i in range(spp):  # LatinHypercube of the slot with four entries: 1-D slot 0, 2-D slot 1 (both dimensions)
            assert sorted(_strata(v[i, 5:9], 4)) == [0, 1, 2, 3]
            assert sorted(_strata(v[i, 12:20:2], 4)) == [0, 1, 2, 3] and sorted(_strata(v[i, 13:20:2], 4)) == [0, 1, 2, 3]
    # another seed, other numbers; the same seed, the same
    assert not np.array_equal(vec, sr.keyed_vectors(film, pixels, xs, ys, True, 78, [4, 1], [1, 4])[0])
    assert np.array_equal(vec, sr.keyed_vectors(film, pixels, xs, ys, True, 77, [4, 1], [1, 4])[0])


def test_without_jitter_the_image_samples_are_the_stratum_centres():
    prims, r = _c1(4, 2, jitter=False)
    vec, xy = sr.keyed_vectors(r.camera.film, [(3, 2)], 4, 2, False, 1, [1], [1])
    want = np.array([[(x + 0.5) / 4, (y + 0.5) / 2] for y in range(2) for x in range(4)], np.float32)
    assert np.array_equal(vec[:, :2], want)
    assert sorted(vec[:, 4]) == [np.float32((i + 0.5) / 8) for i in range(8)]          # time: centres, shuffled
    assert sorted(map(tuple, vec[:, 2:4])) == sorted(map(tuple, want))                   # lens: centres, shuffled
    assert len(set(vec[:, 5])) == 8                                                       # the LatinHypercube draws stay random


def test_counter_key_equals_the_oracles(ob):
    for args in [(5489, 0, 0, 3), (77, 1234, 15, 4), (2 ** 40 + 3, 2 ** 33, 4095, 2)]:
        assert sr.counter_key(*args) == ob.lib().orc_counter_key(*args)


# ---- 2. serial mode: the draws, and keyed == serial in everything but the source of the numbers ----
class _Counting:
    """Counting wrapper of an RNG: calls, and the generator steps they took."""

    def __init__(self, rng):
        self.rng, self.floats, self.uints = rng, 0, 0

    def randomFloat(self):
        self.floats += 1
        return self.rng.randomFloat()

    def randomUint(self):
        self.uints += 1
        return self.rng.randomUint()


class _Fake:
    """A deterministic stand-in: the k-th call returns a value that depends on k alone."""

    def __init__(self):
        self.k = 0

    def randomFloat(self):
        self.k += 1
        return (self.k * 0.6180339887498949) % 1.0

    def randomUint(self):
        self.k += 1
        return (self.k * 2654435761) & 0xffffffff


class _StepCounting(core.DartRandom):
    """The product's generator with its calls and its generator steps counted."""

    def __init__(self, seed):
        self.steps = -4  # (the four warm-up steps of the constructor)
        self.floats = self.uints = 0
        core.DartRandom.__init__(self, seed)

    def _step(self):
        self.steps += 1
        core.DartRandom._step(self)

    def randomFloat(self):
        self.floats += 1
        return core.DartRandom.randomFloat(self)

    def randomUint(self):
        self.uints += 1
        return core.DartRandom.randomUint(self)


@pytest.mark.parametrize("xs,ys,jitter", [(2, 2, True), (4, 2, True), (2, 2, False)])
def test_serial_mode_consumes_the_draws_the_reference_does(xs, ys, jitter):
    """core.StratifiedSampler.pixel_samples on ONE generator (the serial mode): per pixel 5 * spp floats (none without jitter) and
    2 * spp uints, per sample sum(n1D) + 2 sum(n2D) floats and as many uints (stratified_sampler.dart:85-120, montecarlo.dart:270-325)."""
    prims, r = _c1(xs, ys, jitter)
    spp, n1D, n2D, task = xs * ys, [2, 2, 1, 1], [2, 2], 3
    c = _StepCounting(task)
    r.sampler.pixel_samples(7, 9, n1D, n2D, c, lambda i: c)
    per_sample = sum(n1D) + 2 * sum(n2D)
    assert c.floats == (5 * spp if jitter else 0) + spp * per_sample
    assert c.uints == 2 * spp + spp * per_sample
    assert c.steps >= 2 * c.floats + c.uints  # (a randomUint steps again after the one rejected value)
    # the state after the pixel: a DartRandom(taskNum) advanced by the counted number of steps
    twin = core.DartRandom(task)
    for _ in range(c.steps):
        twin._step()
    assert (twin.lo, twin.hi) == (c.lo, c.hi)
    # ... which the restatement reaches from the same seed, too
    ref = sr.RNG(task)
    sr.get_more_samples(7, 9, xs, ys, jitter, n1D, n2D, ref, lambda i: ref)
    assert (ref.random.lo, ref.random.hi) == (c.lo, c.hi)


def test_core_serial_samples_walks_one_rng_through_the_task():
    prims, r = _c1(2, 2, xres=8, yres=6)
    scene = scenes.make_scene(prims)
    hb = r.sampler.serial_samples(r, scene)
    assert isinstance(hb, core.HostBufferSampler) and hb.samplesPerPixel == 4
    n1D, n2D = sr.slot_counts(0, [L.nSamples for L in scene.lights])
    want, _ = sr.serial_vectors(hb.pixel_xy, 2, 2, True, n1D, n2D, sr.RNG(0))
    assert len(hb.pixel_xy) == 9 * 7 and np.array_equal(hb.pixel_xy[:10, 0], np.r_[np.arange(9), 0])
    assert np.array_equal(hb.sample_vec.view(np.uint32), want.view(np.uint32))
    # the state it leaves: 9 * 7 pixels of draws
    c = _Counting(sr.RNG(0))
    sr.serial_vectors(hb.pixel_xy, 2, 2, True, n1D, n2D, c)
    per = sum(n1D) + 2 * sum(n2D)
    assert c.floats == 63 * (20 + 4 * per) and c.uints == 63 * (8 + 4 * per)
    # a path that draws inside Li cannot be serialised by the host alone
    r.surfaceIntegrator = core.PathIntegrator(5)
    with pytest.raises(ValueError, match="li_draws"):
        r.sampler.serial_samples(r, scene)


@pytest.mark.parametrize("jitter", [True, False])
def test_keyed_and_serial_modes_agree_on_the_same_numbers(jitter):
    """core's host mirror against the restatement, both fed the same fake generator (where the numbers come from is all that tells the
    keyed mode from the serial one); and the two agree on the slots the integrators request."""
    prims, r = _c1(4, 2, jitter)
    scene = scenes.make_scene(prims)
    n1D, n2D = [1, 4, 1], [4, 1]
    fa, fb = _Fake(), _Fake()
    a = r.sampler.pixel_samples(11, 5, n1D, n2D, fa, lambda i: fa)
    b, _ = sr.get_more_samples(11, 5, 4, 2, jitter, n1D, n2D, fb, lambda i: fb)
    assert fa.k == fb.k and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    k1, k2 = sr.slot_counts(0, [L.nSamples for L in scene.lights])
    assert (k1, k2) == tuple(r.sampler.slot_counts(r, scene))


# ---- 3. the oracle composition the GPU tests rely on ----
def oracle_film(ob, osc, r, pixels, xs, ys, jitter, seed, light_nsamples):
    """Film and rgb of a stratified render as the frozen oracle prices the restated vectors: orc_li_samples (tail = the head of
    every sample's kind-2 stream) + orc_film_accumulate, samples in trace order.  Returns (film, rgb, vectors, imageXY)."""
    film, spp = r.camera.film, xs * ys
    kind, depth = r.surfaceIntegrator.kind, r.surfaceIntegrator.maxDepth
    n1D, n2D = sr.slot_counts(kind, light_nsamples)
    vec, xy = sr.keyed_vectors(film, pixels, xs, ys, jitter, seed, n1D, n2D)
    mt = sr.need_tail(kind, depth, len(light_nsamples))
    tail = sr.li_stream_tail(seed, film, pixels, spp, mt) if mt else None
    rd = ob.render_desc(r, sampler_mode=0)
    Ls = osc.li_samples(rd, np.repeat(np.asarray(pixels, np.int32).reshape(-1, 2), spp, axis=0), vec, tail)
    out_film = np.zeros((film.height, film.width, 4), np.float32)
    out_rgb = np.zeros((film.height, film.width, 3), np.float32)
    xy = np.ascontiguousarray(xy, np.float64)
    assert ob.lib().orc_film_accumulate(C.byref(rd), len(vec), xy.ctypes.data, Ls.ctypes.data, out_film.ctypes.data, out_rgb.ctypes.data) == 0
    return out_film, out_rgb, vec, xy


def window_pixels(r):
    e = sr.sample_extent(r.camera.film)
    x0, x1, y0, y1 = core.GetSubWindow(e[1] - e[0], e[3] - e[2], r.taskNum, max(1, r.taskCount))
    return np.array([(x, y) for y in range(y0, y1) for x in range(x0, x1)], np.int32)


@pytest.mark.parametrize("xs,ys", [(2, 2), (4, 4)])
def test_oracle_composition_of_the_keyed_vectors(ob, xs, ys):
    prims, r = _c1(xs, ys, xres=64, yres=64)  # scenes.config("C1") as it stands: 64 x 64
    film = r.camera.film
    osc = ob.OracleScene(prims)
    px = window_pixels(r)
    assert len(px) == 65 * 65
    out_film, out_rgb, vec, xy = oracle_film(ob, osc, r, px, xs, ys, True, 5489, [1])
    assert np.isfinite(out_film).all() and np.isfinite(out_rgb).all()
    # box filter (image_film.dart:99-140): a sample lands in the pixels [ceil(X - 1), floor(X)] x [ceil(Y - 1), floor(Y)] of the window
    cx = np.minimum(np.floor(xy[:, 0]), film.left + film.width - 1) - np.maximum(np.ceil(xy[:, 0] - 1.0), film.left) + 1
    cy = np.minimum(np.floor(xy[:, 1]), film.top + film.height - 1) - np.maximum(np.ceil(xy[:, 1] - 1.0), film.top) + 1
    want = float((np.maximum(cx, 0) * np.maximum(cy, 0)).sum())
    assert out_film[..., 3].sum() == want and want >= 64 * 64 * xs * ys
    # against the oracle's LD render of the same scene at the same spp.  Measured over LD seeds 1..8 (C1, 64 x 64, this oracle): the mean
    # of the rgb image is 0.8404 with sigma = 7.4e-3 at 2 x 2 and 0.8395 with sigma = 1.3e-3 at 4 x 4; the bound is 4 sigma of that
    # spread.  The stratified film (seed 5489, the sampler's default) sits 2.5 and 1.2 of those sigma away.  (Its own spread over seeds
    # is about twice the LD sampler's -- random LatinHypercube light samples against (0,2)-sequences; both are unbiased.)
    ld = r.__class__(core.LowDiscrepancySampler(r.camera, xs * ys, 1), r.camera, r.surfaceIntegrator, r.volumeIntegrator)
    means = []
    for seed in range(1, 9):
        ld.sampler.seed = seed
        means.append(float(osc.render(ob.render_desc(ld, sampler_mode=1))["rgb"].mean()))
    sigma = float(np.std(means, ddof=1))
    print("LD mean %.6g sigma %.3g; stratified mean %.6g" % (np.mean(means), sigma, out_rgb.mean()))
    assert abs(float(out_rgb.mean()) - float(np.mean(means))) <= 4 * sigma


# ---- 4. loader ----
_PBRT = '''
Film "image" "integer xresolution" [16] "integer yresolution" [12]
SurfaceIntegrator "path" "integer maxdepth" [3]
%s
LookAt 0 0 -35  0 0 0  0 1 0
Camera "perspective" "float fov" [35]
WorldBegin
AttributeBegin
AreaLightSource "diffuse" "color L" [10 10 10]
Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-1 9 -1  1 9 -1  0 9 1]
AttributeEnd
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-10 -10 -10  10 -10 -10  10 -10 10  -10 -10 10]
WorldEnd
'''


def test_loader_builds_the_stratified_sampler(tmp_path):
    def renderer(line):
        f = tmp_path / "s.pbrt"
        f.write_text(_PBRT % line)
        return pbrt.load(str(f)).rendererObject
    s = renderer('Sampler "stratified" "integer xsamples" [4] "integer ysamples" [2] "bool jitter" ["false"]').sampler
    assert isinstance(s, core.StratifiedSampler)
    assert (s.xPixelSamples, s.yPixelSamples, s.jitterSamples, s.samplesPerPixel) == (4, 2, False, 8)
    assert s.roundSize(3) == 3 and s.maximumSampleCount() == 8
    s = renderer('Sampler "stratified" "integer pixelsamples" [4]').sampler
    assert (s.xPixelSamples, s.yPixelSamples, s.jitterSamples) == (4, 4, True)
    s = renderer('Sampler "stratified"').sampler
    assert (s.xPixelSamples, s.yPixelSamples) == (2, 2)
    with pytest.raises(pbrt.UnsupportedFeature, match="power of two"):
        renderer('Sampler "stratified" "integer pixelsamples" [3]')
    with pytest.raises(pbrt.UnsupportedFeature, match="Sampler"):
        renderer('Sampler "halton"')
    assert isinstance(renderer('Sampler "lowdiscrepancy" "integer pixelsamples" [4]').sampler, core.LowDiscrepancySampler)


# ---- 5. ABI ----
def test_abi_of_the_stratified_mode():
    assert _abi.DrRenderDesc.strat_xsamples.offset == 1292 and C.sizeof(_abi.DrRenderDesc) == 1352
    assert _abi.DrRenderDesc.tile_size.offset == 1288 and _abi.DrRenderDesc.nsamples.offset == 1296
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    v = int(re.search(r"#define DR_ABI_VERSION (\d+)", header).group(1))
    assert v == _abi.DR_ABI_VERSION == int(re.search(r"static const int ABI_VERSION = (\d+);", dart).group(1)) and v >= 8
    for name in ("DR_SAMPLER_STRATIFIED", "DR_SAMPLER_STRATIFIED_NOJITTER"):
        c = int(re.search(r"#define %s (\d+)" % name, header).group(1))
        assert c == getattr(_abi, name) == int(re.search(r"const int %s = (\d+);" % name, dart).group(1))
    assert "OFF_DrRenderDesc_strat_xsamples = 1292" in dart and "dr_generate_samples" in _abi.EXPORTS
    prims, r = _c1(4, 2, jitter=False, seed=9)
    d, _ = r.describe()
    assert (d.sampler_mode, d.strat_xsamples, d.spp, d.seed) == (_abi.DR_SAMPLER_STRATIFIED_NOJITTER, 4, 8, 9)
    r.sampler.jitterSamples = True
    assert r.describe()[0].sampler_mode == _abi.DR_SAMPLER_STRATIFIED
    assert math.log2(d.spp) == 3
