"""The Halton sampler off the GPU: the test side's restatement of DESIGN.md 2.9 (tests/halton_restatement.py), the host mirror
(core.HaltonSampler: descriptor and serial mode), the oracle composition the GPU tests compare films with, and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, scenes

import film_reference as fr
import halton_restatement as hr
import stratified_restatement as sr


def _c1(spp, seed=5489, xres=16, yres=12, depth=None, **kw):
    """C1 (DirectLighting "all"; depth: PathIntegrator(depth) instead) under a HaltonSampler of `spp` pixelsamples."""
    prims, mk = scenes.config("C1", xres=xres, yres=yres, spp=4, **kw)
    r = mk()
    r.sampler = core.HaltonSampler(r.camera, spp, seed)
    if depth is not None:
        r.surfaceIntegrator = core.PathIntegrator(depth)
    return prims, r


def oracle_radiances(ob, osc, r, s, nlights=1):
    """The frozen oracle's Li for the restated samples `s` (vectors + the head of every sample's kind-2 stream), before the guards."""
    need = sr.need_tail(r.surfaceIntegrator.kind, r.surfaceIntegrator.maxDepth, nlights)
    return osc.li_samples(ob.render_desc(r, sampler_mode=0), s.pixel_xy, s.vec, s.tail if need else None)


def restated(r, light_nsamples, first=0, count=None):
    """hr.keyed for the renderer's own window, sampler and integrator."""
    kind, depth = r.surfaceIntegrator.kind, r.surfaceIntegrator.maxDepth
    n1D, n2D = sr.slot_counts(kind, light_nsamples)
    win = hr.task_window(r.camera.film, r.taskNum, r.taskCount)
    return hr.keyed(win, r.sampler.samplesPerPixel, r.sampler.seed, n1D, n2D, sr.need_tail(kind, depth, len(light_nsamples)), first, count)


# ---- 1. RadicalInverse ----
def test_radical_inverse_hand_values():
    assert hr.RadicalInverse(0, 2) == 0.0
    assert hr.RadicalInverse(1, 2) == 0.5 and hr.RadicalInverse(3, 2) == 0.75 and hr.RadicalInverse(6, 2) == 0.375
    third = 1.0 / 3.0
    assert hr.RadicalInverse(5, 3) == 2 * third + 1 * (third * third)  # 5 = 12 in base 3 -> 0.21 = 7/9, as the f64 the loop gives
    assert abs(hr.RadicalInverse(5, 3) - 7.0 / 9.0) <= 2.0 ** -52
    assert hr.RadicalInverse(7, 7) == 1 * ((1.0 / 7.0) * (1.0 / 7.0))
    for n, b in [(1, 2), (3, 2), (5, 3), (1234567, 11), (2 ** 40 + 17, 5)]:
        assert core.RadicalInverse(n, b) == hr.RadicalInverse(n, b)


def test_multiply_and_truncate_is_the_integer_division_on_every_test_size():
    """n = (n * invBase).toInt() (montecarlo.dart:335) equals n // base for every n < 2^20 in the five bases the sampler uses, so the
    restatement, the device loop and an integer implementation walk the same digits at every size the tests reach."""
    n = np.arange(1 << 20, dtype=np.int64)
    for base in (2, 3, 5, 7, 11):
        stepped = (n.astype(np.float64) * (1.0 / base)).astype(np.int64)  # IEEE product, truncated: what Python's int(n * invBase) does
        assert np.array_equal(stepped, n // base), base
        for k in (1, 2, base, base * base - 1, 99991, (1 << 20) - 1):
            assert int(k * (1.0 / base)) == k // base and hr.RadicalInverse(k, base) == hr.radical_inverse_int(k, base)


# ---- 2. acceptance ----
def test_acceptance_on_a_9_by_6_window():
    win, spp = (0, 0, 9, 6), 3
    assert hr.wanted(win, spp) == 243  # delta = 9
    s = hr.keyed(win, spp, 5489, [1], [1])
    every = [hr.image_sample(win, k) for k in range(243)]
    inside = [k for k, (x, y) in enumerate(every) if not (x > 8 or y > 5)]
    assert list(s.k) == inside and all(a < b for a, b in zip(inside, inside[1:]))
    assert (s.imageXY[:, 0] <= 8).all() and (s.imageXY[:, 1] <= 5).all() and (s.imageXY >= 0).all()
    assert np.array_equal(s.pixel_xy, np.floor(np.array([every[k] for k in inside])).astype(np.int32))
    assert s.pixel_xy[:, 0].max() <= 8 and s.pixel_xy[:, 1].max() <= 5
    # a sanity bound on a deterministic count: the window's share of the delta x delta square, the inclusive right / bottom edges counted
    share = (8.0 / 9.0) * (5.0 / 9.0)
    assert abs(len(inside) / 243.0 - share) <= 0.1 * share
    assert len(inside) == 122
    # pixels receive different numbers of samples
    counts = np.bincount(s.pixel_xy[:, 1] * 9 + s.pixel_xy[:, 0], minlength=54)
    assert counts.min() < counts.max()


def test_a_sub_range_is_a_cut_of_the_sequence_and_lens_time_use_the_next_index():
    win = (0, 0, 9, 6)
    whole = hr.keyed(win, 3, 77, [2, 1], [1, 2], max_tail=4)
    part = hr.keyed(win, 3, 77, [2, 1], [1, 2], max_tail=4, first=100, count=90)
    keep = (whole.k >= 100) & (whole.k < 190)
    assert keep.sum() == len(part.k) > 0
    for a, b in zip(whole, part):
        assert np.array_equal(a[keep], b)
    for k, v in zip(whole.k, whole.vec):
        k = int(k)
        assert v[2] == np.float32(hr.RadicalInverse(k + 1, 5)) and v[3] == np.float32(hr.RadicalInverse(k + 1, 7))
        assert v[4] == np.float32(hr.RadicalInverse(k + 1, 11))
    assert np.array_equal(hr.li_tail(77, whole.k, 4), whole.tail) and whole.tail.min() >= 0 and 0 < whole.tail.max() < 1
    big = np.array([0, 1, 2 ** 33 + 5, 2 ** 52], np.uint64)
    assert [list(row) for row in hr.li_tail(5489, big, 3)] == [[r.randomFloat() for _ in range(3)] for r in (core.DartRandom(sr.counter_key(5489, int(k), 0, 2)) for k in big)]
    assert (whole.vec[:, :2] >= 0).all() and (whole.vec[:, :2] <= 1).all() and (whole.vec[:, 2:] < 1).all()
    # LatinHypercube of the slots with two entries: one value per half
    assert all(sorted(np.floor(v[5:7] * 2)) == [0, 1] for v in whole.vec)
    assert not np.array_equal(whole.vec[:, 5:], hr.keyed(win, 3, 78, [2, 1], [1, 2]).vec[:, 5:])
    assert np.array_equal(whole.vec[:, :5], hr.keyed(win, 3, 78, [2, 1], [1, 2]).vec[:, :5])  # the seed moves only the keyed streams


# ---- 3. the host mirror ----
def test_core_halton_sampler_and_its_serial_stream(ob):
    prims, r = _c1(3)
    scene = scenes.make_scene(prims)
    s = r.sampler
    assert s.samplesPerPixel == 3 and s.roundSize(3) == 3 and s.maximumSampleCount() == 1
    assert core.Plugin.get("sampler", "halton") is core.HaltonSampler
    with pytest.raises(ValueError, match="positive"):
        core.HaltonSampler(r.camera, 0)
    hb = s.serial_samples(r, scene)
    assert isinstance(hb, core.HostBufferSampler) and hb.samplesPerPixel == 1
    n1D, n2D = sr.slot_counts(0, [L.nSamples for L in scene.lights])
    assert (n1D, n2D) == tuple(s.slot_counts(r, scene))
    win = hr.task_window(r.camera.film)
    assert win == (0, 0, 17, 13) == core.HaltonSampler.window(r)
    want = hr.serial(win, 3, n1D, n2D, core.DartRandom(0))
    assert len(hb.pixel_xy) == len(hb.sample_vec) == len(want.k) > 0
    assert np.array_equal(hb.pixel_xy, want.pixel_xy)
    assert np.array_equal(hb.sample_vec.view(np.uint32), want.vec.view(np.uint32))
    # ... fed to the oracle through a host-buffer descriptor: the radiances of the restated vectors
    osc = ob.OracleScene(prims)
    r.sampler = hb
    got = osc.li_samples(ob.render_desc(r, sampler_mode=0), hb.pixel_xy, hb.sample_vec)
    r.sampler = s
    ref = osc.li_samples(ob.render_desc(r, sampler_mode=0), want.pixel_xy, want.vec)
    assert np.array_equal(got, ref) and np.isfinite(got).all() and got.max() > 0
    # a path that draws inside Li cannot be serialised by the host alone
    r.surfaceIntegrator = core.PathIntegrator(5)
    with pytest.raises(ValueError, match="li_draws"):
        s.serial_samples(r, scene)


# ---- 4. ABI ----
def test_abi_of_the_halton_mode():
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    v = int(re.search(r"#define DR_ABI_VERSION (\d+)", header).group(1))
    assert v == _abi.DR_ABI_VERSION == 9 == int(re.search(r"static const int ABI_VERSION = (\d+);", dart).group(1))
    c = int(re.search(r"#define DR_SAMPLER_HALTON (\d+)", header).group(1))
    assert c == _abi.DR_SAMPLER_HALTON == 5 == int(re.search(r"const int DR_SAMPLER_HALTON = (\d+);", dart).group(1))
    assert "dr_generate_halton_samples" in _abi.EXPORTS and re.search(r"\bdr_generate_halton_samples\s*\(", header)
    assert "lookupFunction<_HaltonSamplesC, _HaltonSamplesD>('dr_generate_halton_samples')" in dart
    assert C.sizeof(_abi.DrRenderDesc) == 1352  # nothing moved
    prims, r = _c1(3, seed=9, taskNum=1, taskCount=2)
    d, _ = r.describe()
    assert (d.sampler_mode, d.spp, d.seed, d.task_num, d.task_count, d.tile_count) == (5, 3, 9, 1, 2, 1)
    r.sampler = core.HaltonSampler(r.camera, 40)
    assert r.describe()[0].spp == 40  # not rounded to a power of two


# ---- 5. the oracle composition the GPU test relies on ----
def test_restated_film_through_the_oracle_is_finite_and_lit(ob):
    prims, r = _c1(3, depth=5)
    film = r.camera.film
    s = restated(r, [1])
    assert s.tail.shape[1] == sr.need_tail(1, 5, 1) == 32 and len(s.k) > 3 * 16 * 12 // 2
    Ls = oracle_radiances(ob, ob.OracleScene(prims), r, s)
    out_film, out_rgb = fr.oracle_film_of(ob, r, s.imageXY, Ls)
    assert np.isfinite(out_film).all() and np.isfinite(out_rgb).all() and out_rgb.max() > 0
    # 0.5 box filter: a sample reaches its anchor pixel where the film holds it (the window's last column and row are not on the film)
    on_film = (s.pixel_xy[:, 0] < film.width) & (s.pixel_xy[:, 1] < film.height) & (s.vec[:, 0] > 0) & (s.vec[:, 1] > 0) & (s.vec[:, 0] < 1) & (s.vec[:, 1] < 1)
    assert out_film[..., 3].sum() >= on_film.sum() > 0
    ref = fr.reference_from_samples(film, s.pixel_xy, 1, s.vec[:, 0], s.vec[:, 1], Ls, serial=False)
    assert np.all(np.abs(out_film.astype(np.float64) - ref.sum) <= fr.bound(ref.S, ref.n))
