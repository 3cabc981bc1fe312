"""The random sampler off the GPU: the host class (core.RandomSampler: descriptor, limits, the reference's serial stream), the test side's
restatement (tests/random_restatement.py), the plugin registry and the ABI constant."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, scenes

import random_restatement as rr


def _c1(spp, seed=5489, xres=16, yres=12, **kw):
    prims, mk = scenes.config("C1", xres=xres, yres=yres, spp=4, **kw)
    r = mk()
    r.sampler = core.RandomSampler(r.camera, spp, seed)
    return prims, r


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_sampler_builds_its_descriptor():
    prims, r = _c1(8, seed=9)
    d, _ = r.describe()
    assert (d.sampler_mode, d.spp, d.seed) == (_abi.DR_SAMPLER_RANDOM, 8, 9)
    s = r.sampler
    assert s.roundSize(3) == 3 and s.maximumSampleCount() == 8 and s.generatedSamplesPerPixel == 8
    assert core.RandomSampler(r.camera).samplesPerPixel == 10  # RandomSampler.Create's default (random_sampler.dart:96)
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    c = int(re.search(r"#define DR_SAMPLER_RANDOM (\d+)", header).group(1))
    assert c == _abi.DR_SAMPLER_RANDOM == 6 == int(re.search(r"const int DR_SAMPLER_RANDOM = (\d+);", dart).group(1))
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", header).group(1)) == _abi.DR_ABI_VERSION == 9  # additive: no struct changed


@pytest.mark.parametrize("spp", [3, 8192, 10])
def test_the_limits_are_refused_with_their_names(spp):
    prims, r = _c1(spp)
    with pytest.raises(ValueError, match=r"RandomSampler: pixelsamples must be a power of two, at most 4096"):
        r.describe()
    with pytest.raises(ValueError, match="positive"):
        core.RandomSampler(r.camera, 0)


def test_serial_samples_equal_a_serial_restatement_of_get_more_samples():
    """3 x 2 sampler window (a 2 x 1 film under the box filter), spp 4, DirectLighting: ONE RNG(taskNum) through every pixel."""
    prims, r = _c1(4, xres=2, yres=1)
    scene = scenes.make_scene(prims)
    e = rr.sample_extent(r.camera.film)
    assert (e[1] - e[0], e[3] - e[2]) == (3, 2)
    n1D, n2D = rr.slot_counts(0, [L.nSamples for L in scene.lights])
    assert (n1D, n2D) == tuple(r.sampler.slot_counts(r, scene))
    window = [(x, y) for y in range(e[2], e[3]) for x in range(e[0], e[1])]
    xy, want = rr.serial_vectors(window, 4, n1D, n2D, rr.RNG(0))
    assert len(xy) == 6 * 4 and want.shape == (6 * 4 * 4, 5 + sum(n1D) + 2 * sum(n2D))  # as written: four walks of the six pixels
    # the first walk is what the device traces, and the default
    hb = r.sampler.serial_samples(r, scene)
    assert isinstance(hb, core.HostBufferSampler) and hb.samplesPerPixel == 4
    assert np.array_equal(hb.pixel_xy, np.array(window, np.int32)) and np.array_equal(hb.pixel_xy, xy[:6])
    assert np.array_equal(_bits(hb.sample_vec), _bits(want[:24]))
    # all four walks: the same stream, continued
    hb4 = r.sampler.serial_samples(r, scene, passes=4)
    assert np.array_equal(hb4.pixel_xy, xy) and np.array_equal(_bits(hb4.sample_vec), _bits(want))
    # every value is a draw of its own: 24 vectors of nf distinct numbers in [0, 1), none repeated
    assert (want >= 0).all() and (want < 1).all() and len(np.unique(want[:24])) == want[:24].size
    # another task, another stream
    r.taskNum, r.taskCount = 1, 2
    assert not np.array_equal(r.sampler.serial_samples(r, scene).sample_vec[:4], hb.sample_vec[:4])
    # a path that draws inside Li cannot be serialised by the host alone
    r.surfaceIntegrator = core.PathIntegrator(5)
    with pytest.raises(ValueError, match="li_draws"):
        r.sampler.serial_samples(r, scene)


def test_the_restatement_draws_in_the_reference_order():
    """One sample is 5 + sum(n1D) + 2 sum(n2D) consecutive nextDouble() of its stream, stored in field order; the image sample is f32(u)."""
    n1D, n2D = [2, 1], [1, 2]
    key = rr.counter_key(77, 41, 3, rr.STREAM_KIND)
    vec, (ix, iy) = rr.draw_sample(5, 3, n1D, n2D, rr.RNG(key))
    g = rr.RNG(key)
    flat = np.array([g.randomFloat() for _ in range(5 + 3 + 6)])
    assert np.array_equal(vec, flat.astype(np.float32))
    assert (ix, iy) == (flat[0] + 5, flat[1] + 3)
    assert abs(float(vec[0]) - flat[0]) <= 2.0 ** -25  # the stated departure: the image fraction rounded to f32 once
    # the restatement's generator is the product's (both restate dart:math Random), key for key
    p = core.DartRandom(key)
    assert [p.randomFloat() for _ in range(14)] == list(flat)
    # keyed: (pixelIndex, i) decide the stream -- not the pixel list, not the order
    ext = (0, 17, 0, 13)
    a = rr.keyed_vectors(5489, ext, [(3, 2), (9, 9)], 4, n1D, n2D)
    b = rr.keyed_vectors(5489, ext, [(9, 9)], 4, n1D, n2D)
    assert np.array_equal(a[4:], b) and not np.array_equal(a[:4], b)
    assert not np.array_equal(rr.keyed_vectors(5490, ext, [(9, 9)], 4, n1D, n2D), b)


def test_the_plugin_registry_knows_the_name():
    assert core.Plugin.get("sampler", "random") is core.RandomSampler
    assert core.Plugin.get("pixelSampler", "random") is not None  # (Pixels "random" is another plugin and keeps its name)
    assert core.RandomSampler.__name__ == "RandomSampler"
