"""The adaptive sampler off the GPU: the constructor's rules (core.AdaptiveSampler against the restatement of
samplers/adaptive_sampler.dart:40-91 in tests/adaptive_restatement.py), known answers of the restated decision, the
oracle composition the GPU tests compare films with, the PBRT front end, the descriptor and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, pbrt, scenes

import adaptive_restatement as ar


def _c1(mins, maxs, seed=5489, xres=32, yres=24, **kw):
    prims, mk = scenes.config("C1", xres=xres, yres=yres, spp=4, **kw)
    r = mk()
    r.sampler = core.AdaptiveSampler(r.camera, mins, maxs, "contrast", seed)
    return prims, r


# ---- 1. the constructor ----
# (mins, maxs) -> (samplesPerPixel, minSamples, maxSamples), worked out by hand from adaptive_sampler.dart:40-83
_TABLE = [((4, 32), (32, 4, 32)),      # the defaults
          ((32, 4), (32, 4, 32)),      # swapped
          ((3, 20), (32, 4, 32)),      # neither a power of two: both rounded up
          ((5, 9), (16, 8, 16)),
          ((1, 8), (8, 2, 8)),         # one initial sample: two
          ((1, 2), (2, 2, 4)),         # ... which then equals the maximum
          ((1, 1), None),              # see the test
          ((8, 8), (8, 8, 16)),        # equal: the maximum doubles
          ((6, 7), (8, 8, 16)),        # equal after rounding
          ((2, 2), (2, 2, 4)),
          ((64, 256), (256, 64, 256)),
          ((2048, 4096), (4096, 2048, 4096))]


def test_constructor_rules_on_a_table():
    cam = scenes.cornell_camera(8, 8)
    for (mins, maxs), want in _TABLE:
        if (mins, maxs) == (1, 1):
            # min 1 -> 2 (":73-77"), max stays 1: min != max, so nothing doubles -- the reference then holds min 2 > max 1.
            # The device refuses such a pair; the host class reports it rather than hand it on.
            assert ar.normalise(1, 1) == (1, 2, 1)
            with pytest.raises(ValueError, match="more maximum than minimum"):
                core.AdaptiveSampler(cam, 1, 1)
            continue
        assert ar.normalise(mins, maxs) == want, (mins, maxs)
        s = core.AdaptiveSampler(cam, mins, maxs)
        assert (s.samplesPerPixel, s.minSamples, s.maxSamples) == want, (mins, maxs)
        assert s.maximumSampleCount() == s.maxSamples
        assert 2 <= s.minSamples < s.maxSamples and s.minSamples & (s.minSamples - 1) == 0 and s.maxSamples & (s.maxSamples - 1) == 0
    s = core.AdaptiveSampler(cam)
    assert (s.minSamples, s.maxSamples, s.method, s.seed) == (4, 32, "contrast", 5489)
    assert [s.roundSize(n) for n in (1, 3, 4, 5, 33)] == [1, 4, 4, 8, 64]
    assert [ar.round_up_pow2(n) for n in (1, 3, 4, 5, 33)] == [core.RoundUpPow2(n) for n in (1, 3, 4, 5, 33)]
    assert core.Plugin.get("sampler", "adaptive") is core.AdaptiveSampler


def test_bad_counts_and_shapeid_are_refused_by_name():
    cam = scenes.cornell_camera(8, 8)
    with pytest.raises(ValueError, match="shapeid"):
        core.AdaptiveSampler(cam, 4, 32, "shapeid")
    with pytest.raises(ValueError, match="contrast"):
        core.AdaptiveSampler(cam, 4, 32, "variance")
    with pytest.raises(ValueError, match="4096"):
        core.AdaptiveSampler(cam, 4, 8192)
    with pytest.raises(ValueError, match="4096"):
        core.AdaptiveSampler(cam, 4096, 4096)  # equal: the maximum doubles to 8192
    with pytest.raises(ValueError, match="positive"):
        core.AdaptiveSampler(cam, 0, 8)


# ---- 2. the decision, known answers ----
def _grey(*v):
    return np.array([[x, x, x] for x in v], np.float32)


def test_decision_known_answers():
    assert abs(ar.luminance((1.0, 1.0, 1.0)) - 1.0) < 1e-15 and ar.luminance((0, 1, 0)) == 0.715160
    assert not ar.needs_supersampling(_grey(0.25, 0.25, 0.25, 0.25))       # all equal
    assert not ar.needs_supersampling(_grey(0.0, 0.0, 0.0, 0.0))           # all black: 0 / 0 is NaN, never > 0.5
    assert not ar.needs_supersampling(_grey(0.0, 0.0))
    assert ar.needs_supersampling(_grey(1.0, 1.0, 1.0, 9.0))               # one outlier: Lavg 3, |9 - 3| / 3 = 2
    assert ar.needs_supersampling(_grey(0.0, 1.0))                         # Lavg 0.5: both samples are 1.0 away in contrast
    assert ar.needs_supersampling(_grey(1.0, 1.0, 1.0, 0.0))               # Lavg 0.75, the black sample: 1.0
    # the boundary: grey samples 1 and 3 -- Lavg = 2 lum(1) and both contrasts are 0.5 exactly, provided lum(3) == 3 lum(1) and the
    # halving are exact in f64.  They are for these values (asserted first), so neither sample exceeds the STRICT comparison.
    l1, l3 = ar.luminance((1, 1, 1)), ar.luminance((3, 3, 3))
    avg = (np.float64(0.0) + l1 + l3) / 2
    assert abs(l1 - avg) / avg == 0.5 and abs(l3 - avg) / avg == 0.5
    assert not ar.needs_supersampling(_grey(1.0, 3.0))
    assert ar.needs_supersampling(_grey(1.0, 3.0000005))                   # one f32 step beyond it
    # negative luminance average: the contrast is negative, never flagged (the expression is literal)
    assert not ar.needs_supersampling(_grey(-1.0, -3.0))
    # order of the serial sum matters in f64: the restatement sums in sample order from 0.0
    px, flags, black = ar.flagged_pixels([(0, 0)] * 4 + [(1, 0)] * 4, np.concatenate([_grey(1, 1, 1, 9), _grey(0, 0, 0, 0)]), 4)
    assert px.tolist() == [[0, 0], [1, 0]] and flags.tolist() == [True, False] and black.tolist() == [False, True]


# ---- 3. the oracle composition ----
def test_oracle_composition_on_c1(ob):
    """The figures the GPU cases rest on: C1 at 32 x 24, 825 sampler pixels, 700 of them black at min = 4, 35 flagged; at min = 2, 702
    black and 25 flagged.  The composition differs from both plain renders and covers every pixel once."""
    prims, r = _c1(4, 32)
    osc = ob.OracleScene(prims)
    got = ar.oracle_adaptive(ob, osc, r, 4, 32)
    assert len(got["pixels"]) == 33 * 25 == 825
    assert int(got["flags"].sum()) == 35 and int(got["black"].sum()) == 700
    assert not (got["flags"] & got["black"]).any()
    lo = ob.render_desc(r, sampler_mode=1)
    lo.spp = 4
    hi = ob.render_desc(r, sampler_mode=1)
    hi.spp = 32
    film_lo, film_hi = osc.render(lo)["film"], osc.render(hi)["film"]
    assert not np.array_equal(got["film"], film_lo) and not np.array_equal(got["film"], film_hi)
    # box filter: a film pixel holds its own pixel's samples -- 4 or 32 of them, 32 exactly where the pixel is flagged
    w = got["film"][..., 3]
    assert set(np.unique(w).tolist()) == {4.0, 32.0}
    f = r.camera.film
    inside = [(x, y) for (x, y) in got["flagged"] if f.left <= x < f.left + f.width and f.top <= y < f.top + f.height]
    assert int((w == 32.0).sum()) == len(inside) and all(w[y - f.top, x - f.left] == 32.0 for x, y in inside)
    assert np.array_equal(got["film"][w == 4.0], film_lo[w == 4.0]) and np.array_equal(got["film"][w == 32.0], film_hi[w == 32.0])
    two = ar.oracle_adaptive(ob, osc, _c1(2, 4)[1], 2, 4)
    assert int(two["flags"].sum()) == 25 and int(two["black"].sum()) == 702


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


def test_loader_builds_the_adaptive_sampler(tmp_path):
    def renderer(line):
        f = tmp_path / "a.pbrt"
        f.write_text(_PBRT % line)
        return pbrt.load(str(f)).rendererObject
    s = renderer('Sampler "adaptive"').sampler
    assert isinstance(s, core.AdaptiveSampler) and (s.minSamples, s.maxSamples, s.method) == (4, 32, "contrast")
    s = renderer('Sampler "adaptive" "integer minsamples" [3] "integer maxsamples" [100] "string method" ["contrast"]').sampler
    assert (s.minSamples, s.maxSamples, s.samplesPerPixel) == (4, 128, 128)
    s = renderer('Sampler "adaptive" "integer minsamples" [16] "integer maxsamples" [2]').sampler
    assert (s.minSamples, s.maxSamples) == (2, 16)
    s = renderer('Sampler "adaptive" "string method" ["entropy"]').sampler  # unknown: 'contrast', as the reference warns and does
    assert s.method == "contrast" and (s.minSamples, s.maxSamples) == (4, 32)
    with pytest.raises(pbrt.UnsupportedFeature, match=r"a\.pbrt:4.*shapeid") as e:
        renderer('Sampler "adaptive" "string method" ["shapeid"]')
    assert "adaptive" in str(e.value)
    with pytest.raises(pbrt.UnsupportedFeature, match="4096"):
        renderer('Sampler "adaptive" "integer maxsamples" [5000]')
    assert isinstance(renderer('Sampler "lowdiscrepancy" "integer pixelsamples" [4]').sampler, core.LowDiscrepancySampler)


# ---- 5. descriptor and ABI ----
def test_abi_of_the_adaptive_mode():
    assert _abi.DrRenderDesc.strat_xsamples.offset == 1292 and C.sizeof(_abi.DrRenderDesc) == 1352
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    v = int(re.search(r"#define DR_ABI_VERSION (\d+)", header).group(1))
    assert v == _abi.DR_ABI_VERSION == int(re.search(r"static const int ABI_VERSION = (\d+);", dart).group(1)) == 9
    c = int(re.search(r"#define DR_SAMPLER_ADAPTIVE (\d+)", header).group(1))
    assert c == _abi.DR_SAMPLER_ADAPTIVE == int(re.search(r"const int DR_SAMPLER_ADAPTIVE = (\d+);", dart).group(1)) == 4
    assert len({_abi.DR_SAMPLER_HOST_BUFFER, _abi.DR_SAMPLER_COUNTER, _abi.DR_SAMPLER_STRATIFIED, _abi.DR_SAMPLER_STRATIFIED_NOJITTER,
                _abi.DR_SAMPLER_ADAPTIVE}) == 5
    assert "DR_ABI_OFFSET(DrRenderDesc, strat_xsamples, 1292);" in header and "DR_ABI_SIZE(DrRenderDesc, 1352);" in header
    assert "dr_scene_get_adaptive_pixels" in _abi.EXPORTS and re.search(r"\bdr_scene_get_adaptive_pixels\s*\(", header)
    assert "lookupFunction<_AdaptivePixelsC, _AdaptivePixelsD>('dr_scene_get_adaptive_pixels')" in dart
    assert "adapt.minSamples" in dart and "adapt.maxSamples" in dart and "OFF_DrRenderDesc_strat_xsamples, minSamples" in dart
    prims, r = _c1(3, 20, seed=9)
    d, _ = r.describe()
    assert (d.sampler_mode, d.strat_xsamples, d.spp, d.seed) == (_abi.DR_SAMPLER_ADAPTIVE, 4, 32, 9)
    # the other samplers' descriptors are what they were
    r.sampler = core.LowDiscrepancySampler(r.camera, 8, 9)
    d, _ = r.describe()
    assert (d.sampler_mode, d.strat_xsamples, d.spp) == (_abi.DR_SAMPLER_COUNTER, 0, 8)


def test_library_exports_the_new_entry_point_and_reports_the_version(hip):
    lib = hip.lib()
    assert lib.dr_abi_version() == 9 and b"abi 9" in lib.dr_version()
    n = C.c_uint64(7)
    assert lib.dr_scene_get_adaptive_pixels(None, None, 0, C.byref(n)) == -1  # DR_ERR_INVALID: no scene
    assert b"null" in lib.dr_last_error()
