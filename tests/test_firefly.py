"""Firefly suppression without a GPU: answers derived by hand, checked against both the numpy restatement
(tests/firefly_restatement.py, written from the text) and dr_firefly_host after those two agree bit for bit; the two against each other on
every seeded case of tests/firefly_cases.py, each of which is first held to the condition that makes it a test -- it clamps a pixel and
leaves a valid one alone; every refusal by code and text; the host code under the address and undefined-behaviour sanitizers as a
stand-alone program (tests/firefly_host_check.cpp); and the Python module above them (dartray_amd/denoise.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, denoise, scenes

import firefly_cases as fc
import firefly_restatement as fr

F = np.float32
same = fr.same_bits
BASE = np.float32([0.5, 0.4, 0.3])


def _both(rgb, normal, depth, ps=fc.DEFAULTS):
    """The restatement's and the host entry's (out, removed), which must agree before either is compared with a derived answer.
    ps = (radius, rank, threshold, floor, depth_tol, normal_tol)."""
    a = fr.firefly(rgb, normal, depth, *ps)
    b = fc.host(rgb, normal, depth, ps)
    assert same(a[0], b[0]) and same(a[1], b[1]), ps
    return a


def _flat(w, h, colour=BASE):
    """One surface, one colour."""
    return (np.broadcast_to(np.float32(colour), (h, w, 3)).copy(), np.full((h, w, 3), 0.5, np.float32), np.full((h, w), 3.0, np.float32))


def _with(ps=fc.DEFAULTS, **kw):
    names = ("radius", "rank", "threshold", "floor", "depth_tol", "normal_tol")
    return tuple(kw.get(n, v) for n, v in zip(names, ps))


def _changed(out, rgb):
    return (out.view(np.uint32) != rgb.view(np.uint32)).any(axis=2)


# ---- 1. answers derived by hand ----
@pytest.mark.parametrize("limit", fc.LIMITS + [(2.0, 1.0)], ids=str)
@pytest.mark.parametrize("radius", fc.RADII)
def test_a_lone_outlier_on_a_flat_field_is_scaled_to_the_limit(hip, radius, limit):
    rgb, normal, depth = _flat(5, 7)
    rgb[3, 2] = F(100) * BASE
    out, removed = _both(rgb, normal, depth, _with(radius=radius, threshold=limit[0], floor=limit[1]))
    m, l = fr.lum(BASE), fr.lum(rgb[3, 2])                               # every member is as bright as the field
    t = F(limit[0]) * m + F(limit[1])
    s = t / l
    if limit == (0.0, 0.0):                                              # the limit is 0 for every pixel: all of them lit, all go black (+0)
        assert same(out, np.zeros_like(rgb)) and same(removed, fr.lum(rgb))
        return
    want = rgb.copy()
    want[3, 2] = rgb[3, 2] * s
    assert t < l and same(out, want) and same(removed[3, 2], l - t) and (np.delete(removed.reshape(-1), 3 * 5 + 2) == 0).all()


def test_b_two_adjacent_outliers_survive_rank_one_and_are_both_clamped_at_rank_two(hip):
    rgb, normal, depth = _flat(5, 7)
    rgb[3, 2] = rgb[3, 3] = F(100) * BASE
    out, removed = _both(rgb, normal, depth, _with(rank=1))
    assert same(out, rgb) and (removed == 0).all()                       # each is the other's brightest member
    out, removed = _both(rgb, normal, depth)
    t = F(4) * fr.lum(BASE) + F(0)
    want = rgb.copy()
    want[3, 2] = want[3, 3] = rgb[3, 2] * (t / fr.lum(rgb[3, 2]))
    assert same(out, want) and (removed != 0).sum() == 2


def test_c_a_bright_line_and_a_bright_block_survive_rank_two(hip):
    rgb, normal, depth = _flat(9, 7)
    rgb[3, :] = F(100) * BASE                                            # a line one pixel wide, from edge to edge
    out, _ = _both(rgb, normal, depth)
    # every pixel of the line with a bright neighbour on either side stays; its two ends, at the image's edge, have one and are clamped
    assert same(out[3, 1:-1], rgb[3, 1:-1]) and _changed(out, rgb).sum() == 2 and _changed(out, rgb)[3, [0, 8]].all()
    rgb, normal, depth = _flat(9, 7)
    rgb[2:5, 3:6] = F(100) * BASE                                        # a corner of the block has three bright neighbours
    out, removed = _both(rgb, normal, depth)
    assert same(out, rgb) and (removed == 0).all()
    out, _ = _both(rgb, normal, depth, _with(rank=4))                    # ... and no fourth
    assert _changed(out, rgb).sum() == 4 and _changed(out, rgb)[[2, 2, 4, 4], [3, 5, 3, 5]].all()


@pytest.mark.parametrize("step", ["depth", "normal"])
def test_d_an_outlier_across_a_guide_step_has_too_few_members_and_passes_through(hip, step):
    rgb, normal, depth = _flat(5, 7)
    rgb[3, 2] = F(100) * BASE
    if step == "depth":
        depth[3, 2] = 3.5                                                # 14 % off: outside depth_tol * z either way
    else:
        normal[3, 2] = 0.5 + 0.2                                         # a squared distance of 0.12
    out, removed = _both(rgb, normal, depth)
    assert same(out, rgb) and (removed == 0).all()
    n, _ = fr.members(rgb, normal, depth, 1, fc.DEPTH_TOL, fc.NORMAL_TOL)
    assert n[3, 2] == 0 and n[3, 1] == 7 and n[0, 0] == 3
    wide = _with(depth_tol=0.2, normal_tol=0.2)
    out, _ = _both(rgb, normal, depth, wide)
    assert _changed(out, rgb).sum() == 1 and _changed(out, rgb)[3, 2]
    # one member on the outlier's side of the step is still fewer than rank 2, and enough for rank 1
    if step == "depth":
        depth[3, 3] = 3.5
    else:
        normal[3, 3] = 0.5 + 0.2
    out, _ = _both(rgb, normal, depth)
    assert same(out, rgb)
    out, _ = _both(rgb, normal, depth, _with(rank=1))
    assert _changed(out, rgb).sum() == 1 and _changed(out, rgb)[3, 2]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=str)
@pytest.mark.parametrize("plane", ["rgb", "normal", "depth"])
def test_e_a_non_finite_pixel_passes_through_and_is_in_no_set(hip, plane, bad):
    """A row of three: field, outlier, invalid.  The outlier's only member is the field pixel, one short of rank 2."""
    rgb, normal, depth = _flat(3, 1)
    rgb[0, 1] = F(100) * BASE
    ok = _both(rgb, normal, depth)[0]
    assert _changed(ok, rgb)[0, 1]                                       # with a valid third pixel it is clamped
    rgb[0, 2, 0] = 1.0e6
    if plane == "depth":
        depth[0, 2] = bad
    else:
        dict(rgb=rgb, normal=normal)[plane][0, 2, 1] = bad
    out, removed = _both(rgb, normal, depth)
    assert same(out, rgb) and (removed == 0).all()
    out1, _ = _both(rgb, normal, depth, _with(rank=1))                   # at rank 1 the field pixel alone is the limit, not the 1e6
    assert same(out1[0, 1], rgb[0, 1] * ((F(4) * fr.lum(BASE) + F(0)) / fr.lum(rgb[0, 1]))) and same(out1[0, 2], rgb[0, 2])


def test_f_on_every_case_removed_is_the_luminance_taken_and_unchanged_pixels_keep_their_bits(hip):
    n = 0
    for key, (rgb, normal, depth), ps in fc.grid():
        out, removed = fc.host(rgb, normal, depth, ps)
        valid = fr.valid(rgb, normal, depth)
        with np.errstate(all="ignore"):
            lin, lout = fr.lum(rgb), fr.lum(out)
        clamped = removed != 0
        assert (removed >= 0).all() and not clamped[~valid].any(), key
        assert same(out[~clamped], rgb[~clamped]), key                   # bytes, NaN payloads and zero signs included
        assert (lout[valid] <= lin[valid]).all(), key
        assert (lin[clamped] > 0).all() and (lout[clamped] < lin[clamped]).all(), key
        # removed = L - T0, and out's luminance is T0 up to the roundings of s = T0 / L, the three products and the weighted sum: half an
        # ulp each of s and a product, and five more in the sum's terms, all relative to the luminance of the channels' magnitudes
        t0 = lin[clamped] - removed[clamped]
        assert (np.abs(lout[clamped] - t0) <= 8 * np.finfo(np.float32).eps * fr.lum(np.abs(rgb))[clamped]).all(), key
        n += 1
    assert n == len(fc.SIZES) * len(fc.KINDS) * len(fc.PARAM_SETS) == 875


# ---- 2. host == restatement, bit for bit, on cases that test something ----
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("size", fc.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_bit_for_bit(hip, size, kind):
    rgb, normal, depth = fc.image(*size, kind)
    valid = fr.valid(rgb, normal, depth)
    if kind == "extremes" and size[0] * size[1] >= 325:                  # 3 % of the pixels each: the three larger images hold them all
        assert not valid.all() and (rgb < 0).any() and (np.abs(rgb) >= 3e38).any() and ((rgb != 0) & (np.abs(rgb) < 1e-38)).any()
    if size != (1, 1):
        black = rgb[(rgb == 0).all(axis=2)]
        assert np.signbit(black).any() and not np.signbit(black).all()   # both zeros
    outs = []
    for ps in fc.PARAM_SETS:
        out, removed = _both(rgb, normal, depth, ps)
        assert (out != fc.SENTINEL).all() and (removed != fc.SENTINEL).all()
        changed = _changed(out, rgb)
        count, _ = fr.members(rgb, normal, depth, ps[0], ps[4], ps[5])
        if (count >= ps[1]).any():                                       # the case's condition (tests/firefly_cases.py)
            assert changed.any() and (valid & ~changed).any(), ps
        else:
            assert not changed.any() and (size[0] == 1 or size[1] == 1), ps
        without = fc.host(rgb, normal, depth, ps, with_removed=False)[0]
        assert same(without, out), ps
        outs.append(np.concatenate([out.reshape(-1), removed.reshape(-1)]))
    if size == (64, 48) and kind == "surfaces":
        # every parameter is read: no two sets with a limit above 0 agree (at threshold 0, floor 0 every lit pixel with enough members goes
        # black, whatever the rank)
        lit = [k for k, ps in enumerate(fc.PARAM_SETS) if ps[2] > 0]
        agree = [(fc.PARAM_SETS[i], fc.PARAM_SETS[j]) for i in lit for j in lit if j < i and same(outs[i], outs[j])]
        assert not agree, agree


# ---- 3. the refusals, by code and text ----
def test_every_refusal_by_code_and_text(hip):
    lib = hip.lib()
    rgb, normal, depth = fc.image(3, 2, "smooth")
    # the outputs lie in one allocation with room behind them: a pointer moved past an output's end stays clear of the inputs wherever the
    # heap has put those
    room = np.zeros(64, np.float32)
    outs = dict(out=room[:18].reshape(2, 3, 3), removed=room[18:24].reshape(2, 3))
    arrays = dict(rgb=rgb, normal=normal, depth=depth, **outs)
    ptr = {k: v.ctypes.data for k, v in arrays.items()}
    inputs = ["rgb", "normal", "depth"]
    ok = fc.params(*fc.DEFAULTS)

    def refused(needle, w=3, h=2, p=ok, images_only=False, **over):
        a = dict(ptr, **over)
        pp = C.byref(p) if p is not None else None
        calls = [lambda fn=fn: fn(*[a[k] for k in inputs], w, h, pp, a["out"], a["removed"]) for fn in (lib.dr_firefly_host, lib.dr_firefly)]
        calls.append(lambda: lib.dr_firefly_device(*[a[k] for k in inputs], w, h, pp, a["out"], a["removed"], None))
        if not images_only:
            calls.append(lambda: lib.dr_firefly_check(pp, w, h))
        for one in calls:                                                # the same checks, ahead of any device call
            rc = one()
            assert rc == -1, (needle, rc)
            assert needle in lib.dr_last_error().decode(), (needle, lib.dr_last_error())

    def with_(**fields):
        p = fc.params(*fc.DEFAULTS)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    for name in inputs + ["out"]:
        refused("a null pointer", images_only=True, **{name: None})
    refused("a null pointer", p=None)
    refused("w and h must be at least 1", w=0)
    refused("w and h must be at least 1", h=-2)
    refused("the image has 2^31 or more pixels", w=65536, h=32768)
    refused("the image has 2^31 or more pixels", w=2 ** 31 - 1, h=2 ** 31 - 1)
    assert lib.dr_firefly_check(C.byref(ok), 65536, 32767) == 0
    for bad in (0, 3, -1, 2 ** 31 - 1):
        refused("radius must be 1 or 2", p=with_(radius=bad))
    for bad in (0, 5, -1, 2 ** 31 - 1):
        refused("rank must be in 1..4", p=with_(rank=bad))
    for bad in (-1.0, float("inf"), float("nan"), float("-inf"), -1e-30):
        refused("threshold must be finite and not negative", p=with_(threshold=bad))
        refused("floor must be finite and not negative", p=with_(floor=bad))
        refused("depth_tol and normal_tol must be finite and not negative", p=with_(depth_tol=bad))
        refused("depth_tol and normal_tol must be finite and not negative", p=with_(normal_tol=bad))
    for r, k in ((1, 1), (2, 4)):
        assert lib.dr_firefly_check(C.byref(with_(radius=r, rank=k, threshold=0.0, floor=0.0, depth_tol=0.0, normal_tol=0.0)), 3, 2) == 0
    assert lib.dr_firefly_check(C.byref(with_(threshold=-0.0, floor=-0.0)), 3, 2) == 0      # not < 0
    nbytes = {k: v.nbytes for k, v in arrays.items()}
    for o in outs:
        for name in inputs:
            refused("an output overlaps an input", images_only=True, **{o: ptr[name]})
            refused("an output overlaps an input", images_only=True, **{o: ptr[name] + nbytes[name] - 4})     # its first float is the input's last
            refused("an output overlaps an input", images_only=True, **{name: ptr[o] + nbytes[o] - 4})
    refused("an output overlaps another output", images_only=True, removed=ptr["out"] + 8)
    refused("an output overlaps another output", images_only=True, removed=ptr["out"] + nbytes["out"] - 4)
    refused("an output overlaps another output", images_only=True, out=ptr["removed"] + nbytes["removed"] - 4)
    # nothing of the above left a mark, and a NULL removed is served
    assert lib.dr_firefly_check(C.byref(ok), 3, 2) == 0
    assert lib.dr_firefly_host(*[ptr[k] for k in inputs], 3, 2, C.byref(ok), ptr["out"], None) == 0
    assert same(outs["out"], fr.firefly(rgb, normal, depth, *fc.DEFAULTS)[0]) and (outs["removed"] == 0).all()


def test_the_struct_is_twenty_four_bytes_in_every_binding():
    assert C.sizeof(_abi.DrFireflyParams) == 24
    assert [(n, getattr(_abi.DrFireflyParams, n).offset) for n, _ in _abi.DrFireflyParams._fields_] == [
        ("radius", 0), ("rank", 4), ("threshold", 8), ("floor", 12), ("depth_tol", 16), ("normal_tol", 20)]
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    assert "DR_ABI_SIZE(DrFireflyParams, 24);" in header and "#define DR_ABI_VERSION 9" in header
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    assert "const int SIZEOF_DrFireflyParams = 24;" in dart
    for sym in ("dr_firefly_check", "dr_firefly_host", "dr_firefly", "dr_firefly_device"):
        assert "('%s')" % sym in dart, sym


# ---- 4. the host code under the sanitizers, as a program of its own ----
def test_host_loop_runs_clean_under_the_sanitizers(tmp_path):
    """tests/firefly_host_check.cpp + dr_firefly_host.cpp, built with -fsanitize=address,undefined and run as a child process; the
    sanitizer runtimes are linked into the program, which then depends on nothing else the process loads."""
    exe = str(tmp_path / "firefly_host_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "firefly_host_check.cpp"),
                           os.path.join(ROOT, "dartray_amd", "csrc", "dr_firefly_host.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "firefly_host_check: OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ---- 5. the Python module ----
def test_the_defaults_are_the_documented_ones():
    p = denoise.firefly_params()
    assert (p.radius, p.rank, p.threshold, p.floor) == (1, 2, 4.0, 0.0)
    assert (p.depth_tol, p.normal_tol) == (float(F(denoise.DEPTH_TOL)), float(F(denoise.NORMAL_TOL))) == (float(F(0.02)), float(F(0.05)))
    assert (denoise.FIREFLY_RADIUS, denoise.FIREFLY_RANK, denoise.FIREFLY_THRESHOLD, denoise.FIREFLY_FLOOR) == (1, 2, 4.0, 0.0)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "radius = 1, rank = 2, threshold = 4, floor = 0, depth_tol = 0.02, normal_tol = 0.05" in design
    p = denoise.firefly_params(radius=2, rank=4, threshold=1.5, floor=0.25, depth_tol=0.1, normal_tol=0.0)
    assert (p.radius, p.rank, p.threshold, p.floor, p.depth_tol, p.normal_tol) == (2, 4, 1.5, 0.25, float(F(0.1)), 0.0)


def test_the_module_on_the_host_equals_the_restatement(hip):
    rgb, normal, depth = fc.image(65, 5, "surfaces")
    out = denoise.firefly(rgb, normal, depth, device=False)
    want = fr.firefly(rgb, normal, depth, *fc.DEFAULTS)
    assert out.dtype == np.float32 and same(out, want[0]) and not same(out, rgb)
    out, removed = denoise.firefly(rgb, normal, depth, radius=2, rank=3, threshold=1.5, floor=0.25, device=False, return_removed=True)
    want = fr.firefly(rgb, normal, depth, 2, 3, 1.5, 0.25, fc.DEPTH_TOL, fc.NORMAL_TOL)
    assert same(out, want[0]) and same(removed, want[1]) and (removed > 0).any()
    out = denoise.firefly(rgb.astype(np.float64), normal.tolist(), depth, depth_tol=0.0, normal_tol=0.0, device=False)
    assert same(out, fr.firefly(rgb, normal, depth, 1, 2, 4.0, 0.0, 0.0, 0.0)[0])
    with pytest.raises(ValueError, match=r"firefly: rgb and normal must be \[h, w, 3\] and depth \[h, w\] \(got \(5, 65, 3\), \(5, 65, 3\), \(5, 64\)\)"):
        denoise.firefly(rgb, normal, depth[:, :64], device=False)
    with pytest.raises(ValueError, match=r"firefly: rgb and normal must be \[h, w, 3\]"):
        denoise.firefly(rgb[..., 0], normal, depth, device=False)
    with pytest.raises(ValueError, match=r"firefly: rgb and normal must be \[h, w, 3\]"):
        denoise.firefly(rgb, normal[:4], depth, device=False)
    with pytest.raises(_abi.DartRayHipError, match="radius must be 1 or 2"):
        denoise.firefly(rgb, normal, depth, radius=3, device=False)
    with pytest.raises(_abi.DartRayHipError, match=r"rank must be in 1\.\.4"):
        denoise.firefly(rgb, normal, depth, rank=0, device=False)
    with pytest.raises(_abi.DartRayHipError, match="threshold must be finite and not negative"):
        denoise.firefly(rgb, normal, depth, threshold=float("nan"), device=False)


def _renderer():
    cam = scenes.cornell_camera(16, 16)
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, 4, 5489), cam, core.PathIntegrator(3), core.EmissionIntegrator())


def test_the_firefly_keyword_refuses_by_name_before_anything_renders():
    r = _renderer()
    calls = {"render_denoised": lambda **kw: denoise.render_denoised(r, None, **kw),
             "render_denoised_pair": lambda **kw: denoise.render_denoised_pair(r, None, **kw),
             "render_upsampled": lambda **kw: denoise.render_upsampled(r, r, None, **kw),
             "render_sequence": lambda **kw: denoise.render_sequence([r], None, **kw)}
    for who, call in calls.items():
        with pytest.raises(ValueError, match=r"%s: firefly must be False, True or a dict of firefly\(\)'s parameters, got 1" % who):
            call(firefly=1)
        with pytest.raises(ValueError, match="%s: firefly has no parameter iterations, sigma" % who):
            call(firefly={"rank": 1, "sigma": 2.0, "iterations": 3})
    with pytest.raises(ValueError, match="render_firefly: normal_channel must be ns or ng"):
        denoise.render_firefly(r, None, normal_channel="uv")
