"""Demodulation on the GPU (k_demodulate, k_remodulate): dr_demodulate / dr_remodulate (host buffers) and their _device
forms (torch tensors, a stream of its own) against the host loops bit for bit -- the host loops are held to the numpy restatement by
tests/test_demodulate.py -- and the `demodulate` keyword of render_denoised, render_denoised_pair and render_sequence on small renders
against the chain rebuilt by hand from the images they return.  Nothing is started after a failed call: every call's return code raises."""
import ctypes as C

import numpy as np
import pytest
import torch

from dartray_amd import _abi, core, denoise, scenes

import demodulate_cases as dc

pytestmark = pytest.mark.gpu
same = dc.same
F = np.float32
SEED = 5489


def _call(fn, rgb, e, a, eps=dc.EPS):
    h, w = rgb.shape[:2]
    out = np.full_like(rgb, 7.0)
    p = _abi.DrDemodulateParams(eps)
    _abi.check(fn(rgb.ctypes.data, e.ctypes.data if e is not None else None, a.ctypes.data if a is not None else None, w, h, C.byref(p), out.ctypes.data))
    return out


# ---- 1. the kernels against the host loops ----
@pytest.mark.parametrize("absent", sorted(dc.ABSENT))
@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_kernels_equal_the_host_loops_bit_for_bit(gpu, size, absent):
    lib = _abi.lib()
    has_e, has_a = dc.ABSENT[absent]
    stream = torch.cuda.Stream()
    w, h = size
    for rgb, e, a in dc.images(*size):
        e, a = e if has_e else None, a if has_a else None
        want = _call(lib.dr_demodulate_host, rgb, e, a)
        assert same(_call(lib.dr_demodulate, rgb, e, a), want), (size, absent)
        filtered = np.ascontiguousarray(np.where(np.isfinite(want), want * F(0.75), want), F)
        want_re = _call(lib.dr_remodulate_host, filtered, e, a)
        assert same(_call(lib.dr_remodulate, filtered, e, a), want_re), (size, absent)
        # the _device entries on tensors, on a stream of their own
        t = [torch.from_numpy(x).cuda() if x is not None else None for x in (rgb, e, a, filtered)]
        out, out_re = torch.full_like(t[0], 7.0), torch.full_like(t[0], 7.0)
        ptr = lambda x: x.data_ptr() if x is not None else None
        p = _abi.DrDemodulateParams(dc.EPS)
        torch.cuda.synchronize()                                     # the uploads and fills, before another stream reads them
        _abi.check(lib.dr_demodulate_device(ptr(t[0]), ptr(t[1]), ptr(t[2]), w, h, C.byref(p), out.data_ptr(), stream.cuda_stream))
        _abi.check(lib.dr_remodulate_device(ptr(t[3]), ptr(t[1]), ptr(t[2]), w, h, C.byref(p), out_re.data_ptr(), stream.cuda_stream))
        stream.synchronize()
        assert same(out.cpu().numpy(), want) and same(out_re.cpu().numpy(), want_re), (size, absent)


def test_the_exact_round_trip_and_the_overlap_refusal_on_the_device(gpu):
    lib = _abi.lib()
    rgb, e, a, eps = dc.exact_images(67, 9)
    d = _call(lib.dr_demodulate, rgb, e, a, eps)
    assert same(d, _call(lib.dr_demodulate_host, rgb, e, a, eps)) and same(_call(lib.dr_remodulate, d, e, a, eps), rgb)
    t = torch.from_numpy(rgb).cuda()
    p = _abi.DrDemodulateParams(eps)
    torch.cuda.synchronize()
    for fn in (lib.dr_demodulate_device, lib.dr_remodulate_device):
        assert fn(t.data_ptr(), None, None, 67, 9, C.byref(p), t.data_ptr(), None) == -1 and "an output overlaps an input" in lib.dr_last_error().decode()
    assert same(t.cpu().numpy(), rgb)
    assert same(denoise.demodulate(rgb, e, a, eps=eps), d)           # the module's default is the device


# ---- 2. end to end: an emitter in view ----
def _renderer(res, spp=4, seed=SEED):
    cam = scenes.cornell_camera(res, res)
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, spp, seed), cam, core.PathIntegrator(3), core.EmissionIntegrator())


@pytest.fixture(scope="module")
def box(gpu):
    return scenes.make_scene(dc.emitter_box_prims())


def _keeps_lemit(rgb):
    return np.allclose(rgb[dc.INSIDE], np.array(dc.LEMIT, F), rtol=dc.EMITTER_RTOL, atol=dc.EMITTER_ATOL)


def test_render_denoised_keeps_the_emitter_and_equals_the_chain_by_hand(box):
    r = _renderer(32)
    out = denoise.render_denoised(r, box, demodulate=True)
    assert out.emission.shape == out.albedo.shape == out.noisy.shape == (32, 32, 3)
    # the material images are aligned with the beauty image: inside the emitter the render IS the emission, and the emitter's surface is black
    assert _keeps_lemit(out.noisy) and _keeps_lemit(out.emission) and not out.albedo[dc.INSIDE].any()
    assert (out.emission[0] == 0).all() and np.allclose(out.albedo[16, 8], 0.4, rtol=1e-5)
    base = denoise.demodulate(out.noisy, out.emission, out.albedo)
    assert same(out.demodulated, base) and same(base, denoise.demodulate(out.noisy, out.emission, out.albedo, device=False))
    want = denoise.remodulate(denoise.atrous(base, out.normal, out.depth), out.emission, out.albedo)
    assert same(out.rgb, want)
    plain = denoise.render_denoised(r, box)
    assert same(plain.noisy, out.noisy) and same(plain.rgb, denoise.atrous(out.noisy, out.normal, out.depth)) and not hasattr(plain, "emission")
    err = lambda img: np.abs(img[dc.INSIDE] - np.array(dc.LEMIT, F)).max()
    print("emitter interior, max |rgb - Lemit|: unfiltered %.3g, filtered %.3g, demodulated and filtered %.3g (tolerance %.3g)"
          % (err(out.noisy), err(plain.rgb), err(out.rgb), dc.EMITTER_RTOL * 36 + dc.EMITTER_ATOL))
    # what the stage exists for: with it every pixel wholly inside the emitter keeps Lemit through the filter; without it none of them need
    assert _keeps_lemit(out.rgb)
    assert not _keeps_lemit(plain.rgb) and not np.allclose(plain.rgb[16, 16], dc.LEMIT, rtol=dc.EMITTER_RTOL, atol=dc.EMITTER_ATOL)
    # one channel alone, and the firefly clamp behind the demodulation
    for channels in (("emission",), ("albedo",)):
        one = denoise.render_denoised(r, box, demodulate=channels, firefly=True, iterations=2)
        e, a = getattr(one, "emission", None), getattr(one, "albedo", None)
        assert (e is None) != (a is None)
        base = denoise.demodulate(one.noisy, e, a)
        clamped = denoise.firefly(base, one.normal, one.depth)
        assert same(one.rgb, denoise.remodulate(denoise.atrous(clamped, one.normal, one.depth, iterations=2), e, a))


def test_render_denoised_pair_demodulates_both_halves_by_the_same_images(box):
    r = _renderer(32, spp=2)
    out = denoise.render_denoised_pair(r, box, demodulate=True)
    a, b = (denoise.demodulate(x, out.emission, out.albedo) for x in (out.a, out.b))
    assert same(out.demodulated[0], a) and same(out.demodulated[1], b) and not same(out.a, out.b)
    rgb, variance = denoise.atrous_pair(a, b, out.normal, out.depth, return_variance=True)
    assert same(out.rgb, denoise.remodulate(rgb, out.emission, out.albedo)) and same(out.variance, variance)
    plain = denoise.render_denoised_pair(r, box)
    assert same(plain.a, out.a) and same(plain.b, out.b) and same(plain.rgb, denoise.atrous_pair(out.a, out.b, out.normal, out.depth))


@pytest.mark.parametrize("mode", [False, True, "moments"], ids=["accumulate", "atrous", "moments"])
def test_render_sequence_keeps_demodulated_colour_in_the_history(box, mode):
    rs = [_renderer(16, spp=2, seed=SEED + k) for k in range(2)]
    frames = denoise.render_sequence(rs, box, denoise=mode, demodulate=True)
    plain = denoise.render_sequence(rs, box, denoise=mode)
    history = None
    for k, (f, r) in enumerate(zip(frames, rs)):
        assert same(f.noisy, plain[k].noisy) and same(f.normal, plain[k].normal) and not hasattr(plain[k], "albedo")
        base = denoise.demodulate(f.noisy, f.emission, f.albedo)
        assert same(f.demodulated, base)
        history = denoise.temporal(base, f.normal, f.depth, history, denoise.temporal_matrices(r.camera, rs[max(k - 1, 0)].camera))
        assert same(f.accumulated, history.rgb) and same(f.m2, history.m2) and same(f.len, history.len)
        if mode == "moments":
            filtered = denoise.atrous_moments(history)
        else:
            filtered = denoise.atrous(history.rgb, f.normal, f.depth) if mode else history.rgb
        assert same(f.rgb, denoise.remodulate(filtered, f.emission, f.albedo)), (mode, k)
    assert frames[1].len.max() == 2 and not same(frames[1].rgb, plain[1].rgb)
