"""The edge-avoiding a-trous denoiser on the GPU (k_image_pack<DnInputs> / k_denoise_level<DnRule>): dr_denoise_atrous (host buffers) and
dr_denoise_atrous_device (torch tensors, a stream of its own) against dr_denoise_atrous_host bit for bit -- the host entry is itself held to
the numpy restatement by tests/test_denoise.py -- and render_denoised on a small Cornell scene against the restatement.  The host result of a
case is computed once and shared.  Nothing is started after a failed call: every call's return code raises."""
import ctypes as C

import numpy as np
import pytest
import torch

from dartray_amd import _abi, core, denoise, scenes

import denoise_cases as dc
import denoise_restatement as dr

pytestmark = pytest.mark.gpu

same = dr.same_bits
# (w, h) -> the level counts: the CPU suite's shapes at every level count, and two shapes of more than one tile row and column -- 129 x 65 is
# no multiple of the 64 x 4 tile either way -- at 5 levels
CASES = [(size, dc.ITERATIONS) for size in dc.SIZES] + [((129, 65), [5]), ((256, 256), [5])]
_IDS = ["%dx%d" % size for size, _ in CASES]
_host = {}


def _reference(size, iterations, k):
    key = (size, iterations, k)
    if key not in _host:
        _host[key] = dc.host(*dc.images(*size), iterations, *k)
    return _host[key]


def _combos(size):
    return dc.K_COMBOS if size[0] * size[1] <= 64 * 64 else [dc.K_COMBOS[0], dc.K_COMBOS[-1]]


@pytest.mark.parametrize("size,levels", CASES, ids=_IDS)
def test_host_buffer_entry_equals_the_host_filter_bit_for_bit(gpu, size, levels):
    rgb, normal, depth = dc.images(*size)
    for iterations in levels:
        for k in _combos(size):
            rc, out = dc.call(gpu.lib().dr_denoise_atrous, rgb, normal, depth, iterations, *k)
            _abi.check(rc)
            assert same(out, _reference(size, iterations, k)), (iterations, k)


def _device_call(lib, stream, rgb, normal, depth, p, out, scratch, nbytes):
    n = C.c_uint64(nbytes)
    return lib.dr_denoise_atrous_device(rgb.data_ptr(), normal.data_ptr(), depth.data_ptr(), depth.shape[1], depth.shape[0], C.byref(p),
                                        out.data_ptr(), scratch.data_ptr() if scratch is not None else None, C.byref(n), stream.cuda_stream), n.value


@pytest.mark.parametrize("size,levels", CASES, ids=_IDS)
def test_device_entry_on_its_own_stream_equals_the_host_filter_bit_for_bit(gpu, size, levels):
    lib = gpu.lib()
    w, h = size
    rgb, normal, depth = (torch.from_numpy(a).cuda() for a in dc.images(*size))
    out = torch.empty_like(rgb)
    stream = torch.cuda.Stream()
    # the size query answers first, and touches nothing
    rc, need = _device_call(lib, stream, rgb, normal, depth, dc.params(5, 1.0, 1.0, 1.0), out, None, 0)
    _abi.check(rc)
    assert need == 48 * w * h
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                            # the uploads, before another stream reads them
    for iterations in levels:
        for k in _combos(size):
            out.fill_(-7.0)
            torch.cuda.synchronize()
            rc, _ = _device_call(lib, stream, rgb, normal, depth, dc.params(iterations, *k), out, scratch, need)
            _abi.check(rc)
            stream.synchronize()
            assert same(out.cpu().numpy(), _reference(size, iterations, k)), (iterations, k)


def test_device_entry_refuses_aliased_and_short_buffers(gpu):
    lib = gpu.lib()
    rgb, normal, depth = (torch.from_numpy(a).cuda() for a in dc.images(17, 33))
    out = torch.empty_like(rgb)
    need = 48 * 17 * 33
    scratch = torch.empty(need + 12 * 17 * 33, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    p = dc.params(2, 1.0, 1.0, 1.0)
    torch.cuda.synchronize()

    def refused(needle, *args):
        rc, _ = _device_call(lib, stream, *args)
        assert rc == -1 and needle in lib.dr_last_error().decode(), (needle, rc, lib.dr_last_error())

    refused("out overlaps an input", rgb, normal, depth, p, rgb, scratch, need)
    refused("out overlaps an input", rgb, normal, depth, p, normal, scratch, need)
    refused("out overlaps the scratch buffer", rgb, normal, depth, p, scratch[need - 16:].view(torch.float32), scratch, need)
    refused("the scratch buffer is too small", rgb, normal, depth, p, out, scratch, need - 1)
    refused("not 16-byte aligned", rgb, normal, depth, p, out, scratch[4:], need)
    # an output right behind the scratch buffer is no overlap, and the call is served
    tail = scratch[need:].view(torch.float32).view(33, 17, 3)
    rc, _ = _device_call(lib, stream, rgb, normal, depth, p, tail, scratch, need)
    _abi.check(rc)
    stream.synchronize()
    assert same(tail.cpu().numpy(), _reference((17, 33), 2, (1.0, 1.0, 1.0)))


# ---- the render level ----
@pytest.fixture(scope="module")
def cornell(gpu):
    """The small Cornell box with the blob, 64 x 64 at 4 samples per pixel: (scene, renderer factory, render_denoised's result)."""
    prims, mk = scenes.config("C2", xres=64, yres=64, spp=4, blob=(24, 12))
    scene = scenes.make_scene(prims)
    return scene, mk, denoise.render_denoised(mk(), scene)


def test_render_denoised_equals_the_restatement_of_its_own_images(cornell):
    scene, mk, out = cornell
    p = denoise.params()
    assert out.rgb.shape == out.noisy.shape == out.normal.shape == (64, 64, 3) and out.depth.shape == (64, 64)
    assert same(out.rgb, dr.atrous(out.noisy, out.normal, out.depth, p.iterations, p.k_color, p.k_normal, p.k_depth))
    assert not same(out.rgb, out.noisy) and np.isfinite(out.rgb).all()
    hit = out.depth > 0
    assert 0.5 < hit.mean() and out.normal[hit].max() > 0.9 and out.noisy.max() > 0


def test_render_denoised_exposes_the_renders_of_the_same_renderers(cornell):
    scene, mk, out = cornell
    r = mk()
    assert same(out.noisy, r.render(scene).rgb) and same(out.film, r.render(scene).film)

    def feature(channel):
        return core.SamplerRenderer(r.sampler, r.camera, core.FeatureIntegrator(channel), core.EmissionIntegrator()).render(scene).rgb
    assert same(out.normal, feature("ns")) and same(out.depth, feature("depth")[..., 0])
    ng = denoise.render_denoised(r, scene, normal_channel="ng", iterations=2, sigma_depth=float("inf"))
    assert same(ng.normal, feature("ng")) and same(ng.noisy, out.noisy)
    assert same(ng.rgb, dr.atrous(ng.noisy, ng.normal, ng.depth, 2, 1.0, denoise.sharpness(0.1), 0.0))


def test_quality_figures_are_finite(cornell):
    """The figures MEASUREMENTS.md reports: the mean squared error of the 4-spp image and of the denoised one against a 1024-spp render."""
    scene, mk, out = cornell
    prims, mk_ref = scenes.config("C2", xres=64, yres=64, spp=1024, blob=(24, 12))
    ref = mk_ref().render(scene).rgb.astype(np.float64)
    noisy = float(((out.noisy - ref) ** 2).mean())
    filtered = float(((out.rgb - ref) ** 2).mean())
    p = denoise.params()
    print("denoise quality, C2-small 64x64: mse(4 spp) = %.6g, mse(4 spp denoised) = %.6g against 1024 spp; iterations %d, k_color %g, k_normal %g, "
          "k_depth %g" % (noisy, filtered, p.iterations, p.k_color, p.k_normal, p.k_depth))
    assert np.isfinite(noisy) and np.isfinite(filtered)
