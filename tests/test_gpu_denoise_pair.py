"""The variance-guided a-trous denoiser on the GPU (k_image_pack<DnpInputs> / k_denoise_level<DnpRule>): dr_denoise_pair (host buffers)
and dr_denoise_pair_device (torch tensors, a stream of its own) against dr_denoise_pair_host bit for bit, in colour and variance -- the host
entry is itself held to the numpy restatement by tests/test_denoise_pair.py -- and render_denoised_pair on a small Cornell scene against the
restatement.  The host result of a case is computed once and shared.  Nothing is started after a failed call: every call's return code raises."""
import ctypes as C

import numpy as np
import pytest
import torch

from dartray_amd import _abi, core, denoise, scenes

import denoise_pair_cases as pc
import denoise_pair_restatement as pr

pytestmark = pytest.mark.gpu

same = pr.same_bits
# (w, h) -> the level counts: the CPU suite's shapes at every level count, and 129 x 65 -- more than one tile row and column, and no multiple
# of the 64 x 4 tile either way -- at 5 levels
CASES = [(size, pc.ITERATIONS) for size in pc.SIZES] + [((129, 65), [5])]
_IDS = ["%dx%d" % size for size, _ in CASES]
_host = {}


def _reference(size, iterations, k):
    key = (size, iterations, k)
    if key not in _host:
        _host[key] = pc.host(*pc.images(*size), iterations, *k)
    return _host[key]


def _combos(size):
    return pc.K_COMBOS if size[0] * size[1] <= 64 * 64 else [pc.K_COMBOS[0], pc.K_COMBOS[-1]]


@pytest.mark.parametrize("size,levels", CASES, ids=_IDS)
def test_host_buffer_entry_equals_the_host_filter_bit_for_bit(gpu, size, levels):
    images = pc.images(*size)
    for iterations in levels:
        for k in _combos(size):
            rc, out, var = pc.call(gpu.lib().dr_denoise_pair, *images, iterations, *k)
            _abi.check(rc)
            want = _reference(size, iterations, k)
            assert same(out, want[0]) and same(var, want[1]), (iterations, k)
    rc, out, none = pc.call(gpu.lib().dr_denoise_pair, *images, levels[-1], *pc.K_COMBOS[-1], variance=False)    # out_var == NULL
    _abi.check(rc)
    assert none is None and same(out, _reference(size, levels[-1], pc.K_COMBOS[-1])[0])


def _device_call(lib, stream, a, b, normal, depth, p, out, var, scratch, nbytes):
    n = C.c_uint64(nbytes)
    return lib.dr_denoise_pair_device(a.data_ptr(), b.data_ptr(), normal.data_ptr(), depth.data_ptr(), depth.shape[1], depth.shape[0], C.byref(p),
                                      out.data_ptr(), var.data_ptr() if var is not None else None,
                                      scratch.data_ptr() if scratch is not None else None, C.byref(n), stream.cuda_stream), n.value


@pytest.mark.parametrize("size,levels", CASES, ids=_IDS)
def test_device_entry_on_its_own_stream_equals_the_host_filter_bit_for_bit(gpu, size, levels):
    lib = gpu.lib()
    w, h = size
    a, b, normal, depth = (torch.from_numpy(x).cuda() for x in pc.images(*size))
    out, var = torch.empty_like(a), torch.empty_like(depth)
    stream = torch.cuda.Stream()
    # the size query answers first, and touches nothing
    rc, need = _device_call(lib, stream, a, b, normal, depth, pc.params(5, 1.0, 1.0, 1.0), out, var, None, 0)
    _abi.check(rc)
    assert need == 48 * w * h
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                            # the uploads, before another stream reads them
    for iterations in levels:
        for k in _combos(size):
            out.fill_(-7.0)
            var.fill_(-7.0)
            torch.cuda.synchronize()
            rc, _ = _device_call(lib, stream, a, b, normal, depth, pc.params(iterations, *k), out, var, scratch, need)
            _abi.check(rc)
            stream.synchronize()
            want = _reference(size, iterations, k)
            assert same(out.cpu().numpy(), want[0]) and same(var.cpu().numpy(), want[1]), (iterations, k)
    out.fill_(-7.0)
    var.fill_(-7.0)
    torch.cuda.synchronize()
    rc, _ = _device_call(lib, stream, a, b, normal, depth, pc.params(levels[-1], *pc.K_COMBOS[-1]), out, None, scratch, need)    # out_var == NULL
    _abi.check(rc)
    stream.synchronize()
    assert same(out.cpu().numpy(), _reference(size, levels[-1], pc.K_COMBOS[-1])[0]) and (var == -7.0).all()


def test_device_entry_refuses_aliased_and_short_buffers(gpu):
    lib = gpu.lib()
    a, b, normal, depth = (torch.from_numpy(x).cuda() for x in pc.images(17, 33))
    out, var = torch.empty_like(a), torch.empty_like(depth)
    need = 48 * 17 * 33
    scratch = torch.empty(need + 16 * 17 * 33, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    p = pc.params(2, 1.0, 1.0, 1.0)
    torch.cuda.synchronize()

    def refused(needle, *args):
        rc, _ = _device_call(lib, stream, *args)
        assert rc == -1 and needle in lib.dr_last_error().decode(), (needle, rc, lib.dr_last_error())

    refused("out overlaps an input", a, b, normal, depth, p, a, var, scratch, need)
    refused("out overlaps an input", a, b, normal, depth, p, b, var, scratch, need)
    refused("out overlaps an input", a, b, normal, depth, p, normal, var, scratch, need)
    refused("out_var overlaps an input", a, b, normal, depth, p, out, depth, scratch, need)
    refused("out_var overlaps an input", a, b, normal, depth, p, out, b.view(-1)[:17 * 33].view(33, 17), scratch, need)
    refused("out overlaps out_var", a, b, normal, depth, p, out, out.view(-1)[5:5 + 17 * 33].view(33, 17), scratch, need)
    refused("out overlaps the scratch buffer", a, b, normal, depth, p, scratch[need - 16:].view(torch.float32), var, scratch, need)
    refused("out_var overlaps the scratch buffer", a, b, normal, depth, p, out, scratch[need - 16:].view(torch.float32), scratch, need)
    refused("the scratch buffer is too small", a, b, normal, depth, p, out, var, scratch, need - 1)
    refused("not 16-byte aligned", a, b, normal, depth, p, out, var, scratch[4:], need)
    # outputs right behind the scratch buffer are no overlap, and the call is served
    tail = scratch[need:need + 12 * 17 * 33].view(torch.float32).view(33, 17, 3)
    tail_var = scratch[need + 12 * 17 * 33:].view(torch.float32).view(33, 17)
    rc, _ = _device_call(lib, stream, a, b, normal, depth, p, tail, tail_var, scratch, need)
    _abi.check(rc)
    stream.synchronize()
    want = _reference((17, 33), 2, (1.0, 1.0, 1.0))
    assert same(tail.cpu().numpy(), want[0]) and same(tail_var.cpu().numpy(), want[1])


# ---- the render level ----
@pytest.fixture(scope="module")
def cornell(gpu):
    """The small Cornell box with the blob, 64 x 64 at 4 samples per pixel and half: (scene, renderer factory, render_denoised_pair's result)."""
    prims, mk = scenes.config("C2", xres=64, yres=64, spp=4, blob=(24, 12))
    scene = scenes.make_scene(prims)
    return scene, mk, denoise.render_denoised_pair(mk(), scene)


def test_render_denoised_pair_equals_the_restatement_of_its_own_images(cornell):
    scene, mk, out = cornell
    p = denoise.pair_params()
    assert out.rgb.shape == out.a.shape == out.b.shape == out.noisy.shape == out.normal.shape == (64, 64, 3)
    assert out.depth.shape == out.variance.shape == (64, 64)
    want = pr.planes(out.a, out.b, out.normal, out.depth, p.iterations, p.k_color, p.k_normal, p.k_depth, p.var_floor)
    assert same(out.rgb, want[-1][0]) and same(out.variance, want[-1][1]) and same(out.noisy, want[0][0])
    assert not same(out.rgb, out.noisy) and np.isfinite(out.rgb).all() and (out.variance >= 0).all()
    hit = out.depth > 0
    assert 0.5 < hit.mean() and out.normal[hit].max() > 0.9 and out.noisy.max() > 0


def test_render_denoised_pair_renders_the_halves_with_the_two_seeds(cornell):
    scene, mk, out = cornell
    r = mk()
    assert same(out.a, r.render(scene).rgb) and not same(out.b, out.a)
    seed_b = denoise.pair_seed(r.sampler.seed)
    assert seed_b != r.sampler.seed

    def with_seed(seed):
        return core.SamplerRenderer(core.LowDiscrepancySampler(r.camera, r.sampler.samplesPerPixel, seed), r.camera, r.surfaceIntegrator,
                                    r.volumeIntegrator).render(scene).rgb
    assert same(out.b, with_seed(seed_b))
    assert r.sampler.seed == mk().sampler.seed                          # the renderer's own sampler keeps its seed

    def feature(channel):
        return core.SamplerRenderer(r.sampler, r.camera, core.FeatureIntegrator(channel), core.EmissionIntegrator()).render(scene).rgb
    assert same(out.normal, feature("ns")) and same(out.depth, feature("depth")[..., 0])
    other = denoise.render_denoised_pair(r, scene, seed_b=99, normal_channel="ng", iterations=2, sigma_depth=float("inf"), var_floor=0.01)
    assert same(other.a, out.a) and same(other.b, with_seed(99)) and same(other.normal, feature("ng"))
    assert same(other.rgb, pr.denoise_pair(other.a, other.b, other.normal, other.depth, 2, 0.0625, denoise.sharpness(0.1), 0.0, 0.01)[0])


def test_render_denoised_pair_refuses_by_name(cornell):
    scene, mk, out = cornell
    r = mk()

    def renderer(sampler):
        return core.SamplerRenderer(sampler, r.camera, r.surfaceIntegrator, r.volumeIntegrator)
    with pytest.raises(ValueError, match="render_denoised_pair: the adaptive sampler is not supported"):
        denoise.render_denoised_pair(renderer(core.AdaptiveSampler(r.camera, 4, 16, "contrast", 5489)), scene)
    host_buffer = core.HostBufferSampler(r.camera, 1, np.zeros((1, 2), np.int32), np.zeros((1, 5), np.float32))
    with pytest.raises(ValueError, match="render_denoised_pair: HostBufferSampler has no seed to vary"):
        denoise.render_denoised_pair(renderer(host_buffer), scene)
    with pytest.raises(ValueError, match="render_denoised_pair: seed_b equals the sampler's seed"):
        denoise.render_denoised_pair(r, scene, seed_b=r.sampler.seed)


def test_quality_figures_are_finite(cornell):
    """The small-scene figures MEASUREMENTS.md reports: the mean squared error, against a 1024-spp render, of the mean of two 2-spp halves, of
    that pair denoised, and of render_denoised at the same 4 samples per pixel in one render."""
    scene, mk, out = cornell
    prims, mk_ref = scenes.config("C2", xres=64, yres=64, spp=1024, blob=(24, 12))
    ref = mk_ref().render(scene).rgb.astype(np.float64)
    prims, mk_half = scenes.config("C2", xres=64, yres=64, spp=2, blob=(24, 12))
    pair = denoise.render_denoised_pair(mk_half(), scene)
    plain = denoise.render_denoised(mk(), scene)
    figures = [float(((img - ref) ** 2).mean()) for img in (pair.noisy, pair.rgb, plain.noisy, plain.rgb)]
    print("denoise_pair quality, C2-small 64x64 against 1024 spp: mse(mean of 2 + 2 spp) = %.6g, mse(2 + 2 spp, pair filter) = %.6g, "
          "mse(4 spp) = %.6g, mse(4 spp, plain filter) = %.6g" % tuple(figures))
    assert np.isfinite(figures).all()
