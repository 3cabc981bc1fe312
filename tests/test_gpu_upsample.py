"""The joint bilateral upsampler on the GPU (k_image_pack<DnInputs> / k_upsample): dr_upsample (host buffers) and dr_upsample_device
(torch tensors, a stream of its own) against dr_upsample_host bit for bit -- the host entry is itself held to the numpy restatement by
tests/test_upsample.py -- and render_upsampled on the small Cornell scene against upsample() and atrous() of its own parts.  The host result
of a case is computed once and shared.  One process; nothing is started after a failed call: every call's return code raises."""
import ctypes as C

import numpy as np
import pytest
import torch

from dartray_amd import _abi, core, denoise, scenes

import upsample_cases as uc
import upsample_restatement as ur

pytestmark = pytest.mark.gpu

same = ur.same_bits
_host = {}


def _small_cases():
    """The CPU suite's cases: (key, images, factor, taps, k_normal, k_depth)."""
    for size, f, taps, invalid in uc.grid():
        imgs = uc.images(*size, f, invalid=invalid)
        for k in uc.K_COMBOS:
            yield (size, f, taps, invalid, k), imgs, f, taps, k[0], k[1]
    imgs, (f, taps, kn, kz) = uc.overflow_case()
    yield "overflow", imgs, f, taps, kn, kz
    for taps in uc.TAPS:
        for kz in (0.0, 1.0):
            args, _ = uc.step_case(taps, kz)
            yield ("step", taps, kz), args[:5], *args[5:]


def _reference(key, imgs, f, taps, kn, kz):
    if key not in _host:
        _host[key] = uc.host(*imgs, f, taps, kn, kz)
    return _host[key]


def test_host_buffer_entry_equals_the_host_loop_on_every_cpu_case(gpu):
    n = 0
    for key, imgs, f, taps, kn, kz in _small_cases():
        rc, out = uc.call(gpu.lib().dr_upsample, *imgs, f, taps, kn, kz)
        _abi.check(rc)
        assert same(out, _reference(key, imgs, f, taps, kn, kz)), key
        n += 1
    assert n > 400


# 64 x 48 -> 256 x 192: several tiles either way; 31 x 9 -> 62 x 18: no multiple of the 64 x 4 tile; the strips, 4 x 280000 and 280000 x 4:
# 70000 tile rows of a single, mostly empty tile column, and 4375 tile columns of one tile row
LARGE = [((64, 48), 4), ((31, 9), 2), ((1, 70000), 4), ((70000, 1), 4)]


@pytest.mark.parametrize("size,f", LARGE, ids=["%dx%dx%d" % (s + (f,)) for s, f in LARGE])
def test_host_buffer_entry_equals_the_host_loop_on_larger_images(gpu, size, f):
    imgs = uc.random_image(*size, f)
    for taps in uc.TAPS:
        for k in (uc.K_COMBOS[0], uc.K_COMBOS[-1]):
            rc, out = uc.call(gpu.lib().dr_upsample, *imgs, f, taps, *k)
            _abi.check(rc)
            assert same(out, _reference(("large", size, f, taps, k), imgs, f, taps, *k)), (taps, k)


def _device_call(lib, stream, t, p, out, scratch, nbytes):
    rgb_lo, normal_lo, depth_lo, normal, depth = t
    n = C.c_uint64(nbytes)
    return lib.dr_upsample_device(rgb_lo.data_ptr(), normal_lo.data_ptr(), depth_lo.data_ptr(), depth_lo.shape[1], depth_lo.shape[0],
                                  normal.data_ptr(), depth.data_ptr(), C.byref(p), out.data_ptr(), scratch.data_ptr() if scratch is not None else None,
                                  C.byref(n), stream.cuda_stream), n.value


@pytest.mark.parametrize("size,f", [((5, 7), 2), ((64, 48), 4)], ids=["5x7x2", "64x48x4"])
def test_device_entry_on_its_own_stream_equals_the_host_loop(gpu, size, f):
    lib = gpu.lib()
    imgs = uc.random_image(*size, f)
    t = [torch.from_numpy(a).cuda() for a in imgs]
    out = torch.empty_like(t[3])
    stream = torch.cuda.Stream()
    rc, need = _device_call(lib, stream, t, uc.params(f, 2, 1.0, 1.0), out, None, 0)        # the size query answers first, and touches nothing
    _abi.check(rc)
    assert need == 32 * size[0] * size[1]
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                            # the uploads, before another stream reads them
    for taps in uc.TAPS:
        for k in (uc.K_COMBOS[0], uc.K_COMBOS[-1]):
            out.fill_(-7.0)
            torch.cuda.synchronize()
            rc, _ = _device_call(lib, stream, t, uc.params(f, taps, *k), out, scratch, need)
            _abi.check(rc)
            stream.synchronize()
            assert same(out.cpu().numpy(), _reference(("large", size, f, taps, k), imgs, f, taps, *k)), (taps, k)


def test_device_entry_refuses_aliased_short_and_misaligned_buffers(gpu):
    lib = gpu.lib()
    imgs = uc.images(5, 7, 2)
    t = [torch.from_numpy(a).cuda() for a in imgs]
    out = torch.empty_like(t[3])
    need = 32 * 5 * 7
    scratch = torch.empty(need + 12 * 10 * 14, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    p = uc.params(2, 2, 1.0, 1.0)
    torch.cuda.synchronize()

    def refused(needle, out, scratch, nbytes):
        rc, _ = _device_call(lib, stream, t, p, out, scratch, nbytes)
        assert rc == -1 and needle in lib.dr_last_error().decode(), (needle, rc, lib.dr_last_error())

    refused("out overlaps an input", t[3], scratch, need)
    refused("out overlaps an input", t[0], scratch, need)
    refused("out overlaps the scratch buffer", scratch[need - 16:].view(torch.float32), scratch, need)
    refused("the scratch buffer is too small", out, scratch, need - 1)
    refused("not 16-byte aligned", out, scratch[4:], need)
    # an output right behind the scratch buffer is no overlap, and the call is served
    tail = scratch[need:].view(torch.float32).view(14, 10, 3)
    rc, _ = _device_call(lib, stream, t, p, tail, scratch, need)
    _abi.check(rc)
    stream.synchronize()
    assert same(tail.cpu().numpy(), uc.host(*imgs, 2, 2, 1.0, 1.0))


# ---- the render level ----
def _renderers(**full_kw):
    """BASELINE config C1 (the Cornell floor and its emitter, direct lighting) at 16 x 16 and 32 x 32, 4 samples per pixel."""
    prims, low = scenes.config("C1", xres=16, yres=16, spp=4)
    _, full = scenes.config("C1", xres=32, yres=32, spp=4, **full_kw)
    return prims, low(), full()


@pytest.fixture(scope="module")
def cornell(gpu):
    prims, low, full = _renderers()
    scene = scenes.make_scene(prims)
    return scene, low, full, denoise.render_upsampled(low, full, scene)


def test_render_upsampled_equals_upsample_of_its_own_parts(cornell):
    scene, low, full, out = cornell
    assert (out.width, out.height, out.xOffset, out.yOffset) == (32, 32, 0, 0)
    assert out.rgb.shape == out.normal.shape == (32, 32, 3) and out.depth.shape == (32, 32) and out.rgb.dtype == np.float32
    assert out.low.shape == out.normal_lo.shape == (16, 16, 3) and out.depth_lo.shape == (16, 16)
    assert np.isfinite(out.rgb).all() and out.rgb.max() > 0
    assert same(out.rgb, denoise.upsample(out.low, out.normal_lo, out.depth_lo, out.normal, out.depth))
    assert same(out.rgb, denoise.upsample(out.low, out.normal_lo, out.depth_lo, out.normal, out.depth, factor=2, taps=2, device=False))
    p = denoise.upsample_params(2)
    assert same(out.rgb, ur.upsample(out.low, out.normal_lo, out.depth_lo, out.normal, out.depth, 2, 2, p.k_normal, p.k_depth))
    # the parts are the renders of the renderers it was given: the low beauty image, and first-hit guides of either size
    assert same(out.low, low.render(scene).rgb)

    def feature(r, channel):
        return core.SamplerRenderer(r.sampler, r.camera, core.FeatureIntegrator(channel), core.EmissionIntegrator()).render(scene).rgb
    assert same(out.normal, feature(full, "ns")) and same(out.depth_lo, feature(low, "depth")[..., 0])
    hit = out.depth > 0
    assert hit.any() and not hit.all() and (out.normal[hit] > 0).any() and (out.normal[~hit] == 0).all()


def test_render_upsampled_with_denoise_equals_atrous_of_the_upsampled_image(cornell):
    scene, low, full, out = cornell
    both = denoise.render_upsampled(low, full, scene, taps=4, denoise=True, iterations=2, sigma_depth=2.0)
    up = denoise.upsample(both.low, both.normal_lo, both.depth_lo, both.normal, both.depth, taps=4, sigma_depth=2.0)
    assert same(both.low, out.low) and same(both.normal, out.normal) and same(both.upsampled, up) and not same(up, out.rgb)
    assert same(both.rgb, denoise.atrous(up, both.normal, both.depth, iterations=2, sigma_depth=2.0))
    assert both.rgb.shape == (32, 32, 3) and np.isfinite(both.rgb).all() and not same(both.rgb, up)


def test_render_upsampled_by_four(gpu):
    prims, low = scenes.config("C1", xres=8, yres=8, spp=4)
    _, full = scenes.config("C1", xres=32, yres=32, spp=4)
    out = denoise.render_upsampled(low(), full(), scenes.make_scene(prims), normal_channel="ng")
    assert out.rgb.shape == (32, 32, 3) and out.low.shape == (8, 8, 3) and np.isfinite(out.rgb).all()
    assert same(out.rgb, denoise.upsample(out.low, out.normal_lo, out.depth_lo, out.normal, out.depth, factor=4, device=False))


def test_the_command_line_renders_at_half_the_resolution_and_upsamples(gpu, tmp_path):
    from dartray_amd import pbrt
    scene = tmp_path / "tiny.pbrt"
    scene.write_text(uc.TINY_PBRT)
    npy = str(tmp_path / "o.npy")
    assert pbrt.main([str(scene), "-o", npy, "--upsample", "2"]) == 0
    rgb = np.load(npy)
    assert rgb.shape == (16, 24, 3) and rgb.dtype == np.float32 and np.isfinite(rgb).all() and rgb.max() > 0
    api = pbrt.load(str(scene), upsample=2)
    assert same(rgb, denoise.render_upsampled(api.lowRendererObject, api.rendererObject, api.scene).rgb)


def test_render_upsampled_refusals(cornell):
    scene, low, full, _ = cornell
    prims, mk = scenes.config("C1", xres=48, yres=48, spp=4)
    with pytest.raises(ValueError, match=r"full_renderer's film must be exactly 2 or 4 times low_renderer's in both axes \(got 48 x 48 for 16 x 16\)"):
        denoise.render_upsampled(low, mk(), scene)
    cam = full.camera
    adaptive = core.SamplerRenderer(core.AdaptiveSampler(cam, 4, 16, "contrast", 5489), cam, full.surfaceIntegrator, core.EmissionIntegrator())
    with pytest.raises(ValueError, match=r"render_upsampled: the adaptive sampler is not supported \(full_renderer"):
        denoise.render_upsampled(low, adaptive, scene)
    _, _, split = _renderers(tileCount=2)
    with pytest.raises(ValueError, match=r"render_upsampled: tileCount > 1 is not supported \(full_renderer has tileCount 2\)"):
        denoise.render_upsampled(low, split, scene)
