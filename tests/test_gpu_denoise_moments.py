"""The variance-guided a-trous denoiser over a temporal history on the GPU (k_image_pack<DnmInputs> / k_moments_variance /
k_denoise_level<DnmRule>): dr_denoise_moments (host buffers) and dr_denoise_moments_device (torch tensors, a stream of its own) against
dr_denoise_moments_host bit for bit, in colour, variance and first estimate -- the host entry is itself held to the numpy restatement by
tests/test_denoise_moments.py -- and render_sequence(denoise="moments") on the small scene of tests/test_gpu_temporal.py against
atrous_moments on the host.  One process; nothing is started after a failed call: every call's return code raises."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dartray_amd import _abi, core, denoise, scenes

import denoise_moments_cases as mc
import denoise_moments_restatement as mr

pytestmark = pytest.mark.gpu

same = mr.same_bits
# the big image: the long and the short estimate, one and five levels, and a poisoned input
BIG_CASES = [(None, mc.PARAMS[0]), (None, (5, 0.0625, 40.0, 0.3, mc.VAR_FLOOR, 4, 3)), ("len", (5, 0.0625, 40.0, 0.3, mc.VAR_FLOOR, 8, 2))]


def _big():
    for poison, prm in BIG_CASES:
        yield (mc.BIG, poison, prm), mc.images(*mc.BIG, min_history=prm[5], poison=poison), prm


@pytest.mark.parametrize("size", mc.SIZES + [mc.BIG], ids=lambda s: "%dx%d" % s)
def test_host_buffer_entry_equals_the_host_loop_bit_for_bit(gpu, size):
    n = 0
    for key, images, prm in (_big() if size == mc.BIG else mc.grid([size])):
        rc, out, var, var0 = mc.call(gpu.lib().dr_denoise_moments, *images, prm)
        _abi.check(rc)
        want = mc.host(*images, prm)
        assert same(out, want[0]) and same(var, want[1]) and same(var0, want[2]), key
        assert not (out == -7).all() and not (var == -7).any() and not (var0 == -7).any()
        n += 1
    assert n == (len(BIG_CASES) if size == mc.BIG else len(mc.POISON) * len(mc.PARAMS))


def _device_call(lib, stream, images, p, out, var, var0, scratch, nbytes):
    n = C.c_uint64(nbytes)
    h, w = images[4].shape
    return lib.dr_denoise_moments_device(*[t.data_ptr() for t in images], w, h, C.byref(p), out.data_ptr(),
                                         var.data_ptr() if var is not None else None, var0.data_ptr() if var0 is not None else None,
                                         scratch.data_ptr() if scratch is not None else None, C.byref(n), stream.cuda_stream), n.value


@pytest.mark.parametrize("size", [(3, 5), (67, 9), (130, 7), mc.BIG], ids=lambda s: "%dx%d" % s)
def test_device_entry_on_its_own_stream_equals_the_host_loop_bit_for_bit(gpu, size):
    lib = gpu.lib()
    w, h = size
    prm = (5, 0.0625, 40.0, 0.3, mc.VAR_FLOOR, 4, 3)
    host_images = mc.images(*size)
    want = mc.host(*host_images, prm)
    images = [torch.from_numpy(x).cuda() for x in host_images]
    out, var, var0 = torch.empty_like(images[0]), torch.empty_like(images[4]), torch.empty_like(images[4])
    stream = torch.cuda.Stream()
    # the size query answers first, and touches nothing
    rc, need = _device_call(lib, stream, images, mc.params(*prm), out, var, var0, None, 0)
    _abi.check(rc)
    assert need == 48 * w * h
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                            # the uploads, before another stream reads them
    for with_var, with_var0 in ((True, True), (False, True), (True, False), (False, False)):
        for t in (out, var, var0):
            t.fill_(-7.0)
        torch.cuda.synchronize()
        rc, _ = _device_call(lib, stream, images, mc.params(*prm), out, var if with_var else None, var0 if with_var0 else None, scratch, need)
        _abi.check(rc)
        stream.synchronize()
        assert same(out.cpu().numpy(), want[0]), (with_var, with_var0)
        assert same(var.cpu().numpy(), want[1]) if with_var else bool((var == -7.0).all())
        assert same(var0.cpu().numpy(), want[2]) if with_var0 else bool((var0 == -7.0).all())


def test_device_entry_refuses_aliased_and_short_buffers(gpu):
    lib = gpu.lib()
    w, h = 67, 9
    prm = (2, 1.0, 1.0, 1.0, mc.VAR_FLOOR, 4, 3)
    host_images = mc.images(w, h)
    images = [torch.from_numpy(x).cuda() for x in host_images]
    rgb, m2, length, normal, depth = images
    out, var, var0 = torch.empty_like(rgb), torch.empty_like(depth), torch.empty_like(depth)
    need = 48 * w * h
    scratch = torch.empty(need + 20 * w * h, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    p = mc.params(*prm)
    torch.cuda.synchronize()

    def refused(needle, *args):
        rc, _ = _device_call(lib, stream, images, p, *args)
        assert rc == -1 and needle in lib.dr_last_error().decode(), (needle, rc, lib.dr_last_error())

    refused("out overlaps an input", rgb, var, var0, scratch, need)
    refused("out overlaps an input", normal, var, var0, scratch, need)
    refused("out_var overlaps an input", out, m2, var0, scratch, need)
    refused("out_var overlaps an input", out, depth, var0, scratch, need)
    refused("out_var0 overlaps an input", out, var, length, scratch, need)
    refused("out_var0 overlaps an input", out, var, rgb.view(-1)[:w * h].view(h, w), scratch, need)
    refused("out overlaps out_var", out, out.view(-1)[5:5 + w * h].view(h, w), var0, scratch, need)
    refused("out overlaps out_var0", out, var, out.view(-1)[5:5 + w * h].view(h, w), scratch, need)
    refused("out_var overlaps out_var0", out, var, var, scratch, need)
    refused("out overlaps the scratch buffer", scratch[need - 16:].view(torch.float32), var, var0, scratch, need)
    refused("out_var overlaps the scratch buffer", out, scratch[need - 16:].view(torch.float32), var0, scratch, need)
    refused("out_var0 overlaps the scratch buffer", out, var, scratch[need - 16:].view(torch.float32), scratch, need)
    refused("the scratch buffer is too small", out, var, var0, scratch, need - 1)
    refused("not 16-byte aligned", out, var, var0, scratch[4:], need)
    # outputs right behind the scratch buffer are no overlap, and the call is served
    n = w * h
    tail = scratch[need:need + 12 * n].view(torch.float32).view(h, w, 3)
    tail_var = scratch[need + 12 * n:need + 16 * n].view(torch.float32).view(h, w)
    tail_var0 = scratch[need + 16 * n:].view(torch.float32).view(h, w)
    rc, _ = _device_call(lib, stream, images, p, tail, tail_var, tail_var0, scratch, need)
    _abi.check(rc)
    stream.synchronize()
    want = mc.host(*host_images, prm)
    assert same(tail.cpu().numpy(), want[0]) and same(tail_var.cpu().numpy(), want[1]) and same(tail_var0.cpu().numpy(), want[2])


def test_the_module_on_the_device_equals_the_host(gpu):
    frame = denoise.TemporalFrame(*mc.images(130, 7))
    want = denoise.atrous_moments(frame, device=False, return_variance=True, return_estimate=True)
    got = denoise.atrous_moments(frame, return_variance=True, return_estimate=True)
    assert all(same(a, b) for a, b in zip(got, want))
    assert same(denoise.atrous_moments(frame, iterations=2, radius=1, min_history=8),
                denoise.atrous_moments(frame, iterations=2, radius=1, min_history=8, device=False))


# ---- the render level ----
def _renderer(angle, seed, spp=4, res=16):
    """BASELINE config C1 (the Cornell floor and its emitter, direct lighting) at 16 x 16 from a camera `angle` degrees along its orbit: the
    small scene of tests/test_gpu_temporal.py."""
    prims, mk = scenes.config("C1", xres=res, yres=res, spp=spp)
    proto = mk()
    a = math.radians(angle)
    film = core.ImageFilm(res, res, core.BoxFilter(0.5, 0.5))
    cam = core.PerspectiveCamera.lookAt((35.0 * math.sin(a), 0.0, -35.0 * math.cos(a)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, film)
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, spp, seed), cam, proto.surfaceIntegrator, proto.volumeIntegrator)


def test_render_sequence_with_the_moments_filter_over_three_frames(gpu):
    scene = scenes.make_scene(scenes.config("C1")[0])
    renderers = [_renderer(angle, seed) for angle, seed in ((-2.0, 5489), (0.0, 77), (2.0, 991))]
    plain = denoise.render_sequence(renderers, scene)
    frames = denoise.render_sequence(renderers, scene, denoise="moments", min_history=2, iterations=3)
    assert len(frames) == len(plain) == 3
    for f, g in zip(frames, plain):
        assert f.rgb.shape == (16, 16, 3) and f.filtered_variance.shape == (16, 16) and not hasattr(g, "filtered_variance")
        assert same(f.accumulated, g.accumulated) and same(f.m2, g.m2) and same(f.len, g.len) and same(f.accumulated, f.history.rgb)
        rgb, var = denoise.atrous_moments(f.history, min_history=2, iterations=3, device=False, return_variance=True)
        assert same(f.rgb, rgb) and same(f.filtered_variance, var)
    assert not same(frames[2].rgb, frames[2].accumulated) and np.isfinite(frames[2].rgb).all()
    assert (frames[2].len >= 2).any() and (frames[2].len == 1).any()     # both estimates are exercised in the last frame
    defaults = denoise.render_sequence(renderers, scene, denoise="moments")
    assert same(defaults[2].rgb, denoise.atrous_moments(defaults[2].history, device=False)) and not same(defaults[2].rgb, frames[2].rgb)
