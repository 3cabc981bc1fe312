"""Firefly suppression on the GPU (k_firefly): dr_firefly (host buffers) and dr_firefly_device (torch tensors, a stream of
its own) against dr_firefly_host bit for bit -- the host entry is itself held to the numpy restatement by tests/test_firefly.py -- and the
`firefly` keyword of the four render functions on a small Cornell render against the chain rebuilt from their own parts.  One process,
but for the check of a process that never called dr_init, which is a fresh child; nothing is started after a failed call: every call's
return code raises.

What no test here reaches: a workgroup that walks more than one tile.  The walk takes a second tile only above 2^20 tiles (a 268-million
pixel image), so the barrier discipline of that loop -- every lane reaches both barriers of every iteration -- is checked by reading the
kernel, whose header states it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from dartray_amd import _abi, core, denoise, pbrt, scenes

import firefly_cases as fc
import firefly_restatement as fr
from test_display import decode_png

pytestmark = pytest.mark.gpu

same = fr.same_bits


def test_host_buffer_entry_equals_the_host_loop_on_every_cpu_case(gpu):
    n = 0
    for key, imgs, ps in fc.grid():
        rc, out, removed = fc.call(gpu.lib().dr_firefly, *imgs, ps)
        _abi.check(rc)
        want = fc.host(*imgs, ps)
        assert same(out, want[0]) and same(removed, want[1]), key
        n += 1
    assert n == 875


@pytest.mark.parametrize("size", fc.SIZES, ids=lambda s: "%dx%d" % s)
def test_radius_two_with_outliers_in_a_neighbouring_tiles_halo(gpu, size):
    imgs = fc.halo_image(*size)
    changed = 0
    for rank in fc.RANKS:
        ps = (2, rank, 4.0, 0.0, fc.DEPTH_TOL, fc.NORMAL_TOL)
        rc, out, removed = fc.call(gpu.lib().dr_firefly, *imgs, ps)
        _abi.check(rc)
        want = fc.host(*imgs, ps)
        assert same(out, want[0]) and same(removed, want[1]), rank
        changed += int((removed != 0).sum())
    assert changed > 0 or size == (1, 1)


def _device_call(lib, stream, t, w, h, p, out, removed):
    return lib.dr_firefly_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), w, h, C.byref(p), out.data_ptr(),
                                 removed.data_ptr() if removed is not None else None, stream.cuda_stream)


@pytest.mark.parametrize("size", [(5, 7), (130, 9)], ids=lambda s: "%dx%d" % s)
def test_device_entry_on_its_own_stream_equals_the_host_loop(gpu, size):
    lib, stream = gpu.lib(), torch.cuda.Stream()
    w, h = size
    for kind in fc.KINDS:
        imgs = fc.image(w, h, kind)
        t = [torch.from_numpy(a).cuda() for a in imgs]
        for ps in (fc.DEFAULTS, (2, 3, 1.5, 0.25, fc.DEPTH_TOL, fc.NORMAL_TOL)):
            out, removed = torch.full_like(t[0], fc.SENTINEL), torch.full_like(t[2], fc.SENTINEL)
            alone = torch.full_like(t[0], fc.SENTINEL)
            torch.cuda.synchronize()                                     # the uploads and fills, before another stream reads them
            _abi.check(_device_call(lib, stream, t, w, h, fc.params(*ps), out, removed))
            _abi.check(_device_call(lib, stream, t, w, h, fc.params(*ps), alone, None))
            stream.synchronize()
            want = fc.host(*imgs, ps)
            assert same(out.cpu().numpy(), want[0]) and same(removed.cpu().numpy(), want[1]), (kind, ps)
            assert same(alone.cpu().numpy(), want[0]), (kind, ps)         # a NULL removed changes nothing in out


def test_device_entry_refuses_overlapping_buffers(gpu):
    lib, stream = gpu.lib(), torch.cuda.Stream()
    imgs = fc.image(5, 7, "smooth")
    t = [torch.from_numpy(a).cuda() for a in imgs]
    out, removed = torch.empty((7, 5, 3), device="cuda"), torch.empty((7, 5), device="cuda")
    p = fc.params(*fc.DEFAULTS)
    torch.cuda.synchronize()
    for bad_out, bad_removed in ((t[0], removed), (t[1], removed), (out, t[2]), (out, t[0])):          # in place, or into a guide
        assert _device_call(lib, stream, t, 5, 7, p, bad_out, bad_removed) == -1 and "an output overlaps an input" in lib.dr_last_error().decode()
    assert _device_call(lib, stream, t, 5, 7, p, out, out) == -1 and "an output overlaps another output" in lib.dr_last_error().decode()
    _abi.check(_device_call(lib, stream, t, 5, 7, p, out, removed))
    stream.synchronize()
    want = fc.host(*imgs, fc.DEFAULTS)
    assert same(out.cpu().numpy(), want[0]) and same(removed.cpu().numpy(), want[1])


def test_a_process_that_has_not_called_dr_init_is_refused():
    """A fresh child: it loads the library, never calls dr_init, and hands both launching entries arguments that pass every other check."""
    code = ("import ctypes as C, sys, numpy as np\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from dartray_amd import _abi\n"
            "import firefly_cases as fc\n"
            "lib = _abi.lib()\n"
            "rgb, normal, depth = fc.image(5, 7, 'smooth')\n"
            "rc, out, removed = fc.call(lib.dr_firefly, rgb, normal, depth, fc.DEFAULTS)\n"
            "print('host-buffer', rc, lib.dr_last_error().decode())\n"
            "p = fc.params(*fc.DEFAULTS)\n"
            "rc = lib.dr_firefly_device(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, 5, 7, C.byref(p), out.ctypes.data, None, None)\n"
            "print('device', rc, lib.dr_last_error().decode())\n"
            "print('untouched', bool((out == fc.SENTINEL).all()))\n" % (ROOT, os.path.join(ROOT, "tests")))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "host-buffer -3 dr_firefly: called before dr_init" in res.stdout, res.stdout
    assert "device -3 dr_firefly_device: called before dr_init" in res.stdout, res.stdout
    assert "untouched True" in res.stdout, res.stdout


# ---- the render level: a small Cornell render (the path-traced box of config C2 around a 24 x 12 blob) at 64 x 64 and 2 spp ----
BLOB = (24, 12)


def _renderer(seed, spp=2, res=64):
    prims, mk = scenes.config("C2", xres=res, yres=res, spp=spp, blob=BLOB)
    proto = mk()
    cam = proto.camera
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, spp, seed), cam, proto.surfaceIntegrator, proto.volumeIntegrator)


@pytest.fixture(scope="module")
def scene(gpu):
    return scenes.make_scene(scenes.config("C2", xres=64, yres=64, spp=2, blob=BLOB)[0])


def test_render_denoised_with_the_stage_equals_the_chain_of_its_parts(scene):
    r = _renderer(5489)
    got = denoise.render_denoised(r, scene, firefly=True, iterations=3)
    clamped, removed = denoise.firefly(got.noisy, got.normal, got.depth, return_removed=True)
    assert same(got.noisy, r.render(scene).rgb) and same(got.removed, removed)
    assert same(got.rgb, denoise.atrous(clamped, got.normal, got.depth, iterations=3))
    print("firefly on C2 64x64 at 2 spp: %d of %d pixels clamped" % ((removed != 0).sum(), removed.size))
    assert (removed != 0).any() and not same(clamped, got.noisy)
    # a dict of parameters reaches the stage
    tight = denoise.render_denoised(r, scene, firefly=dict(radius=2, rank=3, threshold=1.5), iterations=3)
    want = denoise.firefly(tight.noisy, tight.normal, tight.depth, radius=2, rank=3, threshold=1.5, return_removed=True)
    assert same(tight.removed, want[1]) and same(tight.rgb, denoise.atrous(want[0], tight.normal, tight.depth, iterations=3))
    assert not same(tight.removed, got.removed)
    # and the default leaves every byte as it was
    off, plain = denoise.render_denoised(r, scene, firefly=False, iterations=3), denoise.render_denoised(r, scene, iterations=3)
    assert same(off.rgb, plain.rgb) and same(plain.rgb, denoise.atrous(plain.noisy, plain.normal, plain.depth, iterations=3))
    assert not hasattr(plain, "removed") and not hasattr(off, "removed") and not same(plain.rgb, got.rgb)


def test_render_denoised_pair_and_render_upsampled_clamp_ahead_of_their_stage(scene):
    r = _renderer(5489)
    got = denoise.render_denoised_pair(r, scene, firefly=True, iterations=3)
    a, ra = denoise.firefly(got.a, got.normal, got.depth, return_removed=True)
    b, rb = denoise.firefly(got.b, got.normal, got.depth, return_removed=True)
    assert same(got.removed[0], ra) and same(got.removed[1], rb) and (ra != 0).any() and (rb != 0).any()
    assert same(got.rgb, denoise.atrous_pair(a, b, got.normal, got.depth, iterations=3))
    plain, off = denoise.render_denoised_pair(r, scene, iterations=3), denoise.render_denoised_pair(r, scene, firefly=False, iterations=3)
    assert same(plain.rgb, off.rgb) and same(plain.a, got.a) and same(plain.b, got.b) and not same(plain.rgb, got.rgb)
    low = _renderer(5489, res=32)
    up = denoise.render_upsampled(low, r, scene, firefly=True)
    clamped, removed = denoise.firefly(up.low, up.normal_lo, up.depth_lo, return_removed=True)
    assert removed.shape == (32, 32) and same(up.removed, removed) and (removed != 0).any()
    assert same(up.rgb, denoise.upsample(clamped, up.normal_lo, up.depth_lo, up.normal, up.depth, factor=2))
    plain, off = denoise.render_upsampled(low, r, scene), denoise.render_upsampled(low, r, scene, firefly=False)
    assert same(plain.rgb, off.rgb) and same(plain.low, up.low) and not same(plain.rgb, up.rgb)


def test_render_sequence_clamps_each_frame_before_it_enters_the_history(scene):
    renderers = [_renderer(seed) for seed in (5489, 77, 991)]           # three static frames
    frames = denoise.render_sequence(renderers, scene, firefly=True)
    mats = denoise.temporal_matrices(renderers[0].camera, renderers[0].camera)
    history, any_removed = None, False
    for k, f in enumerate(frames):
        clamped, removed = denoise.firefly(f.noisy, f.normal, f.depth, return_removed=True)
        history = denoise.temporal(clamped, f.normal, f.depth, history, mats)
        assert same(f.removed, removed) and same(f.accumulated, history.rgb) and same(f.m2, history.m2) and same(f.len, history.len), k
        any_removed = any_removed or bool((removed != 0).any())
    assert any_removed and (frames[2].len == 3).any()
    plain, off = denoise.render_sequence(renderers, scene), denoise.render_sequence(renderers, scene, firefly=False)
    assert all(same(p.rgb, o.rgb) and same(p.m2, o.m2) for p, o in zip(plain, off)) and not hasattr(plain[0], "removed")
    assert all(same(p.noisy, f.noisy) for p, f in zip(plain, frames)) and not same(plain[2].m2, frames[2].m2)
    both = denoise.render_sequence(renderers, scene, firefly=True, denoise="moments", iterations=2)
    assert same(both[2].accumulated, frames[2].accumulated)
    assert same(both[2].rgb, denoise.atrous_moments(both[2].history, iterations=2))


def test_the_command_line_with_the_stage_writes_a_png(gpu, tmp_path):
    scene = tmp_path / "tiny.pbrt"
    scene.write_text('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\nSampler "lowdiscrepancy" "integer pixelsamples" [4]\n'
                     'Film "image" "integer xresolution" [24] "integer yresolution" [16]\nSurfaceIntegrator "directlighting"\nWorldBegin\n'
                     'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [8 8 8]\nTranslate 0 3 0\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                     '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nAttributeEnd\n'
                     'Material "matte" "rgb Kd" [0.6 0.4 0.2]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                     '"point P" [-2 -1 -2  2 -1 -2  2 -1 2  -2 -1 2]\nWorldEnd\n')
    png, npy, plain = str(tmp_path / "o.png"), str(tmp_path / "o.npy"), str(tmp_path / "p.npy")
    assert pbrt.main([str(scene), "--firefly", "-o", npy]) == 0 and pbrt.main([str(scene), "-o", plain]) == 0
    api = pbrt.load(str(scene), render=False)
    want = denoise.render_firefly(api.rendererObject, api.scene)
    assert same(np.load(plain), want.noisy) and same(np.load(npy), want.rgb) and want.removed.shape == (16, 24)
    assert pbrt.main([str(scene), "--firefly", "-o", png]) == 0
    from dartray_amd import display
    assert decode_png(png).shape == (16, 24, 4) and same(decode_png(png), display.tonemap(want.rgb, device=False))
    assert pbrt.main([str(scene), "--firefly", "--upsample", "2", "-o", png]) == 0 and decode_png(png).shape == (16, 24, 4)
