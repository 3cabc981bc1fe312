"""Temporal accumulation with reprojection on the GPU (k_temporal): dr_temporal (host buffers) and dr_temporal_device (torch
tensors, a stream of its own, three frames chained on the device) against dr_temporal_host bit for bit -- the host entry is itself held to
the numpy restatement by tests/test_temporal.py -- and render_sequence on the small Cornell scene against temporal() of its own parts.  One
process; nothing is started after a failed call: every call's return code raises."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dartray_amd import _abi, core, denoise, scenes

import temporal_cases as tc
import temporal_restatement as tr

pytestmark = pytest.mark.gpu

F = np.float32
same = tr.same_bits


def test_host_buffer_entry_equals_the_host_loop_on_every_cpu_case(gpu):
    n = 0
    for key, fr, hist, m, ps in tc.grid():
        rc, out = tc.call(gpu.lib().dr_temporal, fr["rgb"], fr["normal"], fr["depth"], hist, m, *ps)
        _abi.check(rc)
        want = tc.host(fr["rgb"], fr["normal"], fr["depth"], hist, m, *ps)
        assert all(same(a, b) for a, b in zip(out, want)), key
        n += 1
    assert n == 1215


def _device_call(lib, stream, cur, hist, p, out):
    h, w = cur[2].shape
    return lib.dr_temporal_device(*[t.data_ptr() for t in cur], *[t.data_ptr() if t is not None else None for t in hist], w, h, C.byref(p),
                                  *[t.data_ptr() for t in out], stream.cuda_stream)


# 5 x 7: one partial tile; 31 x 9: no multiple of the 64 x 4 tile; 64 x 48: several tiles either way; the strips: 17500 tile rows of a
# single, mostly empty tile column, and 1094 tile columns of one tile row
SEQUENCES = [(5, 7), (31, 9), (64, 48), (1, 70000), (70000, 1)]


@pytest.mark.parametrize("size", SEQUENCES, ids=lambda s: "%dx%d" % s)
def test_device_entry_chains_three_frames_on_its_own_stream(gpu, size):
    lib = gpu.lib()
    w, h = size
    seq = tc.random_sequence(w, h, frames=3)
    stream = torch.cuda.Stream()
    # two sets of outputs: a call writes one while it reads the other as its history
    sets = [[torch.empty((h, w, 3), device="cuda"), torch.empty((h, w), device="cuda"), torch.empty((h, w), device="cuda")] for _ in range(2)]
    frames = [[torch.from_numpy(a).cuda() for a in (rgb, normal, depth)] for rgb, normal, depth, _ in seq]
    torch.cuda.synchronize()                                             # the uploads, before another stream reads them
    ref_hist, dev_hist, lens = None, [None] * 5, []
    for k, (rgb, normal, depth, m) in enumerate(seq):
        out = sets[k % 2]
        for t in out:
            t.fill_(tc.SENTINEL)
        torch.cuda.synchronize()
        _abi.check(_device_call(lib, stream, frames[k], dev_hist, tc.params(m, *tc.DEFAULTS), out))
        stream.synchronize()
        want = tc.host(rgb, normal, depth, ref_hist, m, *tc.DEFAULTS)
        got = [t.cpu().numpy() for t in out]
        assert all(same(a, b) for a, b in zip(got, want)), k
        assert not any((a == tc.SENTINEL).any() for a in got)
        ref_hist = (want[0], want[1], want[2], normal, depth)
        dev_hist = out + frames[k][1:]
        lens.append(want[2])
    if w * h > 1:
        assert (lens[0] <= 1).all() and (lens[1] == 2).any() and (lens[2] == 3).any() and (lens[2] == 1).any()


def test_device_entry_refuses_aliased_buffers(gpu):
    lib = gpu.lib()
    fr, m = tc.frame(5, 7, "shift"), tc.matrices("shift", 5, 7)
    cur = [torch.from_numpy(fr[k]).cuda() for k in tc.CURRENT_PLANES]
    hist = [torch.from_numpy(fr[k]).cuda() for k in tc.HISTORY_PLANES]
    out = [torch.empty((7, 5, 3), device="cuda"), torch.empty((7, 5), device="cuda"), torch.empty((7, 5), device="cuda")]
    stream = torch.cuda.Stream()
    p = tc.params(m, *tc.DEFAULTS)
    torch.cuda.synchronize()
    for bad in ([hist[0], out[1], out[2]], [out[0], hist[1], out[2]], [out[0], out[1], cur[2]]):      # the history updated in place
        assert _device_call(lib, stream, cur, hist, p, bad) == -1 and "an output overlaps an input" in lib.dr_last_error().decode()
    assert _device_call(lib, stream, cur, hist, p, [out[0], out[1], out[1]]) == -1 and "an output overlaps another output" in lib.dr_last_error().decode()
    assert _device_call(lib, stream, cur, hist[:4] + [None], p, out) == -1 and "the history is only partly NULL" in lib.dr_last_error().decode()
    _abi.check(_device_call(lib, stream, cur, hist, p, out))
    stream.synchronize()
    want = tc.host(fr["rgb"], fr["normal"], fr["depth"], tc.history_of(fr), m, *tc.DEFAULTS)
    assert all(same(t.cpu().numpy(), b) for t, b in zip(out, want))


# ---- the render level ----
def _renderer(angle, seed, spp=4, res=64):
    """BASELINE config C1 (the Cornell floor and its emitter, direct lighting) at 64 x 64 from a camera `angle` degrees along its orbit."""
    prims, mk = scenes.config("C1", xres=res, yres=res, spp=spp)
    proto = mk()
    a = math.radians(angle)
    film = core.ImageFilm(res, res, core.BoxFilter(0.5, 0.5))
    cam = core.PerspectiveCamera.lookAt((35.0 * math.sin(a), 0.0, -35.0 * math.cos(a)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, film)
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, spp, seed), cam, proto.surfaceIntegrator, proto.volumeIntegrator)


@pytest.fixture(scope="module")
def scene(gpu):
    return scenes.make_scene(scenes.config("C1")[0])


def _parts_agree(frames):
    history = None
    for k, f in enumerate(frames):
        m = denoise.temporal_matrices(f.camera_, frames[max(k - 1, 0)].camera_)
        for device in (True, False):
            got = denoise.temporal(f.noisy, f.normal, f.depth, history, m, device=device)
            assert same(got.rgb, f.accumulated) and same(got.m2, f.m2) and same(got.len, f.len), (k, device)
        history = f.history


def test_render_sequence_at_one_pose_gives_the_mean_of_two_seeds(scene):
    renderers = [_renderer(0.0, 5489), _renderer(0.0, 77)]
    frames = denoise.render_sequence(renderers, scene)
    assert len(frames) == 2
    for f, r in zip(frames, renderers):
        f.camera_ = r.camera
        assert f.rgb.shape == (64, 64, 3) and f.rgb.dtype == np.float32 and f.len.shape == f.depth.shape == (64, 64) and f.rgb is f.accumulated
    _parts_agree(frames)
    a, b = frames[0].noisy, frames[1].noisy
    assert same(a, renderers[0].render(scene).rgb) and same(frames[0].rgb, a) and not same(a, b)
    valid = np.isfinite(b).all(axis=2) & np.isfinite(frames[1].normal).all(axis=2) & np.isfinite(frames[1].depth) & (frames[1].depth > 0)
    assert valid.any() and not valid.all()
    # every frame's guides are rendered with the first renderer's seed: at one pose they are the same bytes, silhouette pixels included
    assert same(frames[0].normal, frames[1].normal) and same(frames[0].depth, frames[1].depth)
    with np.errstate(all="ignore"):
        rel = np.abs(frames[0].depth - frames[1].depth)[valid] / frames[1].depth[valid]
    mean = a + F(0.5) * (b - a)
    print("temporal, one pose, two seeds: %d current-valid pixels of %d; largest relative depth difference between the seeds' guides %.3g; "
          "%d valid pixels with len != 2, %d whose colour is not a + 0.5 (b - a)"
          % (valid.sum(), valid.size, rel.max(), (frames[1].len[valid] != 2).sum(),
             (mean.view(np.uint32) != frames[1].rgb.view(np.uint32)).any(axis=2)[valid].sum()))
    assert same(frames[1].rgb[valid], mean[valid]) and (frames[1].len[valid] == 2).all()
    assert same(frames[1].rgb[~valid], b[~valid]) and (frames[1].len[~valid] == 1).all()
    assert (frames[1].variance >= 0).all() and (frames[1].variance > 0).any() and (frames[0].variance == 0).all()


def test_render_sequence_over_three_poses_of_a_small_orbit(scene):
    renderers = [_renderer(angle, seed) for angle, seed in ((-2.0, 5489), (0.0, 77), (2.0, 991))]
    frames = denoise.render_sequence(renderers, scene)
    for f, r in zip(frames, renderers):
        f.camera_ = r.camera
        assert all(np.isfinite(a).all() for a in (f.rgb, f.m2, f.len))
    _parts_agree(frames)
    assert (frames[0].len == 1).all() and (frames[1].len == 2).any()
    assert (frames[2].len == 3).any() and (frames[2].len == 1).any() and frames[2].len.max() == 3
    both = denoise.render_sequence(renderers, scene, denoise=True, iterations=2)
    assert same(both[2].accumulated, frames[2].accumulated) and not same(both[2].rgb, frames[2].rgb) and np.isfinite(both[2].rgb).all()
    assert same(both[2].rgb, denoise.atrous(both[2].accumulated, both[2].normal, both[2].depth, iterations=2))


def test_quality_figures_are_finite(scene):
    """The small-scene figures MEASUREMENTS.md reports: the mean squared error, against a 1024-spp render of the last pose, of the last
    frame alone (4 spp) and of the frame accumulated over the three poses of the orbit.  No order between them is asserted."""
    renderers = [_renderer(angle, seed) for angle, seed in ((-2.0, 5489), (0.0, 77), (2.0, 991))]
    frames = denoise.render_sequence(renderers, scene)
    ref = _renderer(2.0, 5489, spp=1024).render(scene).rgb.astype(np.float64)
    alone = float(((frames[2].noisy - ref) ** 2).mean())
    accumulated = float(((frames[2].rgb - ref) ** 2).mean())
    n = frames[2].len
    print("temporal quality, C1 64x64, three poses 2 degrees apart, against 1024 spp: mse(last frame, 4 spp) = %.6g, mse(accumulated) = %.6g; "
          "pixels with history length 1 / 2 / 3: %d / %d / %d" % (alone, accumulated, (n == 1).sum(), ((n > 1) & (n < 3)).sum(), (n == 3).sum()))
    assert np.isfinite(alone) and np.isfinite(accumulated)
