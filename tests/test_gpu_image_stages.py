"""The tile walk the four tiled image stages share (dr_image_device.h: img_tiles on the host, img_tile_pixel in k_denoise_level<DnRule>,
k_denoise_level<DnpRule>, k_upsample and k_temporal), at the sizes where it can go wrong: one pixel; one short of a 64 x 4 tile either way;
exactly one tile; one past it, so that a second tile row and column hold a single row and column of pixels; and three tile columns by three
tile rows with a ragged edge.  Every *_device entry runs on a stream of its own on torch tensors and must equal its *_host entry byte for
byte, NaN patterns included; the host entries are held to the numpy restatements by the CPU suites.  The inputs are the seeded ones of the
*_cases.py generators, which every entry accepts.  One process; nothing is started after a failed call: every call's return code raises."""
import ctypes as C

import pytest
import torch

from dartray_amd import _abi

import denoise_cases as dc
import denoise_pair_cases as pc
import denoise_restatement as dr
import temporal_cases as tc
import upsample_cases as uc

pytestmark = pytest.mark.gpu

same = dr.same_bits
SIZES = [(1, 1), (63, 3), (64, 4), (65, 5), (129, 9)]                    # (w, h)
LOW_SIZES = [(32, 2), (33, 3), (65, 5)]                                  # (wl, hl) at factor 2: 64 x 4, 66 x 6 and 130 x 10
LEVELS = [1, 3]
_ids = lambda sizes: ["%dx%d" % s for s in sizes]


def _cuda(arrays):
    t = [torch.from_numpy(a).cuda() if a is not None else None for a in arrays]
    torch.cuda.synchronize()                                             # the uploads, before another stream reads them
    return t


def _with_scratch(call):
    """call(scratch pointer, byref(bytes)) twice: the size query, then the work on a buffer of that size."""
    n = C.c_uint64(0)
    _abi.check(call(None, C.byref(n)))
    scratch = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _abi.check(call(scratch.data_ptr(), C.byref(n)))


@pytest.mark.parametrize("size", SIZES, ids=_ids(SIZES))
def test_denoiser_levels_walk_the_tiles_as_the_host_loop_does(gpu, size):
    lib, stream = gpu.lib(), torch.cuda.Stream()
    imgs = dc.images(*size)
    rgb, normal, depth = _cuda(imgs)
    out = torch.empty_like(rgb)
    for levels in LEVELS:
        p = dc.params(levels, *dc.K_COMBOS[-1])
        out.fill_(-7.0)
        _with_scratch(lambda s, n: lib.dr_denoise_atrous_device(rgb.data_ptr(), normal.data_ptr(), depth.data_ptr(), size[0], size[1], C.byref(p),
                                                                out.data_ptr(), s, n, stream.cuda_stream))
        stream.synchronize()
        assert same(out.cpu().numpy(), dc.host(*imgs, levels, *dc.K_COMBOS[-1])), levels


@pytest.mark.parametrize("size", SIZES, ids=_ids(SIZES))
def test_pair_denoiser_levels_walk_the_tiles_as_the_host_loop_does(gpu, size):
    lib, stream = gpu.lib(), torch.cuda.Stream()
    imgs = pc.images(*size)
    a, b, normal, depth = _cuda(imgs)
    out, var = torch.empty_like(a), torch.empty_like(depth)
    for levels in LEVELS:
        p = pc.params(levels, *pc.K_COMBOS[-1])
        out.fill_(-7.0)
        var.fill_(-7.0)
        _with_scratch(lambda s, n: lib.dr_denoise_pair_device(a.data_ptr(), b.data_ptr(), normal.data_ptr(), depth.data_ptr(), size[0], size[1],
                                                              C.byref(p), out.data_ptr(), var.data_ptr(), s, n, stream.cuda_stream))
        stream.synchronize()
        ref, ref_var = pc.host(*imgs, levels, *pc.K_COMBOS[-1])
        assert same(out.cpu().numpy(), ref) and same(var.cpu().numpy(), ref_var), levels


@pytest.mark.parametrize("low", LOW_SIZES, ids=_ids(LOW_SIZES))
def test_upsampler_walks_the_tiles_as_the_host_loop_does(gpu, low):
    lib, stream = gpu.lib(), torch.cuda.Stream()
    imgs = uc.random_image(*low, 2)
    t = _cuda(imgs)
    out = torch.empty_like(t[3])
    assert tuple(out.shape) == (2 * low[1], 2 * low[0], 3)
    for taps in uc.TAPS:
        p = uc.params(2, taps, *uc.K_COMBOS[-1])
        out.fill_(-7.0)
        _with_scratch(lambda s, n: lib.dr_upsample_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), low[0], low[1], t[3].data_ptr(),
                                                          t[4].data_ptr(), C.byref(p), out.data_ptr(), s, n, stream.cuda_stream))
        stream.synchronize()
        assert same(out.cpu().numpy(), uc.host(*imgs, 2, taps, *uc.K_COMBOS[-1])), taps


@pytest.mark.parametrize("size", SIZES, ids=_ids(SIZES))
def test_temporal_accumulation_walks_the_tiles_as_the_host_loop_does(gpu, size):
    lib, stream = gpu.lib(), torch.cuda.Stream()
    fr, m = tc.frame(*size, "shift"), tc.matrices("shift", *size)
    cur = [fr[k] for k in tc.CURRENT_PLANES]
    p = tc.params(m, *tc.DEFAULTS)
    for history in (None, tc.history_of(fr)):
        t = _cuda(cur + list(history or [None] * 5))
        out = [torch.full_like(t[0], tc.SENTINEL), torch.full_like(t[2], tc.SENTINEL), torch.full_like(t[2], tc.SENTINEL)]
        torch.cuda.synchronize()
        _abi.check(lib.dr_temporal_device(*[x.data_ptr() if x is not None else None for x in t], size[0], size[1], C.byref(p),
                                          *[o.data_ptr() for o in out], stream.cuda_stream))
        stream.synchronize()
        ref = tc.host(*cur, history, m, *tc.DEFAULTS)
        assert all(same(o.cpu().numpy(), r) for o, r in zip(out, ref)), history is not None
