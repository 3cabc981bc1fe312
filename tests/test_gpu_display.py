"""The display transform on the GPU (k_display_hist / k_display_pick / k_display_encode): dr_display (host buffers) and
dr_display_device (torch tensors, a stream of its own) against dr_display_host byte for byte -- the host entry is itself held to the numpy
restatement by tests/test_display.py --, the histogram and the scale of dr_display_exposure against the host's, the worst-case images, and the
render leg: a small BASELINE scene through display.to_image and through the command line into a PNG.  The host result of a case is computed
once and shared.  Nothing is started after a failed call: every call's return code raises."""
import ctypes as C

import numpy as np
import pytest
import torch

from dartray_amd import _abi, display, pbrt, scenes

import display_cases as dc
import display_restatement as dr
from test_display import decode_png

pytestmark = pytest.mark.gpu

same = dr.same_bytes
# 1 x 1; 67 x 5 and 257 x 3: no multiple of a wave or a workgroup; 1031 x 1021: more pixels than one pass of either grid (1024 and 2048
# workgroups of 256), so the grid stride and the merge of many workgroups' bins are exercised
SHAPES = [(1, 1), (67, 5), (257, 3), (1031, 1021)]
_IDS = ["%dx%d" % s for s in SHAPES]
NEED = 2048 * 4 + 16
_host = {}


def _params(combo):
    curve, encode, (auto, permille, exposure, iw) = combo
    return dc.params(curve, encode, auto, permille, exposure, iw)


def _reference(key, img, combo):
    if (key, combo) not in _host:
        _host[(key, combo)] = dc.host(img, _params(combo))
    return _host[(key, combo)]


def _combos(size):
    """Every curve x encode x exposure mode; at the large shape one automatic and one manual exposure instead of two of each."""
    return dc.COMBOS if size[0] * size[1] <= 4096 else [c for c in dc.COMBOS if c[2] in (dc.EXPOSURES[1], dc.EXPOSURES[3])]


def _device_call(lib, stream, rgb, p, out, scratch, nbytes):
    n = C.c_uint64(nbytes)
    h, w = rgb.shape[:2]
    return lib.dr_display_device(rgb.data_ptr(), w, h, C.byref(p), out.data_ptr(), scratch.data_ptr() if scratch is not None else None,
                                 C.byref(n), stream.cuda_stream), n.value


@pytest.mark.parametrize("size", SHAPES, ids=_IDS)
def test_host_buffer_entry_equals_the_host_loop_byte_for_byte(gpu, size):
    img = dc.images(*size)
    for combo in _combos(size):
        rc, out = dc.call(gpu.lib().dr_display, img, _params(combo))
        _abi.check(rc)
        assert same(out, _reference(size, img, combo)), combo


@pytest.mark.parametrize("size", SHAPES, ids=_IDS)
def test_device_entry_on_its_own_stream_equals_the_host_loop_byte_for_byte(gpu, size):
    lib = gpu.lib()
    w, h = size
    img = dc.images(*size)
    rgb = torch.from_numpy(img).cuda()
    out = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    rc, need = _device_call(lib, stream, rgb, _params(dc.COMBOS[0]), out, None, 0)     # the size query answers first, and touches nothing
    _abi.check(rc)
    assert need == NEED
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                            # the upload, before another stream reads it
    for combo in _combos(size):
        out.fill_(7)
        scratch.fill_(0xA5)                                             # stale counts and a stale scale: the call clears what it reads
        torch.cuda.synchronize()
        rc, _ = _device_call(lib, stream, rgb, _params(combo), out, scratch, need)
        _abi.check(rc)
        stream.synchronize()
        assert same(out.cpu().numpy(), _reference(size, img, combo)), combo
        if not combo[2][0]:                                             # manual exposure: the first two kernels do not run
            assert (scratch == 0xA5).all()


@pytest.mark.parametrize("name", sorted(dc.WORST))
@pytest.mark.parametrize("size", [(67, 5), (1031, 1021)], ids=["67x5", "1031x1021"])
def test_worst_case_images(gpu, size, name):
    """One luminance everywhere (a single bin takes every atomic), no valid pixel (n == 0), one valid pixel among invalid ones, and a ramp that
    occupies every normal bin."""
    lib = gpu.lib()
    img = dc.WORST[name](*size)
    p = dc.params(1, 0, 1, 500)
    rc, bits, hist = dc.exposure(lib.dr_display_exposure, img, p)
    _abi.check(rc)
    rc, host_bits, host_hist = dc.exposure(lib.dr_display_exposure_host, img, p)
    _abi.check(rc)
    assert same(hist, host_hist) and bits == host_bits
    n = size[0] * size[1]
    want = {"flat": n, "all_invalid": 0, "one_valid": 1, "ramp": n}[name]
    assert int(hist.sum()) == want and (name != "ramp" or n < 2032 or (hist[8:2040] >= 1).all())
    for combo in dc.COMBOS[::7]:
        rc, out = dc.call(lib.dr_display, img, _params(combo))
        _abi.check(rc)
        assert same(out, _reference((name, size), img, combo)), combo


@pytest.mark.parametrize("size", SHAPES, ids=_IDS)
def test_histogram_and_scale_equal_the_hosts(gpu, size):
    lib = gpu.lib()
    img = dc.images(*size)
    for permille in (0, 500, 731, 1000):
        p = dc.params(0, 0, 1, permille, key=0.5)
        rc, bits, hist = dc.exposure(lib.dr_display_exposure, img, p)
        _abi.check(rc)
        rc, host_bits, host_hist = dc.exposure(lib.dr_display_exposure_host, img, p)
        _abi.check(rc)
        assert same(hist, host_hist) and bits == host_bits, permille
    rc, bits, none = dc.exposure(lib.dr_display_exposure, img, p, want_hist=False)
    _abi.check(rc)
    assert none is None and bits == host_bits
    if size[0] * size[1] <= 4096:
        assert same(hist, dr.histogram(img))


def test_device_entry_refuses_aliased_and_short_buffers(gpu):
    lib = gpu.lib()
    rgb = torch.from_numpy(dc.images(17, 33)).cuda()
    out = torch.empty((33, 17, 4), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(NEED + 4 * 17 * 33, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    p = _params(dc.COMBOS[0])
    torch.cuda.synchronize()

    def refused(needle, *args):
        rc, _ = _device_call(lib, stream, *args)
        assert rc == -1 and needle in lib.dr_last_error().decode(), (needle, rc, lib.dr_last_error())

    refused("out overlaps an input", rgb, p, rgb.view(torch.uint8), scratch, NEED)
    refused("out overlaps the scratch buffer", rgb, p, scratch[NEED - 4:], scratch, NEED)
    refused("the scratch buffer is too small", rgb, p, out, scratch, NEED - 1)
    refused("not 16-byte aligned", rgb, p, out, scratch[4:], NEED)
    # an output right behind the scratch buffer is no overlap, and the call is served
    tail = scratch[NEED:].view(33, 17, 4)
    rc, _ = _device_call(lib, stream, rgb, p, tail, scratch, NEED)
    _abi.check(rc)
    stream.synchronize()
    assert same(tail.cpu().numpy(), dc.host(dc.images(17, 33), p))


# ---- the render leg ----
@pytest.fixture(scope="module")
def c1(gpu):
    """BASELINE C1 at 64 x 64, 4 samples per pixel."""
    prims, mk = scenes.config("C1")
    return mk().render(scenes.make_scene(prims))


def test_a_render_through_to_image_equals_the_host_path(c1):
    h, w = c1.rgb.shape[:2]
    for kw in (dict(), dict(exposure=1.0, curve="clamp", encode="reference"), dict(curve="filmic", encode="gamma22", percentile=0.9)):
        got = display.to_image(c1, **kw)
        assert got.shape == (h, w, 4) and got.dtype == np.uint8 and (got[..., 3] == 255).all()
        assert same(got, display.tonemap(c1.rgb, device=False, **kw))
    got = display.to_image(c1)
    assert 1 < len(np.unique(got[..., :3])) and got[..., :3].max() > 128      # a picture, not a constant
    scale, hist = display.exposure_of(c1.rgb)
    host_scale, host_hist = display.exposure_of(c1.rgb, device=False)
    assert scale == host_scale and same(hist, host_hist)


def test_the_command_line_writes_a_png_and_a_ppm(gpu, tmp_path):
    scene = tmp_path / "tiny.pbrt"
    scene.write_text('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\nSampler "lowdiscrepancy" "integer pixelsamples" [4]\n'
                     'Film "image" "integer xresolution" [24] "integer yresolution" [16]\nSurfaceIntegrator "directlighting"\nWorldBegin\n'
                     'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [8 8 8]\nTranslate 0 3 0\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                     '"point P" [-1 0 -1  1 0 -1  1 0 1  -1 0 1]\nAttributeEnd\n'
                     'Material "matte" "rgb Kd" [0.6 0.4 0.2]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
                     '"point P" [-2 -1 -2  2 -1 -2  2 -1 2  -2 -1 2]\nWorldEnd\n')
    png, ppm, npy = str(tmp_path / "o.png"), str(tmp_path / "o.ppm"), str(tmp_path / "o.npy")
    assert pbrt.main([str(scene), "-o", npy]) == 0
    rgb = np.load(npy)
    assert rgb.shape == (16, 24, 3) and rgb.dtype == np.float32           # .npy is the linear radiance, as before
    assert pbrt.main([str(scene), "-o", png]) == 0
    assert same(decode_png(png), display.tonemap(rgb, device=False))       # the defaults: auto-exposure at the median, reinhard, srgb
    assert pbrt.main([str(scene), "-o", ppm, "--exposure", "0.5", "--tonemap", "filmic", "--encode", "gamma22"]) == 0
    want = display.tonemap(rgb, exposure=0.5, curve="filmic", encode="gamma22", device=False)
    data = open(ppm, "rb").read()
    assert data == b"P6\n24 16\n255\n" + want[..., :3].tobytes()
