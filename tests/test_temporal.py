"""Temporal accumulation with reprojection without a GPU: dr_temporal_host against the numpy restatement
(tests/temporal_restatement.py, written from the text) bit for bit on the smallest images and camera moves where the rule can go wrong, with
and without a history, non-finite values and holes; answers derived by hand, checked against both; every refusal by code and text; and the
Python module above them (dartray_amd/denoise.py)."""
import ctypes as C

import numpy as np
import pytest

from dartray_amd import _abi, core, denoise, scenes

import temporal_cases as tc
import temporal_restatement as tr

F = np.float32
same = tr.same_bits


def _both(rgb, normal, depth, history, m, ps=tc.DEFAULTS):
    """The restatement's and the host entry's results, which must agree before either is compared with a derived answer.
    ps = (max_history, depth_tol, normal_tol)."""
    a = tr.temporal(rgb, normal, depth, history, m, ps[1], ps[2], ps[0])
    b = tc.host(rgb, normal, depth, history, m, *ps)
    assert all(same(x, y) for x, y in zip(a, b)), ps
    return a


def _next(out, normal, depth):
    """The history a call's outputs and its frame's guides make for the next call."""
    return out[0], out[1], out[2], normal, depth


def _lum2(rgb):
    l = tr.lum(np.asarray(rgb, np.float32))
    return l * l


# ---- 1. host == restatement, bit for bit ----
@pytest.mark.parametrize("name", tc.MOVES)
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_bit_for_bit(hip, size, name):
    fr, m = tc.frame(*size, name), tc.matrices(name, *size)
    outs = [_both(fr["rgb"], fr["normal"], fr["depth"], tc.history_of(fr), m, ps) for ps in tc.PARAM_SETS]
    assert all(np.isfinite(a).all() and (a != tc.SENTINEL).all() for o in outs for a in o)
    first = [_both(fr["rgb"], fr["normal"], fr["depth"], None, m, (mh, 0.02, 0.05)) for mh in tc.MAX_HISTORY]
    assert all(same(a, b) for o in first[1:] for a, b in zip(o, first[0]))          # no parameter is read without a history
    gaps = tc.holes(fr)
    _both(gaps["rgb"], gaps["normal"], gaps["depth"], tc.history_of(gaps), m)
    if size == (5, 7) and name == "identity":
        # ... and the switches are read: no two of the twelve parameter sets agree.  The identity move is the one where the history's guides
        # -- built from the current ones pixel by pixel -- have pixels that pass a tolerance of 0; under any other move a depth_tol of 0
        # passes no tap, every pixel restarts and nothing else can show.
        flat = [np.concatenate([a.reshape(-1) for a in o]) for o in outs]
        assert not any(same(flat[i], flat[j]) for i in range(len(flat)) for j in range(i))
        holed = tr.temporal(gaps["rgb"], gaps["normal"], gaps["depth"], tc.history_of(gaps), m, 0.02, 0.05, 32)
        assert not same(holed[2], outs[tc.PARAM_SETS.index(tc.DEFAULTS)][2])


@pytest.mark.parametrize("plane", tc.CURRENT_PLANES + tc.HISTORY_PLANES)
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement_on_non_finite_values(hip, size, plane):
    for name in tc.MOVES:
        bad, m = tc.plant(tc.frame(*size, name), plane), tc.matrices(name, *size)
        assert not np.isfinite(bad[plane]).all()
        _both(bad["rgb"], bad["normal"], bad["depth"], tc.history_of(bad), m)
        if plane in tc.CURRENT_PLANES:
            _both(bad["rgb"], bad["normal"], bad["depth"], None, m)


def test_the_grid_has_every_case_and_both_outcomes(hip):
    """The generator the GPU suite walks: its size, and that among its default-parameter cases each move but `behind` has pixels that
    accumulate and pixels that restart at 16 x 9 (`behind` only restarts: its surfaces are behind the previous camera or far off in depth)."""
    cases = list(tc.grid())
    assert len(cases) == len(tc.SIZES) * len(tc.MOVES) * (12 + 1 + 8 + 3 + 3) == 1215
    for key, fr, hist, m, ps in cases:
        if key[0] == (16, 9) and key[2] == "history" and ps == tc.DEFAULTS:
            n = tr.temporal(fr["rgb"], fr["normal"], fr["depth"], hist, m, ps[1], ps[2], ps[0])[2]
            assert (n == 1).any(), key
            assert (n > 1).any() == (key[1] != "behind"), key


# ---- 2. answers derived by hand ----
def test_a_first_frame_gives_its_inputs_back(hip):
    fr = tc.frame(5, 7, "identity")
    rgb, m2, n = _both(fr["rgb"], fr["normal"], fr["depth"], None, tc.matrices("identity", 5, 7))
    assert same(rgb, fr["rgb"]) and (n == 1).all() and same(m2, _lum2(fr["rgb"]))


def test_b_static_camera_and_a_constant_image_stay_put(hip):
    fr, m = tc.frame(16, 9, "identity"), tc.matrices("identity", 16, 9)
    c, normal, depth = fr["rgb"], fr["normal"], fr["depth"]
    for most in (1, 3, 32):
        hist = None
        for k in range(1, 6):
            out = _both(c, normal, depth, hist, m, (most, 0.02, 0.05))
            assert same(out[0], c) and (out[2] == min(k, most)).all() and same(out[1], _lum2(c)), (most, k)
            hist = _next(out, normal, depth)


def test_c_static_camera_two_frames_give_their_mean_in_the_rules_order(hip):
    fr, m = tc.frame(16, 9, "identity"), tc.matrices("identity", 16, 9)
    a, b, normal, depth = fr["rgb"], fr["h_rgb"], fr["normal"], fr["depth"]
    first = _both(a, normal, depth, None, m)
    out = _both(b, normal, depth, _next(first, normal, depth), m)
    assert same(out[0], a + F(0.5) * (b - a)) and (out[2] == 2).all()
    la, lb = _lum2(a), _lum2(b)
    assert same(out[1], la + F(0.5) * (lb - la))
    third = _both(a, normal, depth, _next(out, normal, depth), m)
    assert same(third[0], out[0] + (F(1) / F(3)) * (a - out[0])) and (third[2] == 3).all()


def _plane(w, h, z):
    """The guides of the plane z = Z in front of tc.pinhole(w, h): depth t = Z * |(x, y, 1)| along the normalised ray, one normal."""
    yy, xx = np.mgrid[0:h, 0:w]
    x, y = (xx + 0.5 - 0.5 * w) / tc.FOCAL, (yy + 0.5 - 0.5 * h) / tc.FOCAL
    return np.full((h, w, 3), 0.5, np.float32), (z * np.sqrt(x * x + y * y + 1.0)).astype(np.float32)


@pytest.mark.parametrize("k", [1, 3, -2])
@pytest.mark.parametrize("size", [(5, 7), (16, 9)], ids=lambda s: "%dx%d" % s)
def test_d_a_plane_and_an_exact_pixel_shift_take_the_history_from_pixel_x_plus_k(hip, size, k):
    """A fronto-parallel plane at z = Z under a pinhole of focal length f pixels, the camera translated by k Z / f along x: the point under
    pixel x lay under pixel x + k, exactly, so the snapped coordinate is an integer, one tap has weight 1 and the answer has the bits of c."""
    w, h = size
    z = 4.0
    r2c, c2r = tc.pinhole(w, h)
    m = (r2c, tc.rigid(tx=k * z / tc.FOCAL), c2r)
    normal, depth = _plane(w, h, z)
    ud, vd, tz, ok = tr.reproject(depth, m)
    yy, xx = np.mgrid[0:h, 0:w]
    assert ok.all() and np.abs(ud - (xx + k)).max() < 1 / 1024 and np.abs(vd - yy).max() < 1 / 1024      # the condition for exactness
    fr = tc.frame(w, h, "shift")
    a, b = fr["rgb"], fr["h_rgb"]
    first = _both(a, normal, depth, None, m)
    out = _both(b, normal, depth, _next(first, normal, depth), m)
    inside = (xx + k >= 0) & (xx + k < w)
    assert inside.any() and not inside.all()
    src = np.clip(xx + k, 0, w - 1)
    moved = a[yy, src]
    la, lb = _lum2(moved), _lum2(b)
    assert same(out[0][inside], (moved + F(0.5) * (b - moved))[inside]) and (out[2][inside] == 2).all()
    assert same(out[1][inside], (la + F(0.5) * (lb - la))[inside])
    assert same(out[0][~inside], b[~inside]) and (out[2][~inside] == 1).all() and same(out[1][~inside], lb[~inside])


def test_e_a_disoccluded_pixel_restarts(hip):
    fr, m = tc.frame(16, 9, "identity"), tc.matrices("identity", 16, 9)
    a, b, normal, depth = fr["rgb"], fr["h_rgb"], fr["normal"], fr["depth"]
    first = _both(a, normal, depth, None, m)
    off = np.zeros((9, 16), bool)
    off[2:5, 3:9] = True
    mean = a + F(0.5) * (b - a)
    # the previous frame saw something 5 % further away there
    h_depth = np.where(off, depth * F(1.05), depth).astype(np.float32)
    out = _both(b, normal, depth, (first[0], first[1], first[2], normal, h_depth), m)
    assert same(out[0][off], b[off]) and (out[2][off] == 1).all() and same(out[1][off], _lum2(b)[off])
    assert same(out[0][~off], mean[~off]) and (out[2][~off] == 2).all()
    out = _both(b, normal, depth, (first[0], first[1], first[2], normal, h_depth), m, (32, 0.1, 0.05))
    assert same(out[0], mean) and (out[2] == 2).all()
    # ... or a surface turned by 0.2 in every component of the encoded normal: a squared distance of 0.12
    h_normal = np.where(off[..., None], normal + F(0.2), normal).astype(np.float32)
    out = _both(b, normal, depth, (first[0], first[1], first[2], h_normal, depth), m)
    assert same(out[0][off], b[off]) and (out[2][off] == 1).all() and same(out[0][~off], mean[~off]) and (out[2][~off] == 2).all()
    out = _both(b, normal, depth, (first[0], first[1], first[2], h_normal, depth), m, (32, 0.02, 0.2))
    assert same(out[0], mean) and (out[2] == 2).all()


@pytest.mark.parametrize("plane", tc.CURRENT_PLANES)
def test_f_an_invalid_pixel_passes_through_and_is_no_tap_of_the_next_frame(hip, plane):
    """Frame 1 has three pixels with a NaN, a +inf and a -inf in `plane`; frame 2 is seen from a camera shifted by a fraction of a pixel, so
    that every pixel blends four taps and the invalid ones are among its neighbours'."""
    w, h = 16, 9
    m = tc.matrices("shift", w, h)
    normal, depth = _plane(w, h, 3.0)
    fr = tc.frame(w, h, "shift")
    planes = tc.plant(dict(rgb=fr["rgb"], normal=normal, depth=depth), plane)
    ok = np.isfinite(planes["rgb"]).all(axis=2) & np.isfinite(planes["normal"]).all(axis=2) & np.isfinite(planes["depth"])
    assert (~ok).sum() == 3
    first = _both(planes["rgb"], planes["normal"], planes["depth"], None, m)
    assert same(first[0], planes["rgb"])                                 # passed through, bit for bit
    colour = np.isfinite(planes["rgb"]).all(axis=2)
    assert (first[2] == np.where(colour, 1, 0)).all() and (first[1][~colour] == 0).all() and np.isfinite(first[1]).all()
    second = _both(fr["h_rgb"], normal, depth, _next(first, planes["normal"], planes["depth"]), m)
    assert all(np.isfinite(a).all() for a in second) and (second[2] == 2).sum() > w * h // 2 and second[0].max() < 1000.0
    # the invalid pixels' finite colour values, changed to 1e6, show nowhere in the next frame
    other = planes["rgb"].copy()
    other[~ok] = np.where(np.isfinite(other[~ok]), 1.0e6, other[~ok])
    assert not same(other, planes["rgb"])
    first2 = _both(other, planes["normal"], planes["depth"], None, m)
    second2 = _both(fr["h_rgb"], normal, depth, _next(first2, planes["normal"], planes["depth"]), m)
    assert all(same(x, y) for x, y in zip(second, second2))
    # and with a static camera the pixel above an invalid one restarts, while every other one accumulates
    still = tc.matrices("identity", w, h)
    again = _both(fr["h_rgb"], normal, depth, _next(first, planes["normal"], planes["depth"]), still)
    assert (again[2][~ok] == 1).all() and (again[2][ok] == 2).all() and same(again[0][~ok], fr["h_rgb"][~ok])


def test_a_miss_passes_through(hip):
    """depth 0 is what the feature integrator writes where the camera ray leaves the scene: not current-valid, len 1."""
    fr, m = tc.frame(5, 7, "identity"), tc.matrices("identity", 5, 7)
    depth = fr["depth"].copy()
    depth[2, 1:4] = 0.0
    depth[3, 2] = -1.0
    out = _both(fr["rgb"], fr["normal"], depth, (fr["h_rgb"], fr["h_m2"], fr["h_len"], fr["normal"], depth), m)
    miss = depth <= 0
    assert same(out[0][miss], fr["rgb"][miss]) and (out[2][miss] == 1).all() and (out[2][~miss] > 1).all()


# ---- 3. the refusals, by code and text ----
def test_every_refusal_by_code_and_text(hip):
    lib = hip.lib()
    fr = tc.frame(3, 2, "identity")
    m = tc.matrices("identity", 3, 2)
    # the outputs lie in one allocation with room behind them: a pointer moved past an output's end stays clear of the inputs wherever the
    # heap has put those
    room = np.zeros(64, np.float32)
    outs = dict(out_rgb=room[:18].reshape(2, 3, 3), out_m2=room[18:24].reshape(2, 3), out_len=room[24:30].reshape(2, 3))
    arrays = dict(fr, **outs)
    ptr = {k: v.ctypes.data for k, v in arrays.items()}
    order = tc.CURRENT_PLANES + tc.HISTORY_PLANES
    ok = tc.params(m, *tc.DEFAULTS)

    def refused(needle, w=3, h=2, p=ok, images_only=False, **over):
        a = dict(ptr, **over)
        pp = C.byref(p) if p is not None else None
        calls = [lambda fn=fn: fn(*[a[k] for k in order], w, h, pp, a["out_rgb"], a["out_m2"], a["out_len"]) for fn in (lib.dr_temporal_host, lib.dr_temporal)]
        calls.append(lambda: lib.dr_temporal_device(*[a[k] for k in order], w, h, pp, a["out_rgb"], a["out_m2"], a["out_len"], None))
        if not images_only:
            calls.append(lambda: lib.dr_temporal_check(pp, w, h))
        for one in calls:                                                # the same checks, ahead of any device call
            rc = one()
            assert rc == -1, (needle, rc)
            assert needle in lib.dr_last_error().decode(), (needle, lib.dr_last_error())

    def with_(**fields):
        p = tc.params(m, *tc.DEFAULTS)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    for name in tc.CURRENT_PLANES + list(outs):
        refused("a null pointer", images_only=True, **{name: None})
    refused("a null pointer", p=None)
    for name in tc.HISTORY_PLANES:                                       # one missing, or only one there
        refused("the history is only partly NULL", images_only=True, **{name: None})
        refused("the history is only partly NULL", images_only=True, **{k: None for k in tc.HISTORY_PLANES if k != name})
    refused("w and h must be at least 1", w=0)
    refused("w and h must be at least 1", h=-2)
    refused("the image has 2^31 or more pixels", w=65536, h=32768)
    refused("the image has 2^31 or more pixels", w=2 ** 31 - 1, h=2 ** 31 - 1)
    assert lib.dr_temporal_check(C.byref(ok), 65536, 32767) == 0
    for bad in (-1.0, float("inf"), float("nan"), -0.5):
        refused("depth_tol and normal_tol must be finite and not negative", p=with_(depth_tol=bad))
        refused("depth_tol and normal_tol must be finite and not negative", p=with_(normal_tol=bad))
    for bad in (0, -1, 4097, 2 ** 31 - 1):
        refused("max_history must be in 1..4096", p=with_(max_history=bad))
    assert lib.dr_temporal_check(C.byref(with_(max_history=4096, depth_tol=0.0, normal_tol=0.0)), 3, 2) == 0
    for field in ("raster_to_camera", "cur_to_prev", "prev_to_raster"):
        for k in (0, 7, 15):
            for bad in (float("nan"), float("inf"), float("-inf")):
                p = tc.params(m, *tc.DEFAULTS)
                getattr(p, field)[k] = bad
                refused("a matrix element is not finite", p=p)
    nbytes = {k: v.nbytes for k, v in arrays.items()}
    for o in outs:
        for name in order:
            refused("an output overlaps an input", images_only=True, **{o: ptr[name]})
            refused("an output overlaps an input", images_only=True, **{o: ptr[name] + nbytes[name] - 4})     # its first float is the input's last
            refused("an output overlaps an input", images_only=True, **{name: ptr[o] + nbytes[o] - 4})
    refused("an output overlaps another output", images_only=True, out_m2=ptr["out_rgb"] + 8)
    refused("an output overlaps another output", images_only=True, out_len=ptr["out_m2"])
    refused("an output overlaps another output", images_only=True, out_len=ptr["out_rgb"] + nbytes["out_rgb"] - 4)
    # nothing of the above left a mark, and the all-NULL history is served
    assert lib.dr_temporal_check(C.byref(ok), 3, 2) == 0
    assert lib.dr_temporal_host(*[ptr[k] for k in tc.CURRENT_PLANES], None, None, None, None, None, 3, 2, C.byref(ok), ptr["out_rgb"], ptr["out_m2"],
                                ptr["out_len"]) == 0
    assert same(outs["out_rgb"], fr["rgb"])


def test_the_struct_is_four_hundred_bytes_in_every_binding():
    assert C.sizeof(_abi.DrTemporalParams) == 400
    assert [(n, getattr(_abi.DrTemporalParams, n).offset) for n, _ in _abi.DrTemporalParams._fields_] == [
        ("raster_to_camera", 0), ("cur_to_prev", 128), ("prev_to_raster", 256), ("depth_tol", 384), ("normal_tol", 388), ("max_history", 392),
        ("reserved", 396)]


# ---- 4. the Python module ----
def _film(xres=32, yres=24):
    return core.ImageFilm(xres, yres, core.BoxFilter(0.5, 0.5))


def _poses():
    film = _film()
    cur = core.PerspectiveCamera.lookAt((1.0, 0.5, -35.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, film)
    prev = core.PerspectiveCamera.lookAt((-2.0, 1.0, -34.0), (0.5, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, film)
    return cur, prev


def test_temporal_matrices_against_a_direct_composition():
    cur, prev = _poses()
    r2c, c2p, p2r = denoise.temporal_matrices(cur, prev)
    assert all(a.dtype == np.float64 and a.shape == (4, 4) for a in (r2c, c2p, p2r))
    d = lambda a: np.array(a, np.float64).reshape(4, 4)
    assert np.array_equal(r2c, d(cur.rasterToCamera))
    assert np.array_equal(c2p, np.linalg.inv(d(prev.cameraToWorld)) @ d(cur.cameraToWorld))
    assert np.array_equal(p2r, np.linalg.inv(d(prev.rasterToCamera)))
    # ... and what they are for: a world point seen by both cameras, taken from the current camera's space to the previous raster, lands
    # where the previous camera's own matrices put it
    world = np.array([0.7, -0.4, 1.5, 1.0])
    in_cur = np.linalg.solve(d(cur.cameraToWorld), world)
    in_prev = np.linalg.solve(d(prev.cameraToWorld), world)
    assert np.allclose(c2p @ in_cur, in_prev, rtol=0, atol=1e-9) and in_prev[2] > 0
    raster = p2r @ in_prev
    back = d(prev.rasterToCamera) @ np.array([raster[0] / raster[3], raster[1] / raster[3], 0.0, 1.0])
    back = back[:3] / back[3]
    assert np.allclose(back / back[2], in_prev[:3] / in_prev[2], rtol=0, atol=1e-9)
    assert 0 < raster[0] / raster[3] < 32 and 0 < raster[1] / raster[3] < 24
    # one camera twice: the identity up to the inverse's rounding, and every pixel centre back onto itself after the snap
    r2c, c2p, p2r = denoise.temporal_matrices(cur, cur)
    assert np.allclose(c2p, np.eye(4), rtol=0, atol=1e-12)
    ud, vd, _, ok = tr.reproject(np.full((24, 32), 30.0, np.float32), (r2c, c2p, p2r))
    yy, xx = np.mgrid[0:24, 0:32]
    assert ok.all() and np.array_equal(tr.snap(ud), xx.astype(np.float32)) and np.array_equal(tr.snap(vd), yy.astype(np.float32))


def test_temporal_matrices_refuses_by_name():
    cur, prev = _poses()
    ortho = core.OrthographicCamera.lookAt((0.0, 0.0, -35.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), _film())
    env = core.EnvironmentCamera.lookAt((0.0, 0.0, -35.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), _film())
    lens = core.PerspectiveCamera.lookAt((0.0, 0.0, -35.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, _film(), lensradius=0.5, focaldistance=30.0)
    small = core.PerspectiveCamera.lookAt((0.0, 0.0, -35.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, _film(16, 24))
    with pytest.raises(ValueError, match="temporal_matrices: camera is a OrthographicCamera: only a PerspectiveCamera is supported"):
        denoise.temporal_matrices(ortho, prev)
    with pytest.raises(ValueError, match="temporal_matrices: prev_camera is a EnvironmentCamera: only a PerspectiveCamera is supported"):
        denoise.temporal_matrices(cur, env)
    with pytest.raises(ValueError, match=r"temporal_matrices: prev_camera has lensRadius 0.5: a camera with a lens is not supported"):
        denoise.temporal_matrices(cur, lens)
    with pytest.raises(ValueError, match=r"temporal_matrices: camera has lensRadius 0.5"):
        denoise.temporal_matrices(lens, prev)
    with pytest.raises(ValueError, match=r"temporal_matrices: the two cameras' films differ in size \(32 x 24 and 16 x 24\)"):
        denoise.temporal_matrices(cur, small)


def test_the_module_on_the_host_equals_the_restatement(hip):
    assert (denoise.DEPTH_TOL, denoise.NORMAL_TOL, denoise.MAX_HISTORY) == (0.02, 0.05, 32)
    fr, m = tc.frame(16, 9, "shift"), tc.matrices("shift", 16, 9)
    first = denoise.temporal(fr["rgb"], fr["normal"], fr["depth"], None, m, device=False)
    assert same(first.rgb, fr["rgb"]) and (first.len == 1).all() and first.normal.shape == (9, 16, 3) and first.depth.shape == (9, 16)
    assert (first.variance == 0).all()
    second = denoise.temporal(fr["h_rgb"], fr["normal"], fr["depth"], first, m, device=False)
    want = tr.temporal(fr["h_rgb"], fr["normal"], fr["depth"], (first.rgb, first.m2, first.len, first.normal, first.depth), m, 0.02, 0.05, 32)
    assert same(second.rgb, want[0]) and same(second.m2, want[1]) and same(second.len, want[2]) and (second.len == 2).any()
    l = tr.lum(second.rgb)
    assert same(second.variance, np.maximum(F(0), second.m2 - l * l)) and (second.variance > 0).any() and second.variance.dtype == np.float32
    tight = denoise.temporal(fr["h_rgb"], fr["normal"], fr["depth"], first, m, depth_tol=0.0, normal_tol=0.01, max_history=1, device=False)
    want = tr.temporal(fr["h_rgb"], fr["normal"], fr["depth"], (first.rgb, first.m2, first.len, first.normal, first.depth), m, 0.0, 0.01, 1)
    assert same(tight.rgb, want[0]) and same(tight.len, want[2])
    with pytest.raises(ValueError, match=r"temporal: rgb and normal must be \[h, w, 3\] and depth \[h, w\] \(got \(9, 16, 3\), \(9, 16, 3\), \(9, 15\)\)"):
        denoise.temporal(fr["rgb"], fr["normal"], fr["depth"][:, :15], None, m, device=False)
    with pytest.raises(ValueError, match=r"temporal: the history is of another size \(\(9, 16, 3\) for \(8, 16, 3\)\)"):
        denoise.temporal(fr["rgb"][:8], fr["normal"][:8], fr["depth"][:8], first, m, device=False)
    with pytest.raises(ValueError, match="temporal: matrices must be"):
        denoise.temporal(fr["rgb"], fr["normal"], fr["depth"], None, m[:2], device=False)
    with pytest.raises(ValueError, match="temporal: cur_to_prev must be a 4 x 4 matrix"):
        denoise.temporal(fr["rgb"], fr["normal"], fr["depth"], None, (m[0], np.eye(3), m[2]), device=False)
    with pytest.raises(_abi.DartRayHipError, match=r"max_history must be in 1\.\.4096"):
        denoise.temporal(fr["rgb"], fr["normal"], fr["depth"], None, m, max_history=0, device=False)
    with pytest.raises(_abi.DartRayHipError, match="depth_tol and normal_tol must be finite and not negative"):
        denoise.temporal(fr["rgb"], fr["normal"], fr["depth"], first, m, normal_tol=-1.0, device=False)


def _renderer(cam=None, sampler=None, **kw):
    cam = cam or scenes.cornell_camera(16, 16)
    return core.SamplerRenderer(sampler(cam) if sampler else core.LowDiscrepancySampler(cam, 4, 5489), cam, core.PathIntegrator(3),
                                core.EmissionIntegrator(), **kw)


def test_render_sequence_refuses_by_name_before_it_renders():
    ok = _renderer()
    with pytest.raises(ValueError, match="render_sequence: normal_channel must be ns or ng"):
        denoise.render_sequence([ok], None, normal_channel="uv")
    with pytest.raises(ValueError, match="render_sequence: iterations given without denoise=True"):
        denoise.render_sequence([ok], None, iterations=3)
    adaptive = lambda cam: core.AdaptiveSampler(cam, 4, 16, "contrast", 5489)
    with pytest.raises(ValueError, match=r"render_sequence: the adaptive sampler is not supported \(renderers\[1\]"):
        denoise.render_sequence([ok, _renderer(sampler=adaptive)], None)
    with pytest.raises(ValueError, match=r"render_sequence: tileCount > 1 and taskCount > 1 are not supported \(renderers\[0\] has 2 and 1\)"):
        denoise.render_sequence([_renderer(tileCount=2), ok], None)
    cropped = _renderer()
    cropped.camera.film = core.ImageFilm(16, 16, core.BoxFilter(0.5, 0.5), (0.0, 0.5, 0.0, 1.0))
    with pytest.raises(ValueError, match=r"render_sequence: a crop window other than the whole film is not supported \(renderers\[1\] has"):
        denoise.render_sequence([ok, cropped], None)
    lens = core.PerspectiveCamera.lookAt((0.0, 0.0, -35.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, _film(16, 16), lensradius=0.5, focaldistance=30.0)
    with pytest.raises(ValueError, match=r"render_sequence: renderers\[1\].camera has lensRadius 0.5"):
        denoise.render_sequence([ok, _renderer(cam=lens)], None)
    ortho = core.OrthographicCamera.lookAt((0.0, 0.0, -35.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), _film(16, 16))
    with pytest.raises(ValueError, match=r"render_sequence: renderers\[0\].camera is a OrthographicCamera"):
        denoise.render_sequence([_renderer(cam=ortho)], None)
    with pytest.raises(ValueError, match=r"temporal_matrices: the two cameras' films differ in size \(32 x 32 and 16 x 16\)"):
        denoise.render_sequence([ok, _renderer(cam=scenes.cornell_camera(32, 32))], None)
