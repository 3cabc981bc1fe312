"""Inputs and callers shared by tests/test_temporal.py and tests/test_gpu_temporal.py (inputs only; the checker is
tests/temporal_restatement.py)."""
import ctypes as C
import itertools
import math

import numpy as np

from dartray_amd import _abi

SIZES = [(1, 1), (1, 5), (2, 2), (5, 7), (16, 9)]                        # (w, h)
MOVES = ["identity", "shift", "dolly", "rotate", "out_left", "out_right", "out_top", "out_bottom", "behind"]
MAX_HISTORY = [1, 2, 32]
DEPTH_TOL = [0.0, 0.02]
NORMAL_TOL = [0.0, 0.05]
PARAM_SETS = list(itertools.product(MAX_HISTORY, DEPTH_TOL, NORMAL_TOL))
DEFAULTS = (32, 0.02, 0.05)
CURRENT_PLANES = ["rgb", "normal", "depth"]
HISTORY_PLANES = ["h_rgb", "h_m2", "h_len", "h_normal", "h_depth"]
FOCAL = 12.0                                                             # pixels: a wide pinhole, so that a 16 x 9 image sees +-34 degrees


def pinhole(w, h, f=FOCAL):
    """(raster_to_camera, camera_to_raster) of a pinhole of focal length f pixels that looks along +z with the raster's centre on the axis:
    raster (X, Y) -> the camera-space point ((X - w/2) / f, (Y - h/2) / f, 1), and a camera-space point (x, y, z) -> (f x / z + w/2, f y / z + h/2)
    with the homogeneous coordinate z."""
    cx, cy = 0.5 * w, 0.5 * h
    r2c = np.array([[1 / f, 0, 0, -cx / f], [0, 1 / f, 0, -cy / f], [0, 0, 0, 1], [0, 0, 0, 1]], np.float64)
    c2r = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0], [0, 0, 1, 0]], np.float64)
    return r2c, c2r


def rigid(tx=0.0, ty=0.0, tz=0.0, yaw=0.0):
    """Current camera space -> previous camera space: a rotation about y by `yaw` radians, then a translation."""
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, 0, s, tx], [0, 1, 0, ty], [-s, 0, c, tz], [0, 0, 0, 1]], np.float64)


def move(name, w, h):
    """cur_to_prev of the named camera move for a scene about 3 units away under pinhole(w, h): one pixel is 3 / FOCAL = 0.25 units there."""
    px = 3.0 / FOCAL
    return {"identity": rigid(),
            "shift": rigid(tx=0.37 * px, ty=-0.21 * px),                 # a non-integer number of pixels
            "dolly": rigid(tz=-0.05),                                    # the current camera stands 0.05 further in
            "rotate": rigid(yaw=0.01, tx=0.003),
            "out_left": rigid(tx=-(0.5 * w + 0.3) * px),                 # half the image leaves the previous frame on that side
            "out_right": rigid(tx=(0.5 * w + 0.3) * px),
            "out_top": rigid(ty=-(0.5 * h + 0.3) * px),
            "out_bottom": rigid(ty=(0.5 * h + 0.3) * px),
            "behind": rigid(tz=-5.0)}[name]                              # depths about 3 and 7: the near surfaces end up at z < 0


def matrices(name, w, h):
    r2c, c2r = pinhole(w, h)
    return r2c, move(name, w, h), c2r


def frame(w, h, name, seed=5):
    """Seeded inputs of one call: the current frame (rgb, normal, depth) and a history (h_rgb, h_m2, h_len, h_normal, h_depth) as a dict.
    Colours over five decades, 0.5 * (n + 1) guides of unit normals a few degrees around one direction, depths within 1 % of 3 with a step of
    4 along a slanted line, so that a moved camera still finds taps that pass.  The
    history's guides are built from the current ones pixel by pixel -- which is what an identity move compares -- in three classes each, so
    that every tolerance has pixels on both sides: h_depth equals depth exactly, or is 1 % or 10 % off; h_normal equals normal exactly, or
    differs by a squared distance of about 0.01 or 0.3.  h_len is 1 .. 6."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * w + 10 * h + 7 * MOVES.index(name)))
    rgb = (10.0 ** rng.uniform(-3.0, 2.0, (h, w, 3))).astype(np.float32)
    n = 0.03 * rng.normal(size=(h, w, 3)) + np.array([0.2, -0.1, -1.0])
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    normal = (0.5 * (n + 1.0)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (3.0 + 0.02 * rng.random((h, w)) + 4.0 * (2 * xx + yy >= w + h // 2)).astype(np.float32)
    h_rgb = (10.0 ** rng.uniform(-3.0, 2.0, (h, w, 3))).astype(np.float32)
    h_m2 = (10.0 ** rng.uniform(-4.0, 4.0, (h, w))).astype(np.float32)
    h_len = rng.integers(1, 7, (h, w)).astype(np.float32)
    p = yy * w + xx
    h_depth = (depth * np.choose(p % 3, [1.0, 1.01, 1.1]).astype(np.float32)).astype(np.float32)
    h_normal = (normal + np.choose((p // 3) % 3, [0.0, 0.0577, 0.316]).astype(np.float32)[..., None]).astype(np.float32)
    return dict(rgb=rgb, normal=normal, depth=depth, h_rgb=h_rgb, h_m2=h_m2, h_len=h_len, h_normal=h_normal, h_depth=h_depth)


def plant(fr, plane, seed=17):
    """A copy of the frame with NaN, +inf and -inf in `plane` (one pixel each, where there are that many; one channel of a colour or normal)."""
    out = {k: v.copy() for k, v in fr.items()}
    target = out[plane]
    h, w = target.shape[:2]
    rng = np.random.Generator(np.random.PCG64(seed + w + 100 * h))
    for k, q in enumerate(rng.permutation(w * h)[:3]):
        bad = [np.nan, np.inf, -np.inf][k]
        if target.ndim == 2:
            target[q // w, q % w] = bad
        else:
            target[q // w, q % w, (q + k) % 3] = bad
    return out


def holes(fr):
    """A copy of the frame whose history has h_len = 0 at every third pixel, the first among them."""
    out = {k: v.copy() for k, v in fr.items()}
    out["h_len"].reshape(-1)[::3] = 0.0
    return out


def history_of(fr):
    return tuple(fr[k] for k in HISTORY_PLANES)


def grid():
    """Every case of the byte-for-byte comparison: (key, frame dict, history or None, matrices, (max_history, depth_tol, normal_tol))."""
    for size in SIZES:
        for name in MOVES:
            fr = frame(*size, name)
            m = matrices(name, *size)
            for ps in PARAM_SETS:
                yield (size, name, "history", ps), fr, history_of(fr), m, ps
            yield (size, name, "holes"), holes(fr), history_of(holes(fr)), m, DEFAULTS
            for plane in CURRENT_PLANES + HISTORY_PLANES:
                bad = plant(fr, plane)
                yield (size, name, "planted", plane), bad, history_of(bad), m, DEFAULTS
            for mh in MAX_HISTORY:
                yield (size, name, "first", mh), fr, None, m, (mh, 0.02, 0.05)
            for plane in CURRENT_PLANES:
                yield (size, name, "first planted", plane), plant(fr, plane), None, m, DEFAULTS


def params(m, max_history, depth_tol, normal_tol):
    p = _abi.DrTemporalParams()
    for name, a in zip(("raster_to_camera", "cur_to_prev", "prev_to_raster"), m):
        getattr(p, name)[:] = [float(v) for v in np.asarray(a, np.float64).reshape(-1)]
    p.depth_tol, p.normal_tol, p.max_history = float(depth_tol), float(normal_tol), int(max_history)
    return p


SENTINEL = -7.0


def call(fn, rgb, normal, depth, history, m, max_history, depth_tol, normal_tol):
    """One of the two host-buffer entry points -> (return code, (out_rgb, out_m2, out_len)); the outputs start as a sentinel."""
    rgb, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb, normal, depth))
    hist = [None] * 5 if history is None else [np.ascontiguousarray(a, np.float32) for a in history]
    h, w = depth.shape
    out = np.full_like(rgb, SENTINEL), np.full_like(depth, SENTINEL), np.full_like(depth, SENTINEL)
    p = params(m, max_history, depth_tol, normal_tol)
    rc = fn(rgb.ctypes.data, normal.ctypes.data, depth.ctypes.data, *[a.ctypes.data if a is not None else None for a in hist], w, h, C.byref(p),
            *[o.ctypes.data for o in out])
    return rc, out


def host(rgb, normal, depth, history, m, max_history, depth_tol, normal_tol):
    rc, out = call(_abi.lib().dr_temporal_host, rgb, normal, depth, history, m, max_history, depth_tol, normal_tol)
    _abi.check(rc)
    return out


def random_sequence(w, h, frames=3, seed=23):
    """The larger GPU cases: `frames` frames of (rgb, normal, depth, matrices) over one slanted surface with a depth step, a small random
    camera move between each two, and NaN / +inf / -inf sprinkled over about one pixel in fifty of each plane."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * w + h))
    f = max(w, h, 64) * 0.9
    r2c, c2r = pinhole(w, h, f=f)
    yy, xx = np.mgrid[0:h, 0:w]
    n = rng.normal(size=(h, w, 3)) * 0.05 + np.array([0.2, -0.1, -1.0])
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    base_normal = (0.5 * (n + 1.0)).astype(np.float32)
    base_depth = 3.0 + 4.0 * (2 * xx + yy >= w + h // 2)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    out = []
    for k in range(frames):
        rgb = (10.0 ** rng.uniform(-3.0, 2.0, (h, w, 3))).astype(np.float32)
        normal = base_normal.copy()
        depth = (base_depth * (1.0 + 0.004 * rng.random((h, w)))).astype(np.float32)
        where, pick = rng.random((h, w)), rng.integers(0, 3, (h, w))
        rgb[where < 0.02, 1] = bad[pick[where < 0.02]]
        normal[(where >= 0.02) & (where < 0.04), 0] = bad[pick[(where >= 0.02) & (where < 0.04)]]
        depth[(where >= 0.04) & (where < 0.06)] = bad[pick[(where >= 0.04) & (where < 0.06)]]
        depth[(where >= 0.06) & (where < 0.07)] = 0.0                    # a miss
        t = rng.uniform(-1.0, 1.0, 3) * np.array([1.5 * 3.0 / f, 1.5 * 3.0 / f, 0.02])     # up to 1.5 pixels sideways at depth 3
        m = (r2c, rigid(tx=t[0], ty=t[1], tz=t[2], yaw=rng.uniform(-0.5, 0.5) / f), c2r)     # and up to half a pixel of rotation
        out.append((rgb, normal, depth, m))
    return out
