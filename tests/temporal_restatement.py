"""Temporal accumulation with reprojection restated in numpy from the text of DESIGN.md 2.23 (not from the C code): the geometry is one
np.float64 operation per operator on arrays, everything after the rounding of (u, v) one np.float32 operation, in the order the text writes
them, so the result is compared with the library's bit for bit.

    temporal(rgb[h, w, 3], normal[h, w, 3], depth[h, w], history, matrices, depth_tol, normal_tol, max_history)
        -> (out_rgb [h, w, 3], out_m2 [h, w], out_len [h, w]) float32

history is None or (h_rgb [h, w, 3], h_m2 [h, w], h_len [h, w], h_normal [h, w, 3], h_depth [h, w]); matrices is (raster_to_camera,
cur_to_prev, prev_to_raster), three 4 x 4 float64 arrays.
"""
import numpy as np

F = np.float32
D = np.float64


def lum(rgb):
    """(0.212671 r + 0.715160 g) + 0.072169 b, the pair denoiser's weights"""
    return (F(0.212671) * rgb[..., 0] + F(0.715160) * rgb[..., 1]) + F(0.072169) * rgb[..., 2]


def _row(m, k, a, b, c):
    """row k of m times (a, b, c, 1): ((m0 a + m1 b) + m2 c) + m3"""
    return ((m[k, 0] * a + m[k, 1] * b) + m[k, 2] * c) + m[k, 3]


def reproject(depth, matrices):
    """Step 2 up to the rounding to f32: (ud, vd, tz, ok), all [h, w]; ud, vd, tz float64, ok False where the pixel has no history for a
    reason of the geometry alone (q.z <= 0, r.w <= 0, something not finite)."""
    rc, c2p, p2r = (np.asarray(m, D).reshape(4, 4) for m in matrices)
    depth = np.ascontiguousarray(depth, np.float32)
    h, w = depth.shape
    ys, xs = np.mgrid[0:h, 0:w]
    rx, ry = xs.astype(D) + D(0.5), ys.astype(D) + D(0.5)
    with np.errstate(all="ignore"):
        pw = (rc[3, 0] * rx + rc[3, 1] * ry) + rc[3, 3]                    # the raster point's z is 0: its column takes no part
        px = ((rc[0, 0] * rx + rc[0, 1] * ry) + rc[0, 3]) / pw
        py = ((rc[1, 0] * rx + rc[1, 1] * ry) + rc[1, 3]) / pw
        pz = ((rc[2, 0] * rx + rc[2, 1] * ry) + rc[2, 3]) / pw
        ln = np.sqrt((px * px + py * py) + pz * pz)
        t = depth.astype(D)
        cx, cy, cz = (px / ln) * t, (py / ln) * t, (pz / ln) * t
        qx, qy, qz = _row(c2p, 0, cx, cy, cz), _row(c2p, 1, cx, cy, cz), _row(c2p, 2, cx, cy, cz)
        tz = np.sqrt((qx * qx + qy * qy) + qz * qz)
        sx, sy, sw = _row(p2r, 0, qx, qy, qz), _row(p2r, 1, qx, qy, qz), _row(p2r, 3, qx, qy, qz)
        ok = np.isfinite(qx) & np.isfinite(qy) & np.isfinite(qz) & np.isfinite(tz) & np.isfinite(sx) & np.isfinite(sy) & np.isfinite(sw)
        ok &= (qz > 0) & (sw > 0)
        ud, vd = sx / sw - D(0.5), sy / sw - D(0.5)
    return ud, vd, tz, ok


def snap(c):
    """f64 -> f32 -> the nearest 1/256"""
    with np.errstate(all="ignore"):
        return np.floor(c.astype(np.float32) * F(256) + F(0.5)) / F(256)


def temporal(rgb, normal, depth, history, matrices, depth_tol, normal_tol, max_history):
    rgb, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb, normal, depth))
    h, w = depth.shape
    assert rgb.shape == normal.shape == (h, w, 3)
    colour = np.isfinite(rgb).all(axis=2)
    valid = colour & np.isfinite(normal).all(axis=2) & np.isfinite(depth) & (depth > 0)                   # step 1
    with np.errstate(all="ignore"):
        cur_m2 = lum(rgb)
        cur_m2 = cur_m2 * cur_m2
    # a pixel that restarts: the colour copied as integers (no operation touches a NaN's payload), m2 = lum^2 or 0, len 1 or 0
    out_rgb = rgb.view(np.uint32).copy()
    out_m2 = np.where(np.isfinite(cur_m2), cur_m2, F(0)).astype(np.float32)
    out_len = np.where(colour, F(1), F(0)).astype(np.float32)
    if history is None:
        return out_rgb.view(np.float32), out_m2, out_len
    h_rgb, h_m2, h_len, h_normal, h_depth = (np.ascontiguousarray(a, np.float32) for a in history)
    dtol, ntol, most = F(depth_tol), F(normal_tol), F(int(max_history))
    ud, vd, tz, ok = reproject(depth, matrices)                                                          # step 2
    with np.errstate(all="ignore"):
        ok = ok & valid & np.isfinite(ud.astype(np.float32)) & np.isfinite(vd.astype(np.float32))
        u, v = snap(ud), snap(vd)
        lim = F(2 ** 24)
        ok = ok & (u >= -lim) & (u <= lim) & (v >= -lim) & (v <= lim)
        u, v = np.where(ok, u, F(0)), np.where(ok, v, F(0))
        tzf = tz.astype(np.float32)
        band = dtol * tzf
        fu, fv = np.floor(u), np.floor(v)                                                                # step 3
        tx, ty = u - fu, v - fv
        bx, by = fu.astype(np.int64), fv.astype(np.int64)
        wx, wy = (F(1) - tx, tx), (F(1) - ty, ty)
        tap_ok = (h_len > 0) & np.isfinite(h_rgb).all(axis=2) & np.isfinite(h_m2) & np.isfinite(h_normal).all(axis=2) & np.isfinite(h_depth)
        sums = [np.zeros((h, w), np.float32) for _ in range(5)]
        values = [h_rgb[..., 0], h_rgb[..., 1], h_rgb[..., 2], h_m2, h_len]
        sumw = np.zeros((h, w), np.float32)
        for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)):                                                    # (i, j) = (0,0), (1,0), (0,1), (1,1)
            qx, qy = bx + i, by + j
            wt = wx[i] * wy[j]
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            jj, ii = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            d = h_normal[jj, ii] - normal
            dn = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
            take = ok & (wt != 0) & inside & tap_ok[jj, ii] & (np.abs(h_depth[jj, ii] - tzf) <= band) & (dn <= ntol)
            for s, val in zip(sums, values):
                s[...] = np.where(take, s + wt * val[jj, ii], s)
            sumw = np.where(take, sumw + wt, sumw)
        has = ok & (sumw > 0)
        hist = [s / sumw for s in sums]
        grown = hist[4] + F(1)                                                                           # step 4
        n = np.where(grown < most, grown, most)
        a = F(1) / n
        cur = [rgb[..., 0], rgb[..., 1], rgb[..., 2], cur_m2]
        blend = [hv + a * (cv - hv) for hv, cv in zip(hist[:4], cur)]
    assert all(b.dtype == np.float32 for b in blend) and n.dtype == np.float32
    for c in range(3):
        out_rgb[..., c][has] = blend[c].view(np.uint32)[has]
    out_m2[has] = blend[3][has]
    out_len[has] = n[has]
    return out_rgb.view(np.float32), out_m2, out_len


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
