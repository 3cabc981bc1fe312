"""The joint bilateral upsampler restated in numpy from the text of DESIGN.md 2.22 (not from the C code): every operation is one np.float32
operation on arrays, in the order the text writes it, so the result is compared with the library's bit for bit.

    upsample(rgb_lo[hl, wl, 3], normal_lo[hl, wl, 3], depth_lo[hl, wl], normal[h, w, 3], depth[h, w], factor, taps, k_normal, k_depth)
        -> [h, w, 3] float32
"""
import numpy as np

F = np.float32


def _dist2(a, b):
    """((a0 - b0)^2 + (a1 - b1)^2) + (a2 - b2)^2"""
    d0, d1, d2 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return ((d0 * d0) + (d1 * d1)) + (d2 * d2)


def upsample(rgb_lo, normal_lo, depth_lo, normal, depth, factor, taps, k_normal, k_depth):
    rgb_lo, normal_lo, depth_lo, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb_lo, normal_lo, depth_lo, normal, depth))
    hl, wl = depth_lo.shape
    f, r = int(factor), int(taps) // 2
    h, w = f * hl, f * wl
    assert depth.shape == (h, w) and normal.shape == (h, w, 3)
    kn, kz, one, half, ff, rf = F(k_normal), F(k_depth), F(1), F(0.5), F(f), F(r)
    valid_lo = np.isfinite(rgb_lo).all(axis=2) & np.isfinite(normal_lo).all(axis=2) & np.isfinite(depth_lo)
    edges = np.isfinite(normal).all(axis=2) & np.isfinite(depth)          # step 4: the pixel's own guide is finite
    xs, ys = np.arange(w), np.arange(h)
    u = (xs.astype(np.float32) + half) / ff - half                        # step 1
    v = (ys.astype(np.float32) + half) / ff - half
    bx, by = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    total = np.zeros((h, w, 3), np.float32)
    sumw = np.zeros((h, w), np.float32)
    with np.errstate(all="ignore"):
        for dj in range(-r + 1, r + 1):                                   # step 2: rows outside, columns inside
            j = by + dj
            wy = one - np.abs(v - j.astype(np.float32)) / rf
            for di in range(-r + 1, r + 1):
                i = bx + di
                wx = one - np.abs(u - i.astype(np.float32)) / rf
                inside = ((j >= 0) & (j < hl))[:, None] & ((i >= 0) & (i < wl))[None, :]
                jj, ii = np.clip(j, 0, hl - 1)[:, None], np.clip(i, 0, wl - 1)[None, :]
                take = inside & valid_lo[jj, ii]
                if not take.any():
                    continue
                cq, nq, zq = rgb_lo[jj, ii], normal_lo[jj, ii], depth_lo[jj, ii]
                wt = wx[None, :] * wy[:, None]                            # step 3
                dn = _dist2(nq, normal)                                   # step 4
                dd = zq - depth
                dz = dd * dd
                we = wt
                if kn != 0:
                    we = we / (one + kn * dn)
                if kz != 0:
                    we = we / (one + kz * dz)
                wt = np.where(edges, we, wt)
                total = np.where(take[..., None], total + wt[..., None] * cq, total)      # step 5
                sumw = np.where(take, sumw + wt, sumw)
        out = total / sumw[..., None]                                     # step 6
    assert out.dtype == np.float32 and sumw.dtype == np.float32
    # step 7: sumw == 0 -- the colour of low pixel (x / f, y / f), copied as integers: no operation touches a NaN's payload
    res = out.view(np.uint32).copy()
    near = rgb_lo.view(np.uint32)[(ys // f)[:, None], (xs // f)[None, :]]
    fallback = sumw == 0
    res[fallback] = near[fallback]
    return res.view(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
