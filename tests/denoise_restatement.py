"""The edge-avoiding a-trous filter restated in numpy from the text of DESIGN.md 2.15 (not from the C code): every operation is one
np.float32 operation on arrays, in the order the text writes it, so the result is compared with the library's bit for bit.

    atrous(rgb[h, w, 3], normal[h, w, 3], depth[h, w], iterations, k_color, k_normal, k_depth) -> [h, w, 3] float32
"""
import numpy as np

F = np.float32
_h = [F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16)]
H = np.array([[a * b for b in _h] for a in _h], dtype=np.float32)      # H[dy + 2][dx + 2]; the products are exact
assert np.array_equal(H * F(256), np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]).astype(np.float32))


def level_kc(k_color, i):
    """kc_i = (float)((double)k_color * 4^i)"""
    with np.errstate(over="ignore"):
        return F(np.float64(F(k_color)) * np.float64(4.0) ** i)


def _dist2(a, b):
    """((a0 - b0)^2 + (a1 - b1)^2) + (a2 - b2)^2"""
    d0, d1, d2 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return ((d0 * d0) + (d1 * d1)) + (d2 * d2)


def _shifted(a, ox, oy, fill):
    """b[y, x] = a[y + oy, x + ox] where that lies inside, else `fill`; and the mask of the inside."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    inside = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return out, inside


def one_level(colour, normal, depth, s, kc, kn, kz):
    colour, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (colour, normal, depth))
    kc, kn, kz, one = F(kc), F(kn), F(kz), F(1)
    valid = np.isfinite(colour).all(axis=2) & np.isfinite(normal).all(axis=2) & np.isfinite(depth)
    total = np.zeros(colour.shape, np.float32)
    sumw = np.zeros(depth.shape, np.float32)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, inside = _shifted(colour, dx * s, dy * s, 0)
                nq = _shifted(normal, dx * s, dy * s, 0)[0]
                zq = _shifted(depth, dx * s, dy * s, 0)[0]
                take = inside & _shifted(valid, dx * s, dy * s, False)[0]
                if not take.any():
                    continue
                dc, dn = _dist2(cq, colour), _dist2(nq, normal)
                dz = (zq - depth) * (zq - depth)
                wt = np.full(depth.shape, H[dy + 2][dx + 2], np.float32)
                if kc != 0:
                    wt = wt / (one + kc * dc)
                if kn != 0:
                    wt = wt / (one + kn * dn)
                if kz != 0:
                    wt = wt / (one + kz * dz)
                total = np.where(take[..., None], total + wt[..., None] * cq, total)
                sumw = np.where(take, sumw + wt, sumw)
        out = total / sumw[..., None]
    assert out.dtype == np.float32
    # a pixel that is not valid keeps its input colour bit for bit (copied as integers: no operation touches a NaN's payload)
    res = colour.copy().view(np.uint32)
    res[valid] = out.view(np.uint32)[valid]
    return res.view(np.float32)


def atrous(rgb, normal, depth, iterations, k_color, k_normal, k_depth):
    cur = np.ascontiguousarray(rgb, np.float32)
    for i in range(iterations):
        cur = one_level(cur, normal, depth, 1 << i, level_kc(k_color, i), k_normal, k_depth)
    return cur


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
