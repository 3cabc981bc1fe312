"""The variance-guided a-trous filter over two half renders restated in numpy from the text of DESIGN.md 2.19 (not from the C code): every
operation is one np.float32 operation on arrays, in the order the text writes it, so the result is compared with the library's bit for bit.

    pack(a[h, w, 3], b[h, w, 3], normal[h, w, 3], depth[h, w]) -> (m[h, w, 3], v[h, w])          v = -1: not valid
    one_level(m, v, normal, depth, s, k_color, k_normal, k_depth, var_floor) -> (m, v)
    planes(a, b, normal, depth, iterations, k_color, k_normal, k_depth, var_floor) -> [(m, v) after the pack, after level 0, 1, ...]
    denoise_pair(...the same arguments...) -> the last of them: (out[h, w, 3], out_var[h, w])

The tap table H, the shifted views and the squared distance are those of tests/denoise_restatement.py (2.15's, which 2.19 keeps).
"""
import numpy as np

from denoise_restatement import H, _dist2, _shifted, same_bits  # noqa: F401

F = np.float32
LR, LG, LB = F(0.212671), F(0.715160), F(0.072169)
_g = [F(1) / F(4), F(1) / F(2), F(1) / F(4)]
G = np.array([[a * b for b in _g] for a in _g], dtype=np.float32)      # G[dy + 1][dx + 1]; the products are exact
assert np.array_equal(G * F(16), np.outer([1, 2, 1], [1, 2, 1]).astype(np.float32))
QUIET_NAN = np.uint32(0x7fc00000)


def lum(c):
    """(0.212671 * r + 0.715160 * g) + 0.072169 * b"""
    return (LR * c[..., 0] + LG * c[..., 1]) + LB * c[..., 2]


def pack(a, b, normal, depth):
    a, b, normal, depth = (np.ascontiguousarray(x, np.float32) for x in (a, b, normal, depth))
    with np.errstate(all="ignore"):
        m = F(0.5) * (a + b)
        bits = m.view(np.uint32).copy()
        bits[np.isnan(m)] = QUIET_NAN                                  # a NaN mean is the one quiet NaN
        m = bits.view(np.float32)
        ld = lum(a - b)
        v0 = F(0.25) * (ld * ld)
    valid = np.isfinite(m).all(axis=2) & np.isfinite(v0) & np.isfinite(normal).all(axis=2) & np.isfinite(depth)
    v = np.where(valid, v0, F(-1)).astype(np.float32)
    assert m.dtype == np.float32 and v0.dtype == np.float32
    return m, v


def prefiltered(v):
    """vp: the 3 x 3 binomial mean of the variance over the taps inside the image that are valid (dy outer, dx inner)."""
    sumgv = np.zeros(v.shape, np.float32)
    sumg = np.zeros(v.shape, np.float32)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                vq, inside = _shifted(v, dx, dy, -1)
                take = inside & (vq >= 0)
                g = G[dy + 1][dx + 1]
                sumgv = np.where(take, sumgv + g * vq, sumgv)
                sumg = np.where(take, sumg + g, sumg)
        return sumgv / sumg


def one_level(colour, v, normal, depth, s, kc, kn, kz, var_floor):
    colour, v, normal, depth = (np.ascontiguousarray(x, np.float32) for x in (colour, v, normal, depth))
    kc, kn, kz, one = F(kc), F(kn), F(kz), F(1)
    valid = v >= 0
    total = np.zeros(colour.shape, np.float32)
    sumv = np.zeros(v.shape, np.float32)
    sumw = np.zeros(v.shape, np.float32)
    with np.errstate(all="ignore"):
        den = prefiltered(v) + F(var_floor)
        colour_term = np.isfinite(den) if kc != 0 else np.zeros(v.shape, bool)
        lp = lum(colour)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, inside = _shifted(colour, dx * s, dy * s, 0)
                vq = _shifted(v, dx * s, dy * s, -1)[0]
                nq = _shifted(normal, dx * s, dy * s, 0)[0]
                zq = _shifted(depth, dx * s, dy * s, 0)[0]
                take = inside & (vq >= 0)
                if not take.any():
                    continue
                dl = lum(cq) - lp
                dc = dl * dl
                dn = _dist2(nq, normal)
                dz = (zq - depth) * (zq - depth)
                wt = np.full(v.shape, H[dy + 2][dx + 2], np.float32)
                wt = np.where(colour_term, wt / (one + kc * (dc / den)), wt)
                if kn != 0:
                    wt = wt / (one + kn * dn)
                if kz != 0:
                    wt = wt / (one + kz * dz)
                total = np.where(take[..., None], total + wt[..., None] * cq, total)
                sumv = np.where(take, sumv + (wt * wt) * vq, sumv)
                sumw = np.where(take, sumw + wt, sumw)
        out = total / sumw[..., None]
        vout = sumv / (sumw * sumw)
    assert out.dtype == np.float32 and vout.dtype == np.float32
    vnew = np.where(np.isfinite(out).all(axis=2) & np.isfinite(vout), vout, F(-1)).astype(np.float32)
    # a pixel that is not valid keeps its texel bit for bit (copied as integers: no operation touches a NaN's payload)
    res = colour.copy().view(np.uint32)
    res[valid] = out.view(np.uint32)[valid]
    return res.view(np.float32), np.where(valid, vnew, v).astype(np.float32)


def planes(a, b, normal, depth, iterations, k_color, k_normal, k_depth, var_floor):
    cur = pack(a, b, normal, depth)
    out = [cur]
    for i in range(iterations):
        cur = one_level(cur[0], cur[1], normal, depth, 1 << i, k_color, k_normal, k_depth, var_floor)
        out.append(cur)
    return out


def denoise_pair(a, b, normal, depth, iterations, k_color, k_normal, k_depth, var_floor):
    return planes(a, b, normal, depth, iterations, k_color, k_normal, k_depth, var_floor)[-1]
