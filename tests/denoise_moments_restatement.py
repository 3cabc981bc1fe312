"""The variance-guided a-trous filter over a temporal history restated in numpy from the text of DESIGN.md 2.24 (not from the C code): every
operation is one np.float32 operation on arrays, in the order the text writes it, so the result is compared with the library's bit for bit.

    pack(rgb[h, w, 3], m2[h, w], len[h, w], normal[h, w, 3], depth[h, w]) -> n[h, w]              the history length, -1: not valid
    estimate(rgb, m2, n, normal, depth, min_history, radius, k_normal, k_depth) -> v[h, w]        the first variance, -1: not valid
    planes(rgb, m2, len, normal, depth, iterations, k_color, k_normal, k_depth, var_floor, min_history, radius)
                                                           -> [(rgb, v) after the estimate, after level 0, 1, ...]
    denoise_moments(...the same arguments...) -> (out[h, w, 3], out_var[h, w], out_var0[h, w])

The levels are 2.19's: one_level of tests/denoise_pair_restatement.py.  The shifted views and the squared distance are those of
tests/denoise_restatement.py.
"""
import numpy as np

from denoise_pair_restatement import _dist2, _shifted, lum, one_level, same_bits  # noqa: F401

F = np.float32


def pack(rgb, m2, length, normal, depth):
    rgb, m2, length, normal, depth = (np.ascontiguousarray(x, np.float32) for x in (rgb, m2, length, normal, depth))
    with np.errstate(invalid="ignore"):
        valid = (np.isfinite(rgb).all(axis=2) & np.isfinite(m2) & np.isfinite(length) & np.isfinite(normal).all(axis=2) & np.isfinite(depth)
                 & (length > 0))
    return np.where(valid, length, F(-1)).astype(np.float32)


def estimate(rgb, m2, n, normal, depth, min_history, radius, kn, kz):
    rgb, m2, n, normal, depth = (np.ascontiguousarray(x, np.float32) for x in (rgb, m2, n, normal, depth))
    kn, kz, one, zero = F(kn), F(kz), F(1), F(0)
    valid = n >= 0
    with np.errstate(all="ignore"):
        l = lum(rgb)
        # the temporal estimate
        d = m2 - l * l
        vt = np.where(d < 0, zero, d) / (n - one)
        # the spatial estimate: dy outer, dx inner
        s1 = np.zeros(n.shape, np.float32)
        s2 = np.zeros(n.shape, np.float32)
        sw = np.zeros(n.shape, np.float32)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                lq, inside = _shifted(l, dx, dy, 0)
                nq = _shifted(n, dx, dy, -1)[0]
                gq = _shifted(normal, dx, dy, 0)[0]
                zq = _shifted(depth, dx, dy, 0)[0]
                take = inside & (nq >= 0)
                if not take.any():
                    continue
                dn = _dist2(gq, normal)
                dd = zq - depth
                dz = dd * dd
                wt = np.full(n.shape, one, np.float32)
                if kn != 0:
                    wt = wt / (one + kn * dn)
                if kz != 0:
                    wt = wt / (one + kz * dz)
                s1 = np.where(take, s1 + wt * lq, s1)
                s2 = np.where(take, s2 + wt * (lq * lq), s2)
                sw = np.where(take, sw + wt, sw)
        mean = s1 / sw
        e = s2 / sw - mean * mean
        vs = np.where(e < 0, zero, e)
        v = np.where(n >= F(min_history), vt, vs)
    assert v.dtype == np.float32
    return np.where(valid & np.isfinite(v), v, F(-1)).astype(np.float32)


def planes(rgb, m2, length, normal, depth, iterations, k_color, k_normal, k_depth, var_floor, min_history, radius):
    rgb = np.ascontiguousarray(rgb, np.float32)
    n = pack(rgb, m2, length, normal, depth)
    cur = (rgb, estimate(rgb, m2, n, normal, depth, min_history, radius, k_normal, k_depth))
    out = [cur]
    for i in range(iterations):
        cur = one_level(cur[0], cur[1], normal, depth, 1 << i, k_color, k_normal, k_depth, var_floor)
        out.append(cur)
    return out


def denoise_moments(rgb, m2, length, normal, depth, iterations, k_color, k_normal, k_depth, var_floor, min_history, radius):
    levels = planes(rgb, m2, length, normal, depth, iterations, k_color, k_normal, k_depth, var_floor, min_history, radius)
    return levels[-1][0], levels[-1][1], levels[0][1]
