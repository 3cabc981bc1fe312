"""Firefly suppression restated in numpy from the text of DESIGN.md 2.25 (not from the C code): one np.float32 operation per operator on
whole arrays, in the order the text writes them, so the result is compared with the library's bit for bit.

    firefly(rgb[h, w, 3], normal[h, w, 3], depth[h, w], radius, rank, threshold, floor, depth_tol, normal_tol)
        -> (out [h, w, 3], removed [h, w]) float32

    members(...) -> (n [h, w] int, lums [taps, h, w] float32 with -inf where the tap is no member): steps 1 and 2 alone
"""
import numpy as np

F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def lum(rgb):
    """(0.212671 r + 0.715160 g) + 0.072169 b"""
    return (F(0.212671) * rgb[..., 0] + F(0.715160) * rgb[..., 1]) + F(0.072169) * rgb[..., 2]


def valid(rgb, normal, depth):
    """Step 1: the three colour values, the three normal values, the depth and the luminance are finite."""
    with np.errstate(all="ignore"):
        return np.isfinite(rgb).all(axis=2) & np.isfinite(normal).all(axis=2) & np.isfinite(depth) & np.isfinite(lum(rgb))


def _shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the image, else `fill`"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
    xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    return out


def members(rgb, normal, depth, radius, depth_tol, normal_tol):
    rgb, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb, normal, depth))
    ok = valid(rgb, normal, depth)
    with np.errstate(all="ignore"):
        l = lum(rgb)
        band = F(depth_tol) * depth                                      # computed once per pixel p
        lums = []
        for dy in range(-radius, radius + 1):                            # rows ascending, then columns
            for dx in range(-radius, radius + 1):
                if dx == 0 and dy == 0:
                    continue
                q_ok = _shifted(ok, dx, dy, False)                       # inside the image and valid
                zq, nq, lq = _shifted(depth, dx, dy, F(0)), _shifted(normal, dx, dy, F(0)), _shifted(l, dx, dy, F(0))
                near = np.abs(zq - depth) <= band                        # a NaN fails
                d = nq - normal
                alike = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2]) <= F(normal_tol)
                member = ok & q_ok & near & alike
                lums.append(np.where(member, lq, F(-np.inf)))
    lums = np.stack(lums).astype(np.float32)
    return (lums > F(-np.inf)).sum(axis=0), lums


def firefly(rgb, normal, depth, radius, rank, threshold, floor, depth_tol, normal_tol):
    rgb, normal, depth = (np.ascontiguousarray(a, np.float32) for a in (rgb, normal, depth))
    n, lums = members(rgb, normal, depth, radius, depth_tol, normal_tol)
    ok = valid(rgb, normal, depth)
    with np.errstate(all="ignore"):
        l = lum(rgb)
        m = -np.sort(-lums, axis=0)[rank - 1]                            # the rank-th largest, counted with multiplicity
        t = F(threshold) * m + F(floor)
        t0 = np.where(t > 0, t, F(0)).astype(np.float32)                 # one zero, whatever the sign of a zero m
        clamp = ok & (n >= rank) & (l > t0)
        s = t0 / l
        out = np.where(clamp[..., None], rgb * s[..., None], rgb).astype(np.float32)
        removed = np.where(clamp, l - t0, F(0)).astype(np.float32)
    # np.where copies the unselected elements' bits; make that explicit for the non-finite ones
    keep = ~clamp
    out.view(np.uint32)[keep] = rgb.view(np.uint32)[keep]
    return out, removed
