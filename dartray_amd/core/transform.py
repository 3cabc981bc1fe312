"""lib/core/matrix4x4.dart and transform.dart: the reference's f32 matrices with its f64 term order, for the shapes, the lights and
the cameras."""
import math

import numpy as np


def _m4(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).reshape(4, 4)


def _mul(a, b):  # Matrix4x4.Mul: left-to-right f64 sums, f32 store (matrix4x4.dart:193-206)
    a, b = a.astype(np.float64), b.astype(np.float64)
    r = np.empty((4, 4), dtype=np.float64)
    for i in range(4):
        r[i] = a[i, 0] * b[0] + a[i, 1] * b[1] + a[i, 2] * b[2] + a[i, 3] * b[3]
    return r.astype(np.float32)


def _inv(a):
    """Matrix4x4.Inverse (matrix4x4.dart:212-214, 242-354): the reference's own formula -- cofactors over the determinant,
    every element ONE f64 expression in the reference's term order, stored f32; a singular matrix comes back unchanged.
    (A general-purpose inverse such as numpy.linalg.inv differs in the last bits and leaves 1e-17 where this leaves 0.)"""
    d = [float(v) for v in np.asarray(a, np.float32).reshape(-1)]
    # the reference names the elements column-wise: nRC = data[4 * (C - 1) + (R - 1)]
    n11, n12, n13, n14 = d[0], d[4], d[8], d[12]
    n21, n22, n23, n24 = d[1], d[5], d[9], d[13]
    n31, n32, n33, n34 = d[2], d[6], d[10], d[14]
    n41, n42, n43, n44 = d[3], d[7], d[11], d[15]
    det = ((n14 * n23 * n32 * n41) - (n13 * n24 * n32 * n41) - (n14 * n22 * n33 * n41) + (n12 * n24 * n33 * n41) +
           (n13 * n22 * n34 * n41) - (n12 * n23 * n34 * n41) - (n14 * n23 * n31 * n42) + (n13 * n24 * n31 * n42) +
           (n14 * n21 * n33 * n42) - (n11 * n24 * n33 * n42) - (n13 * n21 * n34 * n42) + (n11 * n23 * n34 * n42) +
           (n14 * n22 * n31 * n43) - (n12 * n24 * n31 * n43) - (n14 * n21 * n32 * n43) + (n11 * n24 * n32 * n43) +
           (n12 * n21 * n34 * n43) - (n11 * n22 * n34 * n43) - (n13 * n22 * n31 * n44) + (n12 * n23 * n31 * n44) +
           (n13 * n21 * n32 * n44) - (n11 * n23 * n32 * n44) - (n12 * n21 * n33 * n44) + (n11 * n22 * n33 * n44))
    if det == 0.0:
        return np.asarray(a, np.float32).reshape(4, 4).copy()
    i = 1.0 / det
    r = [0.0] * 16
    r[0] = (n23 * n34 * n42 - n24 * n33 * n42 + n24 * n32 * n43 - n22 * n34 * n43 - n23 * n32 * n44 + n22 * n33 * n44) * i
    r[4] = (n14 * n33 * n42 - n13 * n34 * n42 - n14 * n32 * n43 + n12 * n34 * n43 + n13 * n32 * n44 - n12 * n33 * n44) * i
    r[8] = (n13 * n24 * n42 - n14 * n23 * n42 + n14 * n22 * n43 - n12 * n24 * n43 - n13 * n22 * n44 + n12 * n23 * n44) * i
    r[12] = (n14 * n23 * n32 - n13 * n24 * n32 - n14 * n22 * n33 + n12 * n24 * n33 + n13 * n22 * n34 - n12 * n23 * n34) * i
    r[1] = (n24 * n33 * n41 - n23 * n34 * n41 - n24 * n31 * n43 + n21 * n34 * n43 + n23 * n31 * n44 - n21 * n33 * n44) * i
    r[5] = (n13 * n34 * n41 - n14 * n33 * n41 + n14 * n31 * n43 - n11 * n34 * n43 - n13 * n31 * n44 + n11 * n33 * n44) * i
    r[9] = (n14 * n23 * n41 - n13 * n24 * n41 - n14 * n21 * n43 + n11 * n24 * n43 + n13 * n21 * n44 - n11 * n23 * n44) * i
    r[13] = (n13 * n24 * n31 - n14 * n23 * n31 + n14 * n21 * n33 - n11 * n24 * n33 - n13 * n21 * n34 + n11 * n23 * n34) * i
    r[2] = (n22 * n34 * n41 - n24 * n32 * n41 + n24 * n31 * n42 - n21 * n34 * n42 - n22 * n31 * n44 + n21 * n32 * n44) * i
    r[6] = (n14 * n32 * n41 - n12 * n34 * n41 - n14 * n31 * n42 + n11 * n34 * n42 + n12 * n31 * n44 - n11 * n32 * n44) * i
    r[10] = (n12 * n24 * n41 - n14 * n22 * n41 + n14 * n21 * n42 - n11 * n24 * n42 - n12 * n21 * n44 + n11 * n22 * n44) * i
    r[14] = (n14 * n22 * n31 - n12 * n24 * n31 - n14 * n21 * n32 + n11 * n24 * n32 + n12 * n21 * n34 - n11 * n22 * n34) * i
    r[3] = (n23 * n32 * n41 - n22 * n33 * n41 - n23 * n31 * n42 + n21 * n33 * n42 + n22 * n31 * n43 - n21 * n32 * n43) * i
    r[7] = (n12 * n33 * n41 - n13 * n32 * n41 + n13 * n31 * n42 - n11 * n33 * n42 - n12 * n31 * n43 + n11 * n32 * n43) * i
    r[11] = (n13 * n22 * n41 - n12 * n23 * n41 - n13 * n21 * n42 + n11 * n23 * n42 + n12 * n21 * n43 - n11 * n22 * n43) * i
    r[15] = (n12 * n23 * n31 - n13 * n22 * n31 + n13 * n21 * n32 - n11 * n23 * n32 - n12 * n21 * n33 + n11 * n22 * n33) * i
    return np.asarray(r, dtype=np.float64).astype(np.float32).reshape(4, 4)


def _normalize(v):
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    return (v / math.sqrt(float(v @ v))).astype(np.float32)


def look_at(pos, look, up):
    """Transform.LookAt (transform.dart:301-329): returns camera-to-world."""
    pos = np.asarray(pos, np.float32)
    look = np.asarray(look, np.float32)
    d = _normalize((look.astype(np.float64) - pos.astype(np.float64)).astype(np.float32))
    upn = _normalize(up)
    left = _normalize(np.cross(upn.astype(np.float64), d.astype(np.float64)).astype(np.float32))
    new_up = np.cross(d.astype(np.float64), left.astype(np.float64)).astype(np.float32)
    m = np.eye(4, dtype=np.float32)
    m[:3, 0] = left
    m[:3, 1] = new_up
    m[:3, 2] = d
    m[:3, 3] = pos
    return m


def transform_points(m, P):
    """Transform.transformPoint (transform.dart:110-129) over an [n,3] array: the reference's left-to-right
    f64 sums (no fused multiply-add, which a BLAS matmul may use), stored f32; w != 1 divides (Point.invScale)."""
    m = np.asarray(m, np.float32).astype(np.float64).reshape(4, 4)
    P = np.asarray(P, np.float64).astype(np.float32).astype(np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    out = np.stack([m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3)], axis=1).astype(np.float32)
    w = m[3, 0] * x + m[3, 1] * y + m[3, 2] * z + m[3, 3]
    sel = w != 1.0
    if np.any(sel):
        out[sel] = (out[sel].astype(np.float64) / w[sel, None]).astype(np.float32)
    return out


def _bbox_transform(m, lo, hi):
    """Transform.transformBBox (transform.dart:163-178): union of the 8 transformed corners, f32."""
    m = np.asarray(m, np.float32).astype(np.float64)
    lo = np.asarray(lo, np.float64).astype(np.float32).astype(np.float64)  # Point(...) stores f32
    hi = np.asarray(hi, np.float64).astype(np.float32).astype(np.float64)
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)                         # BBox(p1, p2) bbox.dart:36-40
    corners = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)])
    pts = transform_points(m, corners)
    return pts.min(0), pts.max(0)
