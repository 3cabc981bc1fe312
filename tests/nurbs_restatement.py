"""DESIGN.md 2.21 (Shape "nurbs") restated in plain Python: Nurbs.refine, NurbsEvaluateSurface, NurbsEvaluate and KnotOffset
(shapes/nurbs.dart:76-263) line by line in the reference's own list style -- a Float32List is a list whose stores round to numpy.float32
and whose indices are checked like Dart's (a negative or too large index raises RangeError; numpy and Python would wrap a negative one
silently), Vector / Point / Normal components store f32 (vector.dart:27-34), every expression is a Python float (f64).  Written apart
from dartray_amd/csrc/dr_nurbs.h: it shares no code with it.  Cited by file.dart:line of the reference.

Two index expressions of the text are NOT restated but repaired, each marked REPAIRED where it stands (DESIGN.md 2.21 has the reasons):
  :208       j = cpi + ((cpOffset + i) * cpStride), i counting floats, cpOffset points: beyond the first knot span the iso call of :178
             indexes at -3 * uFirstCp, a RangeError in Dart.  Here (cpOffset * 4 + i): the same index wherever the text does not raise.
  :222-225   cpWork[j + c], the point's NUMBER, as the de Boor step's left operand.  Here cpWork[k + c]: the B-spline recurrence.
With REPAIRED = False the module is the text as it stands; tests/test_nurbs.py shows on it what the two lines do.
"""
import math

import numpy as np

REPAIRED = True


class RangeError(IndexError):
    """Dart's RangeError of a list index out of range."""


class Float32List:
    def __init__(self, n):
        self.d = [0.0] * n

    @staticmethod
    def of(values):
        l = Float32List(len(values))
        for i, v in enumerate(values):
            l[i] = v
        return l

    def __len__(self):
        return len(self.d)

    def _at(self, i):
        if not 0 <= i < len(self.d):
            raise RangeError("index %d out of range 0..%d" % (i, len(self.d) - 1))
        return i

    def __getitem__(self, i):
        return self.d[self._at(i)]

    def __setitem__(self, i, v):
        self.d[self._at(i)] = float(np.float32(v))


class Vector:                                                       # vector.dart:26-34: a Float32List of 3
    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.data = Float32List.of([x, y, z])

    x = property(lambda s: s.data[0], lambda s, v: s.data.__setitem__(0, v))
    y = property(lambda s: s.data[1], lambda s, v: s.data.__setitem__(1, v))
    z = property(lambda s: s.data[2], lambda s, v: s.data.__setitem__(2, v))


def _div(a, b):
    """Dart's double division: x / 0.0 is an infinity or NaN, never an exception."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def Cross(v1, v2):                                                  # vector.dart:158-168
    v1x, v1y, v1z, v2x, v2y, v2z = v1.data[0], v1.data[1], v1.data[2], v2.data[0], v2.data[1], v2.data[2]
    return Vector((v1y * v2z) - (v1z * v2y), (v1z * v2x) - (v1x * v2z), (v1x * v2y) - (v1y * v2x))


def NormalNormalize(n):                                             # normal.dart:55-57, :35-38; vector.dart:80-83, :92-97
    out = Vector(n.data[0], n.data[1], n.data[2])
    s = math.sqrt(out.data[0] * out.data[0] + out.data[1] * out.data[1] + out.data[2] * out.data[2])
    out.data[0] = _div(out.data[0], s)
    out.data[1] = _div(out.data[1], s)
    out.data[2] = _div(out.data[2], s)
    return out


def Lerp(t, v1, v2):                                                # common.dart:80-81
    return v1 * (1.0 - t) + v2 * t


def KnotOffset(knot, order, np_, t):                                # :253-263
    firstKnot = order - 1
    knotOffset = firstKnot
    while t > knot[knotOffset + 1]:
        knotOffset += 1
    return knotOffset


def NurbsEvaluate(order, knot, cp, cpi, np_, cpStride, t, deriv=None):  # :197-251
    knotOffset = KnotOffset(knot, order, np_, t)
    cpOffset = knotOffset - order + 1
    cpWork = Float32List(4 * order)
    i = 0
    while i < len(cpWork):
        j = cpi + (((cpOffset * 4 if REPAIRED else cpOffset) + i) * cpStride)   # REPAIRED (:208)
        for _ in range(4):
            cpWork[i] = cp[j]
            i += 1
            j += 1
    for i in range(order - 2):
        j, k, l = 0, 0, 4
        while j < order - 1 - i:
            alpha = _div(knot[knotOffset + 1 + j] - t, knot[knotOffset + 1 + j] - knot[knotOffset + j + 2 - order + i])
            m = k if REPAIRED else j                                # REPAIRED (:222-225): the text has cpWork[j + c]
            cpWork[k] = cpWork[m] * alpha + cpWork[l] * (1 - alpha)
            cpWork[k + 1] = cpWork[m + 1] * alpha + cpWork[l + 1] * (1 - alpha)
            cpWork[k + 2] = cpWork[m + 2] * alpha + cpWork[l + 2] * (1 - alpha)
            cpWork[k + 3] = cpWork[m + 3] * alpha + cpWork[l + 3] * (1 - alpha)
            j, k, l = j + 1, k + 4, l + 4
    alpha = _div(knot[knotOffset + 1] - t, knot[knotOffset + 1] - knot[knotOffset + 0])
    vx = cpWork[0] * alpha + cpWork[4] * (1 - alpha)
    vy = cpWork[1] * alpha + cpWork[5] * (1 - alpha)
    vz = cpWork[2] * alpha + cpWork[6] * (1 - alpha)
    vw = cpWork[3] * alpha + cpWork[7] * (1 - alpha)
    if deriv is not None:
        factor = _div(order - 1, knot[knotOffset + 1] - knot[knotOffset])
        dx = (cpWork[4] - cpWork[0]) * factor
        dy = (cpWork[5] - cpWork[1]) * factor
        dz = (cpWork[6] - cpWork[2]) * factor
        dw = (cpWork[7] - cpWork[3]) * factor
        deriv.x = _div(dx, vw) - _div(vx * dw, vw * vw)
        deriv.y = _div(dy, vw) - _div(vy * dw, vw * vw)
        deriv.z = _div(dz, vw) - _div(vz * dw, vw * vw)
    return [vx, vy, vz, vw]


def NurbsEvaluateSurface(uOrder, uKnot, ucp, u, vOrder, vKnot, vcp, v, cp, dPdu, dPdv):  # :156-195
    iso = Float32List(max(uOrder, vOrder) * 4)
    uOffset = KnotOffset(uKnot, uOrder, ucp, u)
    uFirstCp = uOffset - uOrder + 1
    j = 0
    for i in range(uOrder):
        pt = NurbsEvaluate(vOrder, vKnot, cp, (uFirstCp + i) * 4, vcp, ucp, v)
        for c in range(4):
            iso[j] = pt[c]
            j += 1
    vOffset = KnotOffset(vKnot, vOrder, vcp, v)
    vFirstCp = vOffset - vOrder + 1
    P = NurbsEvaluate(uOrder, uKnot, iso, (-uFirstCp) * 4, ucp, 1, u, dPdu)
    j = 0
    for i in range(vOrder):
        pt = NurbsEvaluate(uOrder, uKnot, cp, ((vFirstCp + i) * ucp) * 4, ucp, 1, u)
        for c in range(4):
            iso[j] = pt[c]
            j += 1
    NurbsEvaluate(vOrder, vKnot, iso, -vFirstCp * 4, vcp, 1, v, dPdv)
    return Vector(_div(P[0], P[3]), _div(P[1], P[3]), _div(P[2], P[3]))


def refine(nu, uorder, uknot, umin, umax, nv, vorder, vknot, vmin, vmax, P, isHomogeneous, diceu=30, dicev=30):
    """:76-154 with the dice rates as parameters: (P [n, 3], N [n, 3], uv [n, 2], indices [ntris, 3]) as numpy arrays.  The inputs are
    the f32 values the C ABI carries."""
    f = lambda a: [float(np.float32(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]
    uknot, vknot, P = f(uknot), f(vknot), f(P)
    umin, umax, vmin, vmax = f([umin, umax, vmin, vmax])
    ueval, veval = Float32List(diceu), Float32List(dicev)
    for i in range(diceu):
        ueval[i] = Lerp(i / (diceu - 1), umin, umax)
    for i in range(dicev):
        veval[i] = Lerp(i / (dicev - 1), vmin, vmax)
    uvs = Float32List(2 * diceu * dicev)
    Pw = Float32List.of(P)
    if not isHomogeneous:
        Pw = Float32List(nu * nv * 4)
        pi = wi = 0
        for i in range(nu * nv):
            for _ in range(3):
                Pw[wi] = P[pi]
                wi, pi = wi + 1, pi + 1
            Pw[wi] = 1.0
            wi += 1
    evalPs, evalNs = [], []
    pi = 0
    for v in range(dicev):
        for u in range(diceu):
            uvs[2 * pi] = ueval[u]
            uvs[2 * pi + 1] = veval[v]
            dPdu, dPdv = Vector(), Vector()
            pt = NurbsEvaluateSurface(uorder, uknot, nu, ueval[u], vorder, vknot, nv, veval[v], Pw, dPdu, dPdv)
            evalPs.append(pt)
            evalNs.append(NormalNormalize(Cross(dPdu, dPdv)))
            pi += 1
    vertices = []
    VN = lambda u, v: v * diceu + u
    for v in range(dicev - 1):
        for u in range(diceu - 1):
            vertices += [VN(u, v), VN(u + 1, v), VN(u + 1, v + 1)]
            vertices += [VN(u, v), VN(u + 1, v + 1), VN(u, v + 1)]
    return (np.array([p.data.d for p in evalPs], np.float32), np.array([n.data.d for n in evalNs], np.float32),
            np.array(uvs.d, np.float32).reshape(-1, 2), np.array(vertices, np.uint32).reshape(-1, 3))
