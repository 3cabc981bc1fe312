"""The patches of tests/test_nurbs.py, tests/test_gpu_nurbs.py, each small, as keyword arguments of core.nurbs_dice
(and, through restated(), of tests/nurbs_restatement.refine).  CASES hold no NaN; NAN_CASES is the degenerate pole; REFUSALS: one input
per refusal of include/dartray_hip.h."""
import functools
import math

import numpy as np

F = np.float32
RATES = [(30, 30), (2, 2), (65, 3), (3, 257)]  # the reference's rate; the least; rows that are no multiple of a wave; a tail wave


def _clamped(order):
    return [0.0] * order + [1.0] * order


def _net(nu, nv, seed):
    """A gently curved nu x nv net over [0, 3] x [0, 2], u fastest: heights from a seeded generator, every value an f32."""
    rng = np.random.RandomState(seed)
    P = np.empty((nv, nu, 3), np.float32)
    for j in range(nv):
        for i in range(nu):
            P[j, i] = (3.0 * i / (nu - 1), 2.0 * j / (nv - 1), rng.uniform(-0.5, 0.5))
    return P.reshape(-1, 3)


def _patch(nu, uorder, uknots, nv, vorder, vknots, u=None, v=None, **cp):
    u = (uknots[uorder - 1], uknots[nu]) if u is None else u
    v = (vknots[vorder - 1], vknots[nv]) if v is None else v
    return dict(nu=nu, uorder=uorder, uknots=uknots, u0=u[0], u1=u[1], nv=nv, vorder=vorder, vknots=vknots, v0=v[0], v1=v[1], **cp)


R, H, W = 2.0, 3.0, float(F(math.sqrt(2.0) / 2.0))
_MULTI_U, _MULTI_V = [0, 0, 0, 0, 1, 2, 3, 3, 3, 3], [0, 0, 0, 1, 2, 3, 3, 3]
_DOUBLE = [0, 0, 0, 0.25, 0.25, 1, 1, 1]  # non-uniform, the interior knot 0.25 of multiplicity order - 1 = 2
_POLE = _net(4, 4, 5)
_POLE[:4] = (1.0, 1.0, 1.0)  # the row v = 0 is one point: dPdu is 0 there, the cross product too

CASES = {
    # z = x / 2 + y / 4
    "bilinear": _patch(2, 2, _clamped(2), 2, 2, _clamped(2), P=[[0, 0, 0], [2, 0, 1], [0, 4, 1], [2, 4, 2]]),
    "bezier_bicubic": _patch(4, 4, _clamped(4), 4, 4, _clamped(4), P=_net(4, 4, 1)),
    # several spans, mixed order; diced 4 x 4 as well, u = 0, 1, 2, 3: u = 1.0 and u = 2.0 lie exactly on interior knots (KnotOffset's `>`)
    "multi_span_mixed_order": _patch(6, 4, _MULTI_U, 5, 3, _MULTI_V, P=_net(6, 5, 2)),
    "double_interior_knot": _patch(5, 3, _DOUBLE, 5, 3, _DOUBLE, P=_net(5, 5, 3)),
    # a quarter cylinder of radius R about z: the arc's three points with weights 1, sqrt(2) / 2, 1, times two heights
    "rational_quarter_cylinder": _patch(3, 3, _clamped(3), 2, 2, _clamped(2),
                                        Pw=[[R, 0, 0, 1], [R * W, R * W, 0, W], [0, R, 0, 1],
                                            [R, 0, H, 1], [R * W, R * W, H * W, W], [0, R, H, 1]]),
    "sub_range": _patch(4, 4, _clamped(4), 4, 4, _clamped(4), u=(0.25, 0.75), v=(0.125, 0.5), P=_net(4, 4, 1)),
    "order_8": _patch(8, 8, _clamped(8), 8, 8, _clamped(8), P=_net(8, 8, 4)),
}
NAN_CASES = {"degenerate_pole": _patch(4, 4, _clamped(4), 4, 4, _clamped(4), P=_POLE)}
EXTRA_RATES = {"multi_span_mixed_order": [(4, 4)]}

def _bad(message, **changes):
    p = dict(CASES["bezier_bicubic"])
    p.update(changes)
    return p, message


REFUSALS = {
    "uorder_1": _bad("uorder is below 2 or above DR_NURBS_MAX_ORDER", uorder=1, uknots=[0, 0, 0, 1, 1]),
    "vorder_9": _bad("vorder is below 2 or above DR_NURBS_MAX_ORDER", vorder=9, vknots=[0] * 6 + [1] * 7),
    "nu_below_uorder": _bad("nu is below uorder", nu=3, uknots=[0, 0, 0, 0, 1, 1, 1], P=_net(3, 4, 1)),
    "nv_below_vorder": _bad("nv is below vorder", nv=3, vknots=[0, 0, 0, 0, 1, 1, 1], P=_net(4, 3, 1)),
    "decreasing_knots": _bad("the u knot vector decreases", uknots=[0, 0, 0, 0, 1, 1, 0.5, 1]),
    "nan_knot": _bad("a v knot is not finite", vknots=[0, 0, 0, 0, 1, 1, 1, float("nan")]),
    "infinite_knot": _bad("a u knot is not finite", uknots=[0, 0, 0, 0, 1, 1, 1, float("inf")]),
    "u0_below": _bad(r"u0 or u1 is outside \[uknots\[uorder - 1\], uknots\[nu\]\]", u0=-0.125),
    "u1_above": _bad(r"u0 or u1 is outside", u1=1.5),
    "v0_nan": _bad(r"v0 or v1 is outside \[vknots\[vorder - 1\], vknots\[nv\]\]", v0=float("nan")),
    "v1_above": _bad(r"v0 or v1 is outside", v1=2.0),
    "diceu_1": _bad("diceu or dicev is below 2 or above 4096", diceu=1),
    "dicev_4097": _bad("diceu or dicev is below 2 or above 4096", dicev=4097),
    "dice_product": _bad("diceu [*] dicev is above 2\\^22", diceu=4096, dicev=2048),
}


def rates(name):
    return RATES + EXTRA_RATES.get(name, [])


def every_case():
    """(name, keyword arguments, diceu, dicev) of every patch, at every rate"""
    for group in (CASES, NAN_CASES):
        for name in sorted(group):
            for du, dv in rates(name):
                yield name, group[name], du, dv


@functools.lru_cache(maxsize=None)
def restated(name, diceu, dicev):
    """tests/nurbs_restatement.refine of one case, computed once and shared: (P, N, uv, indices), read-only"""
    import nurbs_restatement
    kw = dict(CASES.get(name) or NAN_CASES[name])
    cp = kw.pop("P", None)
    homogeneous = cp is None
    cp = kw.pop("Pw") if homogeneous else cp
    out = nurbs_restatement.refine(kw["nu"], kw["uorder"], kw["uknots"], kw["u0"], kw["u1"], kw["nv"], kw["vorder"], kw["vknots"], kw["v0"],
                                   kw["v1"], np.asarray(cp, np.float32), homogeneous, diceu, dicev)
    for a in out:
        a.setflags(write=False)
    return out


def same_bits_or_both_nan(a, b):
    """Byte-identical f32 arrays, except that a NaN matches any NaN (x86 and the GPU may disagree on a NaN's sign and payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
