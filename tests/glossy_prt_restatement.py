"""GlossyPRTIntegrator (surface_integrators/glossy_prt_integrator.dart) and what it uses of core/spherical_harmonics.dart -- ComputeTransferMatrix,
ComputeBSDFMatrix, MatrixVectorMultiply, Rotate, RotateZ, RotateXPlus, RotateXMinus, _toZYZ -- with Microfacet / Blinn (microfacet.dart, blinn.dart),
restated in plain Python from the Dart text on top of tests/prt_restatement.py (Evaluate, the projection, the scene walk, getBSDF).

Object identity is kept: a Spectrum is a Python object (RGB), a Dart list is a Python list of references, `c_out[i] = c_in[j]` binds the same object,
`.copy(..)` and `.scale(..)` write INTO an object.  Whatever aliasing the reference's Rotate has therefore happens here by itself."""
import math

import numpy as np

import prt_restatement as prt
from prt_restatement import F32, F64, RGB, Evaluate, EvaluateMany, Index, Sample02, Terms, UniformSampleSphere, Vec, dr, f32  # noqa: F401

FLT_EPSILON = 1.19209290e-07                                       # common.dart:27
INV_TWOPI = 0.15915494309189533577                                 # common.dart:24


# ---- Spectrum methods that write into the object (spectrum / rgb_color.dart: copy, scale) ----
def copy_into(dst, src):
    dst.r, dst.g, dst.b = src.r, src.g, src.b


def scale_into(obj, s):
    obj.r, obj.g, obj.b = f32(obj.r * s), f32(obj.g * s), f32(obj.b * s)


def neg(s):
    return RGB(-s.r, -s.g, -s.b)


def _sinCosIndexed(s, c, n):                                       # :768-780
    si, ci, sout, cout = 0.0, 1.0, [], []
    for _ in range(n):
        sout.append(si)
        cout.append(ci)
        oldsi = si
        si = si * c + ci * s
        ci = ci * c - oldsi * s
    return sout, cout


def toZYZ(m):                                                      # :782-794 (m: sixteen f32, row major)
    sy = math.sqrt(m[9] * m[9] + m[8] * m[8])
    if sy > 16 * FLT_EPSILON:
        return -math.atan2(m[9], m[8]), -math.atan2(sy, m[10]), -math.atan2(m[6], -m[2])     # alpha, beta, gamma
    return -math.atan2(-m[4], m[5]), -math.atan2(sy, m[10]), 0.0


def RotateZ(c_in, c_out, alpha, lmax):                             # :244-271
    assert c_in is not c_out
    copy_into(c_out[0], c_in[0])
    if lmax == 0:
        return
    st, ct = _sinCosIndexed(math.sin(alpha), math.cos(alpha), lmax + 1)
    for l in range(1, lmax + 1):
        for m in range(-l, 0):
            c_out[Index(l, m)] = c_in[Index(l, m)] * ct[-m] + c_in[Index(l, -m)] * -st[-m]
        copy_into(c_out[Index(l, 0)], c_in[Index(l, 0)])
        for m in range(1, l + 1):
            c_out[Index(l, m)] = c_in[Index(l, m)] * ct[m] + c_in[Index(l, -m)] * st[m]


def RotateXPlus(c_in, c_out, lmax):                                # :291-347 (bands 0 .. 4)
    O = lambda l, m: c_in[Index(l, m)]
    rows = [c_in[0]]
    if lmax >= 1:
        rows += [O(1, 0), neg(O(1, -1)), O(1, 1)]
    if lmax >= 2:
        rows += [O(2, 1), neg(O(2, -1)), O(2, 0) * -0.5 + O(2, 2) * -0.8660254037844386, neg(O(2, -2)),
                 O(2, 0) * -0.8660254037844386 + O(2, 2) * 0.5]
    if lmax >= 3:
        rows += [O(3, 0) * -0.7905694150420949 + O(3, 2) * 0.6123724356957945, neg(O(3, -2)),
                 O(3, 0) * -0.6123724356957945 + O(3, 2) * -0.7905694150420949,
                 O(3, -3) * 0.7905694150420949 + O(3, -1) * 0.6123724356957945,
                 O(3, 1) * -0.25 + O(3, 3) * -0.9682458365518543,
                 O(3, -3) * -0.6123724356957945 + O(3, -1) * 0.7905694150420949,
                 O(3, 1) * -0.9682458365518543 + O(3, 3) * 0.25]
    if lmax >= 4:
        rows += [O(4, 1) * -0.9354143466934853 + O(4, 3) * 0.35355339059327373,
                 O(4, -3) * -0.75 + O(4, -1) * 0.6614378277661477,
                 O(4, 1) * -0.35355339059327373 + O(4, 3) * -0.9354143466934853,
                 O(4, -3) * 0.6614378277661477 + O(4, -1) * 0.75,
                 O(4, 0) * 0.375 + O(4, 2) * 0.5590169943749475 + O(4, 4) * 0.739509972887452,
                 O(4, -4) * 0.9354143466934853 + O(4, -2) * 0.35355339059327373,
                 O(4, 0) * 0.5590169943749475 + O(4, 2) * 0.5 + O(4, 4) * -0.6614378277661477,
                 O(4, -4) * -0.35355339059327373 + O(4, -2) * 0.9354143466934853,
                 O(4, 0) * 0.739509972887452 + O(4, 2) * -0.6614378277661477 + O(4, 4) * 0.125]
    assert lmax <= 4 and len(rows) == Terms(lmax)
    # (the Dart statements run one after the other, each reading c_in only: building the rows first and binding them after is the same)
    for oi, row in enumerate(rows):
        c_out[oi] = row


def RotateXMinus(c_in, c_out, lmax):                               # :273-289
    RotateXPlus(c_in, c_out, lmax)
    for l in range(1, lmax + 1):
        s = -1.0 if (l & 1) != 0 else 1.0
        scale_into(c_out[Index(l, 0)], s)
        for m in range(1, l + 1):
            s = -s
            scale_into(c_out[Index(l, m)], s)
            scale_into(c_out[Index(l, -m)], -s)


def Rotate(c_in, c_out, m, lmax, fresh=False, angles=None):        # :228-242
    """fresh=True hands every step private copies of its input (what a reader expects of the code); the reference shares objects."""
    alpha, beta, gamma = toZYZ(m) if angles is None else angles
    work = [RGB(0.0) for _ in range(Terms(lmax))]                   # Spectrum.AllocateList
    cp = (lambda lst: [RGB(*x.tuple()) for x in lst]) if fresh else (lambda lst: lst)
    RotateZ(c_in, c_out, gamma, lmax)
    RotateXPlus(cp(c_out), work, lmax)
    RotateZ(cp(work), c_out, beta, lmax)
    RotateXMinus(cp(c_out), work, lmax)
    RotateZ(cp(work), c_out, alpha, lmax)


def MatrixVectorMultiply(M, v, lmax):                              # :674-683
    terms = Terms(lmax)
    vout = []
    for i in range(terms):
        acc = RGB(0.0)
        for j in range(terms):
            acc = acc + v[j] * M[terms * i + j]
        vout.append(acc)
    return vout


# ---- the BSDF of ComputeBSDFMatrix ----
class FresnelDielectric(dr.FresnelDielectric):
    pass


def microfacet_f(R, exponent, wo, wi, pow_fn=math.pow):            # microfacet.dart:27-56, blinn.dart:30-33
    cosThetaO, cosThetaI = abs(wo.z), abs(wi.z)
    if cosThetaI == 0.0 or cosThetaO == 0.0:
        return RGB(0.0)
    wh = wi + wo
    if wh.x == 0.0 and wh.y == 0.0 and wh.z == 0.0:
        return RGB(0.0)
    wh = dr.Normalize(wh)
    cosThetaH = dr.Dot(wi, wh)
    F = FresnelDielectric(1.5, 1.0).evaluate(cosThetaH)
    d = (exponent + 2.0) * INV_TWOPI * pow_fn(abs(wh.z), exponent)
    NdotWh, WOdotWh = abs(wh.z), dr.AbsDot(wo, wh)
    g = min(1.0, min((2.0 * NdotWh * cosThetaO / WOdotWh), (2.0 * NdotWh * cosThetaI / WOdotWh)))
    return R * (d * g) * F / (4.0 * cosThetaI * cosThetaO)


def bsdf_f(Kd, Ks, exponent, wo, wi, pow_fn=math.pow):             # bsdf.dart:187-211 on the identity frame, ng = (0, 0, 1)
    ng = Vec(0.0, 0.0, 1.0)
    f = RGB(0.0)
    if dr.Dot(wi, ng) * dr.Dot(wo, ng) > 0:                        # both lobes are BSDF_REFLECTION; else only BTDFs match, and there are none
        f = f + Kd * dr.INV_PI                                     # Lambertian.f
        f = f + microfacet_f(Ks, exponent, wo, wi, pow_fn)
    return f


def ComputeBSDFMatrix(Kd, Ks, roughness, scramble, nSamples, lmax, pow_fn=math.pow):   # :609-672 (the scramble: the two randomUint() it draws)
    terms = Terms(lmax)
    Kd, Ks = RGB(*Kd), RGB(*Ks)
    exponent = 1.0 / roughness
    if exponent > 10000.0 or exponent != exponent:                 # blinn.dart:24-28
        exponent = 10000.0
    w = []
    for i in range(nSamples):
        u = Sample02(i, scramble)
        w.append(UniformSampleSphere(u[0], u[1]))
    Ylm = EvaluateMany([[v.x, v.y, v.z] for v in w], lmax, F32)    # the Float32List, [nSamples, terms] as f64 values
    pdf = (1.0 / (4.0 * math.pi)) * (1.0 / (4.0 * math.pi))
    pdf_nSamples = pdf * nSamples * nSamples
    B = np.zeros((terms, terms, 3), F32)
    for osamp in range(nSamples):
        wo = w[osamp]
        for isamp in range(nSamples):
            wi = w[isamp]
            f = bsdf_f(Kd, Ks, exponent, wo, wi, pow_fn)
            if not f.isBlack():
                f = f * (abs(wi.z) / pdf_nSamples)
                k = np.outer(Ylm[osamp], Ylm[isamp])               # [i][j] = Ylm[isamp][j] * Ylm[osamp][i] (a commutative f64 product)
                fv = np.array(f.tuple(), F64)
                B = B + (fv[None, None, :] * k[:, :, None]).astype(F32)   # B.add(f * (..)): f32 product, f32 sum
    return B


# ---- Li ----
def ComputeTransferMatrix(p, rayEpsilon, scene, rng, nSamples, lmax):   # :580-607 (grey: one f32 per element)
    terms = Terms(lmax)
    T = np.zeros((terms, terms), F32)
    scramble = [rng.randomUint(), rng.randomUint()]
    pdf = 1.0 / (4.0 * math.pi)
    for i in range(nSamples):
        u = Sample02(i, scramble)
        w = UniformSampleSphere(u[0], u[1])
        if not scene.bvh.intersectP(dr.Ray(p, w, rayEpsilon)):
            Ylm = np.array(Evaluate(w, lmax), F64)
            T = T + (np.outer(Ylm, Ylm) / (pdf * nSamples)).astype(F32)
    return T


def shading_frame(isect):
    """bsdf = isect.getBSDF(ray): only its frame and point are read (no material function), so every material serves."""
    shape = isect.prim.shape
    dgs = shape.getShadingGeometry(isect.dg) if hasattr(shape, "getShadingGeometry") else isect.dg
    return dr.BSDF(dgs, isect.dg.nn, ("matte", (0.0, 0.0, 0.0)))


class GlossyPRTIntegrator:
    def __init__(self, lm=4, ns=4096):
        self.lmax, self.nSamples = lm, dr.RoundUpPow2(ns)
        self.c_in, self.B = None, None                             # c_in: [RGB]; B: [terms, terms, 3] f32
        self.angles_of = None                                      # optional: m16 -> (alpha, beta, gamma) from another libm

    def Li(self, scene, ray, isect, rng):                          # :56-116
        lmax, terms = self.lmax, Terms(self.lmax)
        wo = -ray.d
        L = RGB(0.0) + dr.isect_Le(isect, wo)
        bsdf = shading_frame(isect)
        T = ComputeTransferMatrix(bsdf.p, isect.rayEpsilon, scene, rng, self.nSamples, lmax)
        Tl = [RGB(float(T[i, j])) for i in range(terms) for j in range(terms)]
        c_t = MatrixVectorMultiply(Tl, self.c_in, lmax)
        r1, r2, nl = bsdf.localToWorld(Vec(1.0, 0.0, 0.0)), bsdf.localToWorld(Vec(0.0, 1.0, 0.0)), bsdf.localToWorld(Vec(0.0, 0.0, 1.0))
        rot = dr.mat_values(r1.x, r2.x, nl.x, 0.0, r1.y, r2.y, nl.y, 0.0, r1.z, r2.z, nl.z, 0.0, 0.0, 0.0, 0.0, 1.0)
        c_l = [RGB(0.0) for _ in range(terms)]
        Rotate(c_t, c_l, rot, lmax, angles=None if self.angles_of is None else self.angles_of(rot))
        Bl = [RGB(*(float(x) for x in self.B[i, j])) for i in range(terms) for j in range(terms)]
        c_o = MatrixVectorMultiply(Bl, c_l, lmax)
        Ylm = Evaluate(bsdf.worldToLocal(wo), lmax, F32)
        Li = RGB(0.0)
        for i in range(terms):
            Li = Li + c_o[i] * Ylm[i]
        return L + Li.clamp()
