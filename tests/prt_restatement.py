"""DiffusePRTIntegrator (surface_integrators/diffuse_prt_integrator.dart) and what it uses of core/spherical_harmonics.dart, light.dart:98-131,
point_light.dart:75-97 and infinite_area_light.dart:207-281, restated in plain Python / numpy from the Dart text -- the test side's own reading of
the reference, on top of tests/golden/dart_restatement.py (lights, BSDF, Spectrum, RNG), tests/whitted_restatement.py (the delta lights) and the
keyed streams of tests/random_restatement.py.  Cited by file.dart:line.

Arithmetic: every operator rounds where the reference's stores round (Spectrum and Vector: f32; a Float32List handed to Evaluate: every store of the
recurrences), and every serial sum runs in the reference's order.  The cube and lat-long projections are vectorised over directions: the
elementwise numpy operators used are IEEE-exact (+ - * / sqrt), the transcendental functions go through Python's math (the C library), and the
serial f32 sums are np.add.accumulate over float32, which adds one element after the other."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import dart_restatement as dr  # noqa: E402
from dart_restatement import INFINITY, INV_PI, RGB, AbsDot, Dot, Normalize, Ray, RoundUpPow2, UniformSampleSphere, Vec, f32  # noqa: E402,F401
import random_restatement as rr  # noqa: E402
import whitted_restatement as wr  # noqa: E402
import feature_restatement as fe  # noqa: E402  (Triangle.getShadingGeometry for meshes with N / S)
from ao_restatement import FaceForward, RendererLi, Sample02, keyed_rng, render, sample_Li  # noqa: E402,F401

INV_FOURPI = 0.07957747154594766788                                # common.dart:25
F32, F64 = np.float32, np.float64


def Terms(lmax):                                                   # spherical_harmonics.dart:27
    return (lmax + 1) * (lmax + 1)


def Index(l, m):                                                   # :29-30
    return l * l + l + m


def _divfact(a, b):                                                # :738-749
    if b == 0:
        return 1.0
    fa, fb = float(a), abs(float(b))
    v, x = 1.0, fa - fb + 1.0
    while x <= fa + fb:
        v *= x
        x += 1.0
    return 1.0 / v


def _K(l, m):                                                      # :734-736
    return math.sqrt((2.0 * l + 1.0) * INV_FOURPI * _divfact(l, m))


def _store(dtype):
    """A store into the list Evaluate is given: a List<double> keeps the f64, a Float32List rounds it; reads widen again."""
    return (lambda v: v) if dtype is F64 else (lambda v: np.asarray(v, F64).astype(F32).astype(F64))


def _legendrep(x, lmax, out, st):                                  # :685-732 (x: [n] f64; out: [terms][n])
    out[Index(0, 0)] = st(np.ones_like(x))
    out[Index(1, 0)] = st(x)
    for l in range(2, lmax + 1):
        out[Index(l, 0)] = st(((2.0 * l - 1.0) * x * out[Index(l - 1, 0)] - (l - 1) * out[Index(l - 2, 0)]) / l)
    neg, dfact = -1.0, 1.0
    xroot = np.sqrt(np.maximum(0.0, 1.0 - x * x))
    xpow = xroot
    for l in range(1, lmax + 1):
        out[Index(l, l)] = st(neg * dfact * xpow)
        neg *= -1.0
        dfact *= 2 * l + 1
        xpow = xpow * xroot
    for l in range(2, lmax + 1):
        out[Index(l, l - 1)] = st(x * (2.0 * l - 1.0) * out[Index(l - 1, l - 1)])
    for l in range(3, lmax + 1):
        for m in range(1, l - 1):
            out[Index(l, m)] = st(((2.0 * (l - 1.0) + 1.0) * x * out[Index(l - 1, m)] - (l - 1.0 + m) * out[Index(l - 2, m)]) / (l - m))


def _sinCosIndexed(s, c, n):                                       # :768-780
    si, ci = np.zeros_like(s), np.ones_like(s)
    sout, cout = [], []
    for _ in range(n):
        sout.append(si)
        cout.append(ci)
        oldsi = si
        si = si * c + ci * s
        ci = ci * c - oldsi * s
    return sout, cout


def EvaluateMany(w, lmax, dtype=F64):
    """SphericalHarmonics.Evaluate (:32-86) of the directions w [n, 3] (f64 values of the Vectors' f32 components) -> [n, Terms] f64 values of a
    list of `dtype` elements."""
    w = np.asarray(w, F64).reshape(-1, 3)
    st = _store(dtype)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    out = [None] * Terms(lmax)
    _legendrep(z, lmax, out, st)
    Klm = {(l, m): _K(l, m) for l in range(lmax + 1) for m in range(-l, l + 1)}
    xyLen = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    zero = xyLen == 0.0
    safe = np.where(zero, 1.0, xyLen)
    sins, coss = _sinCosIndexed(y / safe, x / safe, lmax + 1)
    sins = [np.where(zero, 0.0, s) for s in sins]
    coss = [np.where(zero, 1.0, c) for c in coss]
    sqrt2 = math.sqrt(2.0)
    for l in range(lmax + 1):
        for m in range(-l, 0):
            out[Index(l, m)] = st(sqrt2 * Klm[(l, m)] * out[Index(l, -m)] * sins[-m])
        out[Index(l, 0)] = st(out[Index(l, 0)] * Klm[(l, 0)])
        for m in range(1, l + 1):
            out[Index(l, m)] = st(out[Index(l, m)] * (sqrt2 * Klm[(l, m)] * coss[m]))
    return np.stack(out, axis=1)


def Evaluate(w, lmax, dtype=F64):
    return [float(v) for v in EvaluateMany([[w.x, w.y, w.z]], lmax, dtype)[0]]


def ReduceRinging(c, lmax, lam=0.005):                             # :219-226; Spectrum.scale (spectrum.dart:227-231): c[i] *= v
    for l in range(lmax + 1):
        scale = 1.0 / (1.0 + lam * l * l * (l + 1) * (l + 1))
        for m in range(-l, l + 1):
            c[Index(l, m)] = c[Index(l, m)] * scale


# ---- f32 Spectrum arithmetic over arrays: [n, 3] float32; every operator one store ----
def _mulS(a, s):
    return (a.astype(F64) * np.asarray(s, F64).reshape(-1, 1)).astype(F32)


def _serial_sum(contrib):
    """coeffs += contrib[i] for i in order, from Spectrum(0): contrib [n, 3] f32 -> RGB."""
    acc = np.add.accumulate(np.concatenate([np.zeros((1, 3), F32), contrib]), axis=0, dtype=F32)[-1]
    return RGB(float(acc[0]), float(acc[1]), float(acc[2]))


def _env_Le_many(light, w):
    """InfiniteAreaLight.Le (infinite_area_light.dart:84-90) of the directions w [n, 3] (f32 Vector components as f64) -> [n, 3] f32:
    _radiance(s, t) = lookup(s, t, 0) * L, lookup = triangle(0, s, t) (mipmap.dart:209-224, 342-355)."""
    m = light.worldToLight
    v32 = lambda a: a.astype(F32).astype(F64)
    wx, wy, wz = (v32(m[4 * r] * w[:, 0] + m[4 * r + 1] * w[:, 1] + m[4 * r + 2] * w[:, 2]) for r in range(3))   # transformVector: f32 stores
    ln = np.sqrt(wx * wx + wy * wy + wz * wz)
    hx, hy, hz = v32(wx / ln), v32(wy / ln), v32(wz / ln)                                                       # Normalize: v / length
    phi = np.array([math.atan2(a, b) for a, b in zip(hy, hx)])
    phi = np.where(phi < 0.0, phi + 2.0 * math.pi, phi)                                                         # SphericalPhi
    theta = np.array([math.acos(min(max(a, -1.0), 1.0)) for a in hz])                                           # SphericalTheta
    s, t = phi * dr.INV_TWOPI, theta * INV_PI
    mp = light.radianceMap
    W, H, lvl = mp.pyramid[0]
    tex = np.array([c.tuple() for c in lvl], F32).reshape(H, W, 3)
    s, t = s * W - 0.5, t * H - 0.5
    s0, t0 = np.floor(s), np.floor(t)
    ds, dt = s - s0, t - t0
    s0, t0 = s0.astype(np.int64), t0.astype(np.int64)
    tx = lambda a, b: tex[b % H, a % W]
    acc = _mulS(tx(s0, t0), (1.0 - ds) * (1.0 - dt))
    acc = acc + _mulS(tx(s0, t0 + 1), (1.0 - ds) * dt)
    acc = acc + _mulS(tx(s0 + 1, t0), ds * (1.0 - dt))
    acc = acc + _mulS(tx(s0 + 1, t0 + 1), ds * dt)
    return acc * np.array(light.L.tuple(), F32)


# ---- shProject, per light kind ----
def shProject_point(light, p, lmax):                               # point_light.dart:75-97 (computeLightVisibility false)
    wi = Normalize(light.lightPos - p)
    Ylm = Evaluate(wi, lmax)
    Li = light.intensity / (light.lightPos - p).lengthSquared()
    return [Li * Ylm[i] for i in range(Terms(lmax))]


def shProject_mc(light, p, pEpsilon, lmax, rng, nSamples):          # light.dart:98-131
    coeffs = [RGB(0.0) for _ in range(Terms(lmax))]
    ns = RoundUpPow2(nSamples)
    scramble1D = rng.randomUint()
    scramble2D = [rng.randomUint(), rng.randomUint()]
    for i in range(ns):
        u = Sample02(i, scramble2D)
        Li, wi, pdf, _ = light.sampleLAtPoint(p, pEpsilon, (u[0], u[1]), dr.VanDerCorput(i, scramble1D))
        if not Li.isBlack() and pdf > 0.0:
            Ylm = Evaluate(wi, lmax, F32)                          # a Float32List
            for j in range(Terms(lmax)):
                coeffs[j] = coeffs[j] + Li * Ylm[j] / (pdf * ns)
    return coeffs


def shProject_infinite(light, p, lmax):                            # infinite_area_light.dart:207-281 (computeLightVis false)
    terms = Terms(lmax)
    mp = light.radianceMap
    ntheta, nphi = mp.height, mp.width
    if min(ntheta, nphi) > 50:                                     # the lat-long representation
        sintheta = [f32(math.sin((t + 0.5) / ntheta * math.pi)) for t in range(ntheta)]
        costheta = [f32(math.cos((t + 0.5) / ntheta * math.pi)) for t in range(ntheta)]
        sinphi = [f32(math.sin((ph + 0.5) / nphi * 2.0 * math.pi)) for ph in range(nphi)]
        cosphi = [f32(math.cos((ph + 0.5) / nphi * 2.0 * math.pi)) for ph in range(nphi)]
        theta_phi_pi = (math.pi / ntheta) * ((2.0 * math.pi) / nphi)
        T, P = np.meshgrid(np.arange(ntheta), np.arange(nphi), indexing="ij")   # theta outer, phi inner
        T, P = T.reshape(-1), P.reshape(-1)
        st_, ct_, sp_, cp_ = np.array(sintheta)[T], np.array(costheta)[T], np.array(sinphi)[P], np.array(cosphi)[P]
        v32 = lambda a: a.astype(F32).astype(F64)
        w = np.stack([v32(st_ * cp_), v32(st_ * sp_), v32(ct_)], axis=1)        # new Vector(...)
        m = light.lightToWorld
        w = np.stack([v32(m[4 * r] * w[:, 0] + m[4 * r + 1] * w[:, 1] + m[4 * r + 2] * w[:, 2]) for r in range(3)], axis=1)
        ln = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
        w = v32(w / ln.reshape(-1, 1))
        W, H, lvl = mp.pyramid[0]
        Le = np.array([c.tuple() for c in lvl], F32).reshape(H, W, 3)[T, P]     # radianceMap.texel(0, phi, theta)
        Ylm = EvaluateMany(w, lmax, F32)
        return [_serial_sum(_mulS(Le, Ylm[:, i] * st_ * theta_phi_pi)) for i in range(terms)]
    # ProjectCube at resolution 200 (spherical_harmonics.dart:88-143); func = Le of the direction (the light's time and point are not read)
    res = 200
    U, V = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    U, V = U.reshape(-1), V.reshape(-1)
    fu, fv = -1.0 + 2.0 * (U + 0.5) / res, -1.0 + 2.0 * (V + 0.5) / res
    one = np.ones_like(fu)
    faces = [(fu, fv, one), (fu, fv, -one), (fu, one, fv), (fu, -one, fv), (one, fu, fv), (-one, fu, fv)]
    v32 = lambda a: a.astype(F32).astype(F64)
    w0 = [v32(a) for a in faces[0]]
    dot0 = w0[0] * w0[0] + w0[1] * w0[1] + w0[2] * w0[2]
    dA = np.array([1.0 / math.pow(d, 3.0 / 2.0) for d in dot0])    # computed at the +z face, reused by the other five
    k4 = 4.0 / (res * res)
    per_face = []
    for fi, face in enumerate(faces):
        w = np.stack([v32(a) for a in face], axis=1)
        ln = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
        Ylm = EvaluateMany(v32(w / ln.reshape(-1, 1)), lmax)
        f = _env_Le_many(light, w)
        per_face.append((f, Ylm))
    out = []
    for k in range(terms):
        contrib = np.zeros((res * res, 6, 3), F32)
        for fi, (f, Ylm) in enumerate(per_face):
            if fi == 0:
                contrib[:, fi] = _mulS(_mulS(_mulS(f, dA), Ylm[:, k]), k4)      # f * dA * Ylm[k] * (4 / res^2)
            else:
                contrib[:, fi] = _mulS(_mulS(_mulS(f, Ylm[:, k]), dA), k4)      # f * Ylm[k] * dA * (4 / res^2)
        out.append(_serial_sum(contrib.reshape(-1, 3)))
    return out


def shProject(light, p, pEpsilon, lmax, rng):
    if isinstance(light, wr.SpotLight) or isinstance(light, DistantLight):
        return shProject_mc(light, p, pEpsilon, lmax, rng, 1)
    if isinstance(light, wr.PointLight):
        return shProject_point(light, p, lmax)
    if isinstance(light, dr.InfiniteAreaLight):
        return shProject_infinite(light, p, lmax)
    return shProject_mc(light, p, pEpsilon, lmax, rng, light.nSamples)


class DistantLight:                                                # distant_light.dart:37-61
    def __init__(self, lightDir, L):
        self.lightDir, self.L = Vec(*lightDir), RGB(*L)

    def Le(self, ray):
        return RGB(0.0)

    def sampleLAtPoint(self, p, pEpsilon, uPos, uComponent):
        return self.L, self.lightDir, 1.0, Ray(p, self.lightDir, pEpsilon, INFINITY)


def ProjectIncidentDirectRadiance(p, pEpsilon, lights, lmax, rng):  # spherical_harmonics.dart:145-170
    c_d = [RGB(0.0) for _ in range(Terms(lmax))]
    for light in lights:
        c = shProject(light, p, pEpsilon, lmax, rng)
        for j in range(Terms(lmax)):
            c_d[j] = c_d[j] + c[j]
    ReduceRinging(c_d, lmax)
    return c_d


def world_centre(scene):
    """Point p = bbox.pMin * 0.5 + bbox.pMax * 0.5 of scene.worldBound, the aggregate's (diffuse_prt_integrator.dart:34-35)."""
    bmin, bmax = scene.bvh.nodes[0][0], scene.bvh.nodes[0][1]
    return Vec(*bmin) * 0.5 + Vec(*bmax) * 0.5


def ComputeDiffuseTransfer(p, n, rayEpsilon, scene, rng, nSamples, lmax):   # spherical_harmonics.dart:557-578
    terms = Terms(lmax)
    c = [RGB(0.0) for _ in range(terms)]
    scramble = [rng.randomUint(), rng.randomUint()]
    pdf = 1.0 / (4.0 * math.pi)                                    # UniformSpherePdf
    for i in range(nSamples):
        u = Sample02(i, scramble)
        w = UniformSampleSphere(u[0], u[1])
        if Dot(w, n) > 0.0 and not scene.bvh.intersectP(Ray(p, w, rayEpsilon)):
            Ylm = Evaluate(w, lmax)
            for j in range(terms):
                c[j] = c[j] + RGB(Ylm[j] * AbsDot(w, n)) / (pdf * nSamples)
    return c


def with_shading_geometry(scene, acc):
    """The golden restatement's triangles carry no per-vertex data.  Those of `scene` (built from the aggregate `acc`, primitives in its order)
    whose mesh has N or S become feature_restatement's Triangle, which restates Triangle.getShadingGeometry (triangle.dart:271-364)."""
    pt = lambda a, i: Vec(float(a[i][0]), float(a[i][1]), float(a[i][2]))
    xf = [(a.reshape(-1), b.reshape(-1)) for a, b in acc.mesh_xforms]
    for i, prim in enumerate(scene.bvh.prims):
        f = int(acc.tri_shading[i]) if acc.tri_shading is not None else 0
        if not (f & 3) or not isinstance(prim.shape, dr.Triangle):
            continue
        a, b, c = (int(v) for v in acc.tri_idx[i])
        o2w, w2o = ([float(v) for v in m] for m in xf[int(acc.tri_xform[i])])
        t = prim.shape
        prim.shape = fe.Triangle(t.p1, t.p2, t.p3, t.reverse, uvs=[(float(acc.vert_uvs[k][0]), float(acc.vert_uvs[k][1])) for k in (a, b, c)] if f & 4 else None,
                                 n=[pt(acc.vert_normals, k) for k in (a, b, c)] if f & 1 else None,
                                 s=[pt(acc.vert_tangents, k) for k in (a, b, c)] if f & 2 else None, o2w=o2w, w2o=w2o)
    return scene


def getBSDF(isect):
    """Intersection.getBSDF -> GeometricPrimitive.getBSDF (geometric_primitive.dart:63-68): dgs = shape.getShadingGeometry(dg), then the material's
    BSDF(dgs, dgGeom.nn).  A shape without per-vertex data returns a copy of dg (triangle.dart:273-276)."""
    shape = isect.prim.shape
    dgs = shape.getShadingGeometry(isect.dg) if hasattr(shape, "getShadingGeometry") else isect.dg
    return dr.BSDF(dgs, isect.dg.nn, isect.prim.material)


def rho2(bsdf, wo, rng):
    """bsdf.rho2(wo, rng, BSDF_ALL_REFLECTION) (bsdf.dart:232-247) for a BSDF of Lambertian lobes: Lambertian.rho is R (lambertian.dart:39-41); the
    72 draws of StratifiedSample2D feed nothing and nothing draws after them."""
    ret = RGB(0.0)
    for bxdf in bsdf.bxdfs:
        assert isinstance(bxdf, dr.Lambertian)
        ret = ret + bxdf.R
    return ret


class DiffusePRTIntegrator:
    def __init__(self, lm=4, ns=4096):                             # :24-31, defaults of Create :83-87
        self.lmax, self.nSamples = lm, RoundUpPow2(ns)
        self.c_in = [RGB(0.0) for _ in range(Terms(lm))]

    def preprocess(self, scene, lights=None):                      # :33-40
        self.c_in = ProjectIncidentDirectRadiance(world_centre(scene), 0.0, scene.lights if lights is None else lights, self.lmax, dr.RNG())
        return self

    def Li(self, scene, ray, isect, rng):                          # :45-81
        wo = -ray.d
        L = RGB(0.0) + dr.isect_Le(isect, wo)
        bsdf = getBSDF(isect)
        p, n = bsdf.p, bsdf.nn
        c_transfer = ComputeDiffuseTransfer(p, FaceForward(n, wo), isect.rayEpsilon, scene, rng, self.nSamples, self.lmax)
        Kd = rho2(bsdf, wo, rng) * INV_PI
        Lo = RGB(0.0)
        for i in range(Terms(self.lmax)):
            Lo = Lo + self.c_in[i] * c_transfer[i]
        return L + Kd * Lo.clamp()
