"""CreateProbesRenderer (renderers/create_probes_renderer.dart) and UseProbesIntegrator (surface_integrators/use_probes_integrator.dart) restated in
plain Python from the Dart text, on top of tests/prt_restatement.py (spherical harmonics, shProject's arithmetic, getBSDF / getShadingGeometry) and
tests/golden/dart_restatement.py (intersection, lights, RNG).  Cited by file.dart:line.  Every Spectrum, Point and Vector store rounds to f32 (the RGB
and Vec classes do), every serial sum runs in the reference's order.  The known answers at the end are hand-checked and need no device."""
import math

import numpy as np

import prt_restatement as prt
from prt_restatement import F32, INV_PI, RGB, Dot, Evaluate, FaceForward, Index, Ray, ReduceRinging, RoundUpPow2, Sample02, Terms, UniformSampleSphere, Vec, dr, f32, wr  # noqa: F401

INFINITY = float("inf")


def Lerp(t, v1, v2):                                               # common.dart:80-81
    return v1 * (1.0 - t) + v2 * t


def RadicalInverse(n, base):                                       # montecarlo.dart:327-339
    val, invBase = 0.0, 1.0 / base
    invBi = invBase
    while n > 0:
        d_i = n % base
        val += d_i * invBi
        n = int(n * invBase)
        invBi *= invBase
    return val


# ---- stage 1: the surface points (create_probes_renderer.dart:78-121) ----
def bounding_sphere(scene):                                        # bbox.dart:66-69, 123-127 of scene.worldBound
    bmin, bmax = Vec(*scene.bvh.nodes[0][0]), Vec(*scene.bvh.nodes[0][1])
    c = bmin * 0.5 + bmax * 0.5
    inside = bmin.x <= c.x <= bmax.x and bmin.y <= c.y <= bmax.y and bmin.z <= c.z <= bmax.z
    return c, ((c - bmax).length() if inside else 0.0)


def surface_points(scene, pCamera, npoints=32768, maxDepth=32):
    """-> (points, hits per walk).  The list may overshoot npoints by up to 31: the inner loop does not re-check."""
    c, radius = bounding_sphere(scene)
    o2w = dr.Transform.Translate(c - Vec(0.0, 0.0, 0.0))
    sphere = dr.Sphere(o2w.m, dr.Transform.Inverse(o2w).m, True, radius, -radius, radius, 360.0)
    pts, walks = [pCamera], []
    rng = dr.RNG()
    while len(pts) < npoints:
        pray = pCamera
        u1 = rng.randomFloat()                                     # (Dart evaluates arguments left to right)
        u2 = rng.randomFloat()
        d = UniformSampleSphere(u1, u2)
        rayEpsilon, hits = 0.0, 0
        for _ in range(maxDepth):
            ray = Ray(pray, d, rayEpsilon, INFINITY)
            isect = scene.bvh.intersect(ray)
            if isect is None:
                hit = sphere.intersect(ray)
                if hit is None:
                    break
                ray.maxt, eps, dg = hit                            # geometric_primitive.dart:47-61
            else:
                eps, dg = isect.rayEpsilon, isect.dg
            pts.append(ray.pointAt(ray.maxt))
            hits += 1
            pray, rayEpsilon = dg.p, eps
            nn = FaceForward(dg.nn, -ray.d)
            u1 = rng.randomFloat()
            u2 = rng.randomFloat()
            d = FaceForward(UniformSampleSphere(u1, u2), nn)
        walks.append(hits)
    return pts, walks


# ---- stage 2: candidates and acceptance (:54-69, 254-309) ----
def make_grid(scene, spacing, bounds=None):
    b = [f32(float(v)) for v in bounds] if bounds is not None else list(scene.bvh.nodes[0][0]) + list(scene.bvh.nodes[0][1])
    delta = Vec(b[3], b[4], b[5]) - Vec(b[0], b[1], b[2])
    return [max(1, math.ceil(v / spacing)) for v in (delta.x, delta.y, delta.z)], b


def candidate(nProbes, b, cell, i):
    s = (cell % nProbes[0], (cell // nProbes[0]) % nProbes[1], cell // (nProbes[0] * nProbes[1]))
    lerp = lambda t: Vec(Lerp(t[0], b[0], b[3]), Lerp(t[1], b[1], b[4]), Lerp(t[2], b[2], b[5]))
    box = dr.BBox(lerp([s[k] / nProbes[k] for k in range(3)]), lerp([(s[k] + 1) / nProbes[k] for k in range(3)]))
    d = (RadicalInverse(i + 1, 2), RadicalInverse(i + 1, 3), RadicalInverse(i + 1, 5))
    return Vec(Lerp(d[0], box.mn.x, box.mx.x), Lerp(d[1], box.mn.y, box.mx.y), Lerp(d[2], box.mn.z, box.mx.z))


def visible(scene, p, pts):
    """Some surface point sees p.  lastVisibleOffset (:292-307) only chooses which point the reference tries first."""
    return any(not scene.bvh.intersectP(Ray(s, p - s, 1e-4, 1.0)) for s in pts)


def accept(scene, nProbes, b, cell, pts):
    """-> (accepted candidate indices, at most 32, in order; the verdict of every candidate tried)."""
    found, tried = [], []
    for i in range(256):
        if len(found) == 32:
            break
        ok = visible(scene, candidate(nProbes, b, cell, i), pts)
        tried.append(ok)
        if ok:
            found.append(i)
    return found, tried


# ---- stage 3: ProjectIncidentDirectRadiance with visibility (spherical_harmonics.dart:145-170; light.dart:98-131; point_light.dart:75-97) ----
def shProject_vis(light, p, pEpsilon, lmax, scene, rng):
    terms = Terms(lmax)
    if isinstance(light, wr.PointLight) and not isinstance(light, wr.SpotLight):
        if scene.bvh.intersectP(Ray(p, prt.Normalize(light.lightPos - p), pEpsilon, (light.lightPos - p).length())):
            return [RGB(0.0) for _ in range(terms)]
        return prt.shProject_point(light, p, lmax)
    # every other light, the infinite one included (infinite_area_light.dart:211-215): Light.shProject
    nSamples = 1 if isinstance(light, (wr.SpotLight, prt.DistantLight)) else light.nSamples
    coeffs = [RGB(0.0) for _ in range(terms)]
    ns = RoundUpPow2(nSamples)
    scramble1D = rng.randomUint()
    scramble2D = [rng.randomUint(), rng.randomUint()]
    for i in range(ns):
        u = Sample02(i, scramble2D)
        Li, wi, pdf, shadow = light.sampleLAtPoint(p, pEpsilon, (u[0], u[1]), dr.VanDerCorput(i, scramble1D))
        if not Li.isBlack() and pdf > 0.0 and not scene.bvh.intersectP(shadow):
            Ylm = Evaluate(wi, lmax, F32)
            for j in range(terms):
                coeffs[j] = coeffs[j] + Li * Ylm[j] / (pdf * ns)
    return coeffs


def project_probe(p, scene, lmax, rng):
    c_d = [RGB(0.0) for _ in range(Terms(lmax))]
    for light in scene.lights:
        c = shProject_vis(light, p, 0.0, lmax, scene, rng)
        for j in range(Terms(lmax)):
            c_d[j] = c_d[j] + c[j]
    ReduceRinging(c_d, lmax)
    return c_d


def bake_cell(scene, nProbes, b, cell, pts, lmax):                 # _CreateRadProbeTask.run (:254-348), includeDirect only
    terms = Terms(lmax)
    rng = dr.RNG(cell)
    c_in = [RGB(0.0) for _ in range(terms)]
    found, _ = accept(scene, nProbes, b, cell, pts)
    for i in found:
        c_probe = project_probe(candidate(nProbes, b, cell, i), scene, lmax, rng)
        for j in range(terms):
            c_in[j] = c_in[j] + c_probe[j]
    if found:
        for j in range(terms):
            c_in[j] = c_in[j] / len(found)
    return c_in, found


def bake(scene, pCamera, lmax=4, spacing=1.0, bounds=None, npoints=32768):
    """-> the reference's Float32List (:139-160) as a float32 array."""
    nProbes, b = make_grid(scene, spacing, bounds)
    pts, _ = surface_points(scene, pCamera, npoints)
    out = [float(lmax), 1.0, 0.0] + [float(n) for n in nProbes] + list(b)
    for cell in range(nProbes[0] * nProbes[1] * nProbes[2]):
        for c in bake_cell(scene, nProbes, b, cell, pts, lmax)[0]:
            out.extend(c.tuple())
    return np.array(out + [0.0, 0.0, 0.0], np.float32)


# ---- UseProbesIntegrator (use_probes_integrator.dart) ----
_C_COSTHETA = [0.8862268925, 1.0233267546, 0.4954159260, 0.0000000000, -0.1107783690, 0.0000000000, 0.0499271341, 0.0000000000, -0.0285469331,
               0.0000000000, 0.0185080823, 0.0000000000, -0.0129818395, 0.0000000000, 0.0096125342, 0.0000000000, -0.0074057109, 0.0000000000]


def ConvolveCosTheta(lmax, c_in):                                  # spherical_harmonics.dart:527-544, 797-798
    out = [None] * Terms(lmax)
    for l in range(lmax + 1):
        for m in range(-l, l + 1):
            o = Index(l, m)
            out[o] = c_in[o] * (math.sqrt((4.0 * math.pi) / (2.0 * l + 1.0)) * _C_COSTHETA[l]) if l < 18 else RGB(0.0)
    return out


class UseProbesIntegrator:
    def __init__(self, data):                                      # :24-72
        fp = [float(v) for v in np.asarray(data, np.float32)]
        self.lmax, self.includeDirect, self.includeIndirect = int(fp[0]), int(fp[1]), int(fp[2])
        self.nProbes = [int(fp[3]), int(fp[4]), int(fp[5])]
        self.bmin, self.bmax = Vec(*fp[6:9]), Vec(*fp[9:12])
        n = Terms(self.lmax) * self.nProbes[0] * self.nProbes[1] * self.nProbes[2]
        self.c_in = [RGB(*fp[12 + 3 * i:15 + 3 * i]) for i in range(n)]
        self.clamped = 0                                           # lookups whose x index left the grid (bookkeeping for the tests)

    def c_inXYZ(self, vx, vy, vz):                                 # :164-170
        cl = lambda v, n: min(max(v, 0), n - 1)
        n = self.nProbes
        return Terms(self.lmax) * (cl(vx, n[0]) + cl(vy, n[1]) * n[0] + cl(vz, n[2]) * n[0] * n[1])

    def lookup(self, p):                                           # :111-145
        off = Vec((p.x - self.bmin.x) / (self.bmax.x - self.bmin.x), (p.y - self.bmin.y) / (self.bmax.y - self.bmin.y),
                  (p.z - self.bmin.z) / (self.bmax.z - self.bmin.z))   # bbox.offset (bbox.dart:193-197)
        vox = [(off.x * self.nProbes[0]) - 0.5, (off.y * self.nProbes[1]) - 0.5, (off.z * self.nProbes[2]) - 0.5]
        v = [math.floor(x) for x in vox]
        d = [x - f for x, f in zip(vox, v)]
        if v[0] < 0 or v[0] + 1 >= self.nProbes[0]:
            self.clamped += 1
        b = {(i, j, k): self.c_inXYZ(v[0] + i, v[1] + j, v[2] + k) for i in (0, 1) for j in (0, 1) for k in (0, 1)}
        out = []
        for i in range(Terms(self.lmax)):
            c00 = Lerp(d[0], self.c_in[b[0, 0, 0] + i], self.c_in[b[1, 0, 0] + i])
            c10 = Lerp(d[0], self.c_in[b[0, 1, 0] + i], self.c_in[b[1, 1, 0] + i])
            c01 = Lerp(d[0], self.c_in[b[0, 0, 1] + i], self.c_in[b[1, 0, 1] + i])
            c11 = Lerp(d[0], self.c_in[b[0, 1, 1] + i], self.c_in[b[1, 1, 1] + i])
            out.append(Lerp(d[2], Lerp(d[1], c00, c10), Lerp(d[1], c01, c11)))
        return out

    def Li(self, scene, ray, isect, rng):                          # :90-162
        assert self.includeDirect != 0
        wo = -ray.d
        L = RGB(0.0) + dr.isect_Le(isect, wo)
        bsdf = prt.getBSDF(isect)
        p, n = bsdf.p, bsdf.nn
        c_E = ConvolveCosTheta(self.lmax, self.lookup(p))
        rho = prt.rho2(bsdf, wo, rng)
        Ylm = Evaluate(FaceForward(n, wo), self.lmax, F32)
        E = RGB(0.0)
        for i in range(Terms(self.lmax)):
            E = E + c_E[i] * Ylm[i]
        return L + rho * INV_PI * E.clamp()


# ---- hand-checked known answers ----
def known_answers():
    # RadicalInverse: 1 -> 1/2 (base 2), 2 -> 2/3 (base 3), 6 = 11 in base 5 -> 1/5 + 1/25
    assert RadicalInverse(1, 2) == 0.5 and abs(RadicalInverse(2, 3) - 2.0 / 3.0) < 1e-15 and abs(RadicalInverse(6, 5) - 0.24) < 1e-15
    # ConvolveCosTheta of a constant function f = 1: its only coefficient is c_00 = sqrt(4 pi); the irradiance of a unit sky is pi, so
    # c_E[0] * Y_00 = pi with Y_00 = 1 / sqrt(4 pi): c_E[0] = pi * sqrt(4 pi)
    cE = ConvolveCosTheta(2, [RGB(math.sqrt(4.0 * math.pi))] + [RGB(0.0)] * 8)
    assert abs(cE[0].tuple()[0] - math.pi * math.sqrt(4.0 * math.pi)) < 2e-6 and all(c.isBlack() for c in cE[1:])
    # the trilinear lookup at a cell centre returns that cell's coefficients: a 2 x 1 x 1 grid over [0, 2] x [0, 1] x [0, 1], lmax 1
    data = [1.0, 1.0, 0.0, 2.0, 1.0, 1.0, 0.0, 0.0, 0.0, 2.0, 1.0, 1.0] + [float(i) for i in range(1, 25)] + [0.0] * 3
    g = UseProbesIntegrator(np.array(data, np.float32))
    assert [c.tuple() for c in g.lookup(Vec(0.5, 0.5, 0.5))] == [(1.0, 2.0, 3.0), (4.0, 5.0, 6.0), (7.0, 8.0, 9.0), (10.0, 11.0, 12.0)]
    assert [c.tuple() for c in g.lookup(Vec(1.5, 0.5, 0.5))][0] == (13.0, 14.0, 15.0)
    # halfway between the two centres: the mean; beyond the last centre: the corner clamp holds the last cell's values
    assert g.lookup(Vec(1.0, 0.5, 0.5))[0].tuple() == (7.0, 8.0, 9.0) and g.lookup(Vec(1.9, 0.2, 0.9))[0].tuple() == (13.0, 14.0, 15.0)
    # nProbes = max(1, ceil(delta / spacing))
    class _S:
        pass
    s = _S()
    s.bvh = _S()
    s.bvh.nodes = [((0.0, 0.0, 0.0), (2.5, 1.0, 0.0))]
    assert make_grid(s, 1.0)[0] == [3, 1, 1]
    return True
