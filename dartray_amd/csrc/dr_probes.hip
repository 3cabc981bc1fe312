// dr_probes.hip -- CreateProbesRenderer (renderers/create_probes_renderer.dart) on the device: the bake of shadowed direct light onto a 3-D grid
// of spherical-harmonic probes that UseProbesIntegrator (dr_shade_probes.hip) reads.  DESIGN.md 2.18.  Four stages, each behind an entry point:
//
//   1 dr_probes_surface_points  (:78-121) the random walks from the camera that deposit surface points.  The one RNG(5489) stream is drawn on the
//       host and uploaded; a walk's place in it is known once the earlier walks' hit counts are: a walk of h hits consumes 2 + 2 h values.  Every
//       walk still needed is run at once under the assumption that the walks before it are full (32 hits: true whenever the camera lies inside
//       the bounding sphere); 32 steps of k_walk_rays -> the closest-hit traversal -> k_walk_step; the hit counts are read back, and the walks
//       behind the first short one are run again from their true offsets.
//   2 dr_probes_candidates      (:254-309) per cell 256 candidates b.lerp(RadicalInverse(i + 1, 2 / 3 / 5)); a candidate is accepted iff SOME surface
//       point s has !intersectP(Ray(s, p - s, 1e-4, 1.0)) -- lastVisibleOffset only orders the reference's tries -- so the test is an order-free
//       "any of N" reduction.  The hot path: k_cand_rays writes one any-hit ray per (live candidate, surface point of the round's chunk), the
//       any-hit traversal traces them, k_cand_reduce marks the candidates some ray found free, k_cand_compact drops them from the work list.  The
//       chunks grow 64, 256, 1024, 4096 points: a visible candidate usually leaves in the first round, and only the candidates nothing sees pay
//       for all N points.  Candidates go in groups of 64 per cell; a cell with 32 accepted ones takes no further group (`nFound == 32` breaks).
//   3 projection  ProjectIncidentDirectRadiance(p, 0, time, scene, true, lmax, RNG(cell)) of every accepted candidate: k_probe_contrib is
//       k_prt_contrib (dr_prt_project.hip) for many points, with the infinite light on Light.shProject's Monte-Carlo route and one visibility ray
//       per sample (the point light: its override's one ray); the any-hit traversal; k_probe_sum adds the unoccluded samples' contributions in
//       sample order, then `c_d += c`; k_probe_finish: ReduceRinging per candidate, `c_in += c_probe` in candidate order, `/= nFound`.
//   4 dr_probes_bake  runs 1 to 3 and writes the reference's Float32List.
// dr_scene_set_probes attaches a grid to a scene.  Every traversal is the library's own (launch_intersect), so a ray's answer is the reference's.
#include <string.h>

#include <vector>

#include "dr_host.h"
#include "dr_rng.h"
#include "dr_shade_hit.h"  // hit_rec, hit_dg, ray_epsilon
#include "dr_li_sampling.h"

using namespace dr_host;

namespace dr_host {
int traceGridMax();                   // dr_api.hip
int ensureTraceSpill(DrScene* sc);    // dr_api.hip
}

namespace {

constexpr uint32_t kMaxRays = 1u << 21;  // rays of one traversal launch (DrRay + DrHit: 72 B each)
constexpr int kMaxDepth = 32, kCandidates = 256, kMaxFound = 32;

DR_DEV F3 ldp(const float* p, size_t i) { return F3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
DR_DEV void put_ray(DrRay* r, F3 o, F3 d, double tmin, double tmax) {
  DrRay q;
  q.o[0] = o.x; q.o[1] = o.y; q.o[2] = o.z;
  q.d[0] = d.x; q.d[1] = d.y; q.d[2] = d.z;
  q.tmin = tmin;
  q.tmax = tmax;
  *r = q;
}

// ---- stage 1 ----
struct Walks {
  float* pray;     // [n][3]
  float* dir;      // [n][3]
  double* eps;     // [n]
  int32_t* alive;  // [n]
  int32_t* hits;   // [n]
  float* points;   // [n][32][3]
  const double* u; // the stream
  const unsigned long long* off;  // [n] first value of each walk
};

__global__ void __launch_bounds__(256) k_walk_init(Walks w, uint32_t n, F3 cam) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const F3 d = UniformSampleSphere(w.u[w.off[i]], w.u[w.off[i] + 1]);
  w.pray[3 * i] = cam.x; w.pray[3 * i + 1] = cam.y; w.pray[3 * i + 2] = cam.z;
  w.dir[3 * i] = d.x; w.dir[3 * i + 1] = d.y; w.dir[3 * i + 2] = d.z;
  w.eps[i] = 0.0;
  w.alive[i] = 1;
  w.hits[i] = 0;
}
__global__ void __launch_bounds__(256) k_walk_rays(Walks w, uint32_t n, DrRay* rays) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // (a walk that has ended: a ray of empty extent, which hits nothing)
  put_ray(rays + i, ldp(w.pray, i), ldp(w.dir, i), w.eps[i], w.alive[i] ? DR_INF : -1.0);
}
__global__ void __launch_bounds__(256) k_walk_step(DScene sc, DQuadric sph, Walks w, uint32_t n, int step, const DrHit* hit) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !w.alive[i]) return;
  const F3 o = ldp(w.pray, i), d = ldp(w.dir, i);
  const DrHit h = hit[i];
  double t, eps;
  DGeo dg;
  if (h.prim >= 0) {  // scene.intersect(ray, isect)
    t = h.t;
    const HitRec rec = hit_rec(sc, (uint32_t)h.prim);
    hit_dg(sc, rec, hit_srec(sc, rec), o, d, t, &dg);
    eps = ray_epsilon(rec.isQuad, t);
  } else {            // sphere.intersect(ray, isect): the bounding sphere of scene.worldBound
    F3 phit;
    if (!quadric_hit(sph, o, d, w.eps[i], DR_INF, &t, &phit)) {
      w.alive[i] = 0;  // break
      return;
    }
    quadric_dg(sph, phit, &dg);
    eps = 5.0e-4 * t;
  }
  const F3 pt = vadd(o, vmul(d, t));  // ray.pointAt(ray.maxDistance)
  float* out = w.points + ((size_t)i * kMaxDepth + (size_t)step) * 3;
  out[0] = pt.x; out[1] = pt.y; out[2] = pt.z;
  w.hits[i] = step + 1;
  const F3 nn = vdot(dg.nn, vneg(d)) < 0.0 ? vneg(dg.nn) : dg.nn;  // Normal.FaceForward(hitGeometry.nn, -ray.direction)
  const unsigned long long k = w.off[i] + 2ull + 2ull * (unsigned long long)step;
  F3 nd = UniformSampleSphere(w.u[k], w.u[k + 1]);
  if (vdot(nd, nn) < 0.0) nd = vneg(nd);                           // Vector.FaceForward(dir, hitGeometry.nn)
  w.pray[3 * i] = dg.p.x; w.pray[3 * i + 1] = dg.p.y; w.pray[3 * i + 2] = dg.p.z;
  w.dir[3 * i] = nd.x; w.dir[3 * i + 1] = nd.y; w.dir[3 * i + 2] = nd.z;
  w.eps[i] = eps;
}

// ---- stage 2 ----
// ray (li, j) of a round: from surface point pos + j to candidate live[li]; n points per candidate
__global__ void __launch_bounds__(256) k_cand_rays(const float* pts, uint32_t pos, uint32_t n, const float* cand, const uint32_t* live, uint32_t nlive, DrRay* rays) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nlive * n) return;
  const F3 s = ldp(pts, pos + idx % n), p = ldp(cand, live[idx / n]);
  put_ray(rays + idx, s, vsub(p, s), 1.0e-4, 1.0);  // Ray(surfacePoints[j], p - surfacePoints[j], 1e-4, 1.0, time)
}
__global__ void __launch_bounds__(256) k_cand_reduce(const DrHit* hit, uint32_t n, const uint32_t* live, uint32_t nlive, uint32_t* visible) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nlive * n) return;
  if (hit[idx].prim < 0) visible[live[idx / n]] = 1u;  // !scene.intersectP: some point sees the candidate (every writer stores the same 1)
}
__global__ void __launch_bounds__(256) k_cand_compact(const uint32_t* live, uint32_t nlive, const uint32_t* visible, uint32_t* out, uint32_t* nout) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nlive) return;
  const uint32_t c = live[i];
  if (!visible[c]) out[atomicAdd(nout, 1u)] = c;  // (the list's order carries no meaning: acceptance is per candidate)
}

// ---- stage 3 ----
enum { PROBE_POINT = 0, PROBE_MC = 1 };
struct ProbeProj {
  int32_t mode, light, lmax, ns;
  int32_t mc, nmc;      // this light's place among the scene's non-point lights, and their number: scr[probe][nmc][3]
  const uint32_t* scr;
  const float* pts;     // the accepted candidates, [nprobes][3]
  const double* K;
};

// one lane per (probe, sample) of a slice: the sample's contribution to every (term, channel) as if it were unoccluded, and its visibility ray
__global__ void __launch_bounds__(128) k_probe_contrib(DScene sc, ProbeProj a, uint32_t first, uint32_t count, float* contrib, DrRay* rays) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= count * (uint32_t)a.ns) return;
  const uint32_t probe = first + tid / (uint32_t)a.ns, i = tid % (uint32_t)a.ns;
  const int terms = sh_terms(a.lmax);
  float* out = contrib + (size_t)tid * (size_t)(3 * terms);
  const F3 p = ldp(a.pts, probe);
  const DLight light = sc.lights[a.light];
  auto put = [&](int j, C3 v) {
    out[3 * j] = v.r;
    out[3 * j + 1] = v.g;
    out[3 * j + 2] = v.b;
  };
  F3 shd = F3{0.f, 0.f, 1.f};
  double shTmax = -1.0;  // (a skipped sample: a ray of empty extent, and a contribution of +0)
  if (a.mode == PROBE_POINT) {  // point_light.dart:75-97 with computeLightVisibility
    const F3 lp = F3{light.pos[0], light.pos[1], light.pos[2]};
    const F3 seg = vsub(lp, p);
    const F3 wi = vnormalize(seg);
    double Ylm[DR_SH_MAX_TERMS];
    sh_evaluate((double)wi.x, (double)wi.y, (double)wi.z, a.lmax, a.K, Ylm);
    const C3 Li = cdivD(C3{light.L[0], light.L[1], light.L[2]}, vlen2(seg));
    for (int j = 0; j < terms; ++j) put(j, cmulD(Li, Ylm[j]));
    shd = wi;            // Ray(p, Normalize(lightPos - p), pEpsilon, Distance(lightPos, p))
    shTmax = vlen(seg);
  } else {                      // light.dart:98-131
    const GlobalLights lv = GlobalLights{sc.lights, sc.ltris, sc.lcdf, sc.mats};
    const uint32_t* scr = a.scr + ((size_t)probe * (size_t)a.nmc + (size_t)a.mc) * 3;
    const uint32_t scr2[2] = {scr[1], scr[2]};
    double u[2];
    Sample02(i, scr2, u);
    const double uc = scrambled_radical(i, scr[0], false);  // VanDerCorput(i, scramble1D)
    F3 wi = F3{0, 0, 0};
    double pdf = 0.0, tmax = -1.0;
    C3 Li;
    if (light.kind >= DR_LIGHT_POINT) {  // SpotLight (spot_light.dart:54-85), DistantLight (distant_light.dart:54-61): pdf = 1
      const F3 lp = F3{light.pos[0], light.pos[1], light.pos[2]};
      pdf = 1.0;
      if (light.kind == DR_LIGHT_DISTANT) {
        wi = lp;
        Li = C3{light.L[0], light.L[1], light.L[2]};
        shd = wi;  // VisibilityTester.setRay(p, eps, wi)
        tmax = DR_INF;
      } else {
        const F3 seg = vsub(lp, p);
        wi = vnormalize(seg);
        C3 I = C3{light.L[0], light.L[1], light.L[2]};
        if (light.kind == DR_LIGHT_SPOT) {
          const F3 wl = vnormalize(q_vector(light.w2l, vneg(wi)));
          const double costheta = wl.z;
          double fo;
          if (costheta < light.cosTotalWidth) fo = 0.0;
          else if (costheta > light.cosFalloffStart) fo = 1.0;
          else {
            const double delta = (costheta - light.cosTotalWidth) / (light.cosFalloffStart - light.cosTotalWidth);
            fo = delta * delta * delta * delta;
          }
          I = cmulD(I, fo);
        }
        Li = cdivD(I, vlen2(seg));
        const double dist = vlen(seg);  // VisibilityTester.setSegment(p, eps, lightPos, 0)
        shd = vdiv(seg, dist);
        tmax = dist * (1.0 - 0.0);
      }
    } else if (light.kind == DR_LIGHT_INFINITE) {  // InfiniteAreaLight.sampleLAtPoint (infinite_area_light.dart:92-131); setRay
      Li = env_sample_x<false>(sc.env, u[0], u[1], &wi, &pdf);
      shd = wi;
      tmax = DR_INF;
    } else {  // DiffuseAreaLight.sampleLAtPoint (diffuse_area_light.dart:60-70); setSegment(p, eps, ps, 1e-3)
      F3 ns;
      const F3 ps = shapeset_sample<true>(sc, lv, light, u[0], u[1], uc, &ns, p);
      wi = vnormalize(vsub(ps, p));
      pdf = shapeset_pdf<true>(sc, lv, light, p, wi);
      Li = light_L(light, ns, vneg(wi));
      const F3 seg = vsub(ps, p);
      const double dist = vlen(seg);
      shd = vdiv(seg, dist);
      tmax = dist * (1.0 - 1.0e-3);
    }
    if (!cblack(Li) && pdf > 0.0) {
      float Ylm[DR_SH_MAX_TERMS];
      sh_evaluate((double)wi.x, (double)wi.y, (double)wi.z, a.lmax, a.K, Ylm);
      const double den = pdf * a.ns;
      for (int j = 0; j < terms; ++j) put(j, cdivD(cmulD(Li, (double)Ylm[j]), den));  // Li * Ylm[j] / (pdf * ns)
      shTmax = tmax;
    } else {
      for (int j = 0; j < terms; ++j) put(j, C3{0.f, 0.f, 0.f});
      shd = F3{0.f, 0.f, 1.f};
    }
  }
  put_ray(rays + tid, p, shd, 0.0, shTmax);  // pEpsilon = 0
}
// one lane per (probe of the slice, term * 3 + channel): c = the serial f32 sum of the unoccluded samples' contributions in sample order; c_d += c
__global__ void __launch_bounds__(256) k_probe_sum(const float* contrib, const DrHit* hit, uint32_t first, uint32_t count, int ns, int n3, float* cd) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= count * (uint32_t)n3) return;
  const uint32_t pl = tid / (uint32_t)n3, tc = tid % (uint32_t)n3;
  float acc = 0.f;
  for (int i = 0; i < ns; ++i) {
    const size_t s = (size_t)pl * (size_t)ns + (size_t)i;
    if (hit[s].prim < 0) acc = acc + contrib[s * (size_t)n3 + tc];
  }
  float* dst = cd + (size_t)(first + pl) * (size_t)n3 + tc;
  *dst = *dst + acc;
}
// one lane per (cell, term * 3 + channel): ReduceRinging of every accepted candidate's c_probe, c_in += c_probe in candidate order, c_in /= nFound
__global__ void __launch_bounds__(256) k_probe_finish(const float* cd, const uint32_t* cellFirst, const int32_t* nfound, uint32_t ncells, int lmax, float* out) {
  const int n3 = 3 * sh_terms(lmax);
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= ncells * (uint32_t)n3) return;
  const uint32_t cell = tid / (uint32_t)n3, tc = tid % (uint32_t)n3;
  const int j = (int)tc / 3;
  int l = 0;
  while ((l + 1) * (l + 1) <= j) ++l;
  const double scale = sh_ringing_scale(l, 0.005);
  const int nf = nfound[cell];
  float acc = 0.f;
  for (int k = 0; k < nf; ++k) acc = acc + (float)((double)cd[(size_t)(cellFirst[cell] + (uint32_t)k) * (size_t)n3 + tc] * scale);
  if (nf > 0) acc = (float)((double)acc / (double)nf);
  out[tid] = acc;
}

double radicalInverse(int n, int base) {  // montecarlo.dart:327-339
  double val = 0.0;
  const double invBase = 1.0 / base;
  double invBi = invBase;
  while (n > 0) {
    const int d_i = n % base;
    val += d_i * invBi;
    n = (int)(n * invBase);
    invBi *= invBase;
  }
  return val;
}
float lerpf(double t, float a, float b) { return (float)((double)a * (1.0 - t) + (double)b * t); }  // Lerp (common.dart:80-81) into a Point

struct Grid {
  int n[3];
  float b[6];
  uint32_t cells() const { return (uint32_t)n[0] * (uint32_t)n[1] * (uint32_t)n[2]; }
};
// the bounds (default: scene.worldBound) and nProbes[i] = max(1, ceil(delta[i] / spacing)) (:54-69)
int makeGrid(const DrScene* sc, const float* bounds, double spacing, Grid* g) {
  if (!(spacing > 0.0)) return fail(DR_ERR_INVALID, "create probes: samplespacing must be positive");
  for (int k = 0; k < 6; ++k) g->b[k] = bounds ? bounds[k] : sc->d.rootBox[k];
  uint64_t cells = 1;
  for (int k = 0; k < 3; ++k) {
    const float delta = g->b[3 + k] - g->b[k];  // Vector delta = bbox.pMax - bbox.pMin
    if (!(delta >= 0.f) || delta - delta != 0.f) return fail(DR_ERR_INVALID, "create probes: bounds must be finite with pMin <= pMax");
    const double c = ceil((double)delta / spacing);
    if (c > 4096.0) return fail(DR_ERR_UNSUPPORTED, "create probes: more than 4096 probes along an axis");
    g->n[k] = std::max(1, (int)c);
    cells *= (uint64_t)g->n[k];
  }
  if (cells > (1ull << 20)) return fail(DR_ERR_UNSUPPORTED, "create probes: more than 2^20 cells");
  return DR_OK;
}
// candidate i of cell `cell` (:256-289)
void candidate(const Grid& g, uint32_t cell, int i, float p[3]) {
  const int s[3] = {(int)(cell % (uint32_t)g.n[0]), (int)((cell / (uint32_t)g.n[0]) % (uint32_t)g.n[1]), (int)(cell / ((uint32_t)g.n[0] * (uint32_t)g.n[1]))};
  const int base[3] = {2, 3, 5};
  for (int k = 0; k < 3; ++k) {
    const double t0 = (double)s[k] / (double)g.n[k], t1 = (double)(s[k] + 1) / (double)g.n[k];
    const float a = lerpf(t0, g.b[k], g.b[3 + k]), c = lerpf(t1, g.b[k], g.b[3 + k]);  // BBox(bbox.lerp(t0), bbox.lerp(t1)): min / max per axis
    p[k] = lerpf(radicalInverse(i + 1, base[k]), std::min(a, c), std::max(a, c));
  }
}

struct TraceBufs {
  DevBuf<DrRay> rays;
  DevBuf<DrHit> hits;
  DevBuf<uint32_t> work;
  int grid = 0;
};
int traceInit(DrScene* sc, TraceBufs& T, size_t cap) {
  const int rc = ensureTraceSpill(sc);
  if (rc) return rc;
  HIP_TRY(T.rays.alloc(cap));
  HIP_TRY(T.hits.alloc(cap));
  HIP_TRY(T.work.alloc(8 * DR_WORK_STRIDE));
  T.grid = traceGridMax();
  return DR_OK;
}
int trace(DrScene* sc, TraceBufs& T, size_t n, int anyHit) {
  if (n == 0) return DR_OK;
  HIP_TRY(hipMemsetAsync(T.work.p, 0, 8 * DR_WORK_STRIDE * sizeof(uint32_t), nullptr));
  const int grid = (int)std::min<size_t>((size_t)T.grid, (n + DR_TRACE_BLOCK - 1) / DR_TRACE_BLOCK);
  launch_intersect(sc->d, T.rays.p, (int64_t)n, T.hits.p, anyHit, sc->ws.spill.p, T.work.p, sc->ctr.p, grid, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(sc->ctr.p, 0, sizeof(TraceCounters), nullptr));  // (a render's statistics count its own rays only)
  return DR_OK;
}
dim3 blocks(size_t n, int b) { return dim3((unsigned)((n + (size_t)b - 1) / (size_t)b)); }

// ---- stage 1 on the host side ----
int surfacePoints(DrScene* sc, const float cam[3], int npoints, std::vector<float>& pts) {
  if (npoints < 1 || npoints > (1 << 22)) return fail(DR_ERR_INVALID, "create probes: npoints must be in 1 .. 2^22");
  // the bounding sphere of scene.worldBound (bbox.dart:66-69) as the reference's Sphere(Translate(centre), inverse, true, r, -r, r, 360)
  const float* rb = sc->d.rootBox;
  float c[3];
  bool inside = true;
  for (int k = 0; k < 3; ++k) {
    c[k] = (float)((double)(float)((double)rb[k] * 0.5) + (double)(float)((double)rb[3 + k] * 0.5));
    inside = inside && c[k] >= rb[k] && c[k] <= rb[3 + k];
  }
  // (boundingSphere answers radius 0 for a box that does not hold its own centre -- an empty or non-finite world bound -- and the Sphere's
  // thetaMin / thetaMax become acos(0 / 0): such a scene is refused by name instead)
  const float dx = c[0] - rb[3], dy = c[1] - rb[4], dz = c[2] - rb[5];
  const double radius = inside ? sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz) : 0.0;
  if (!sc->d.ntris || !(radius > 0.0) || radius - radius != 0.0)
    return fail(DR_ERR_INVALID, "create probes: the scene's world bound is empty or not finite (its bounding sphere has no radius)");
  DQuadric sph;
  memset(&sph, 0, sizeof(sph));
  for (int k = 0; k < 3; ++k) {
    sph.o2w[5 * k] = sph.w2o[5 * k] = 1.f;
    sph.o2w[4 * k + 3] = c[k] - 0.f;  // Translate(sceneCenter - Point.ZERO)
    sph.w2o[4 * k + 3] = -sph.o2w[4 * k + 3];
  }
  sph.kind = DR_QUADRIC_SPHERE;
  sph.reverse = 1;
  sph.radius = radius;
  sph.zmin = std::min(std::max(std::min(-radius, radius), -radius), radius);
  sph.zmax = std::min(std::max(std::max(-radius, radius), -radius), radius);
  auto clampd = [](double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); };
  sph.thetaMin = acos(clampd(sph.zmin / radius, -1.0, 1.0));
  sph.thetaMax = acos(clampd(sph.zmax / radius, -1.0, 1.0));
  sph.phiMax = (3.141592653589793 / 180.0) * 360.0;

  pts.assign(cam, cam + 3);  // surfacePoints.add(pCamera)
  DartRandom rng;
  rng.seed(5489);
  std::vector<double> u;
  unsigned long long base = 0;  // the stream position of the next walk
  TraceBufs T;
  DevBuf<float> pray, dir, points;
  DevBuf<double> eps, du;
  DevBuf<int32_t> alive, hits;
  DevBuf<unsigned long long> off;
  std::vector<unsigned long long> offH;
  std::vector<int32_t> hitsH;
  std::vector<float> pointsH;
  int passes = 0;
  while ((int)(pts.size() / 3) < npoints) {
    if (++passes > 4096) return fail(DR_ERR_UNSUPPORTED, "create probes: more than 4096 passes of the surface-point walks (nearly every walk leaves the scene at once)");
    const uint32_t n = (uint32_t)((npoints - (int)(pts.size() / 3) + kMaxDepth - 1) / kMaxDepth);  // walks still needed if every one is full
    const size_t per = 2 + 2 * kMaxDepth;
    while (u.size() < base + (size_t)n * per) u.push_back(rng.randomFloat());
    offH.resize(n);
    for (uint32_t i = 0; i < n; ++i) offH[i] = base + (unsigned long long)i * per;
    int rc = traceInit(sc, T, n);
    if (rc) return rc;
    HIP_TRY(pray.alloc(3 * (size_t)n));
    HIP_TRY(dir.alloc(3 * (size_t)n));
    HIP_TRY(points.alloc(3 * (size_t)n * kMaxDepth));
    HIP_TRY(eps.alloc(n));
    HIP_TRY(alive.alloc(n));
    HIP_TRY(hits.alloc(n));
    HIP_TRY(off.alloc(n));
    HIP_TRY(du.alloc(u.size()));
    HIP_TRY(hipMemcpy(du.p, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(off.p, offH.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice));
    const Walks w = {pray.p, dir.p, eps.p, alive.p, hits.p, points.p, du.p, off.p};
    hipLaunchKernelGGL(k_walk_init, blocks(n, 256), dim3(256), 0, nullptr, w, n, F3{cam[0], cam[1], cam[2]});
    for (int step = 0; step < kMaxDepth; ++step) {
      hipLaunchKernelGGL(k_walk_rays, blocks(n, 256), dim3(256), 0, nullptr, w, n, T.rays.p);
      rc = trace(sc, T, n, 0);
      if (rc) return rc;
      hipLaunchKernelGGL(k_walk_step, blocks(n, 256), dim3(256), 0, nullptr, sc->d, sph, w, n, step, T.hits.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    hitsH.resize(n);
    pointsH.resize(3 * (size_t)n * kMaxDepth);
    HIP_TRY(hipMemcpy(hitsH.data(), hits.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pointsH.data(), points.p, pointsH.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n && (int)(pts.size() / 3) < npoints; ++i) {  // (the outer loop's test, before every walk)
      const float* p = pointsH.data() + 3 * (size_t)i * kMaxDepth;
      pts.insert(pts.end(), p, p + 3 * (size_t)hitsH[i]);
      base = offH[i] + 2ull + 2ull * (unsigned long long)hitsH[i];
      if (hitsH[i] < kMaxDepth) break;  // the walks behind a short one started from the wrong place in the stream: again
    }
  }
  return DR_OK;
}

// ---- stage 2 on the host side: nfound[cells], accepted[cells][32] (-1: none) ----
int acceptCandidates(DrScene* sc, const Grid& g, const std::vector<float>& pts, std::vector<int32_t>& nfound, std::vector<int32_t>& accepted,
                     std::vector<float>& candH) {
  const uint32_t cells = g.cells(), npts = (uint32_t)(pts.size() / 3);
  nfound.assign(cells, 0);
  accepted.assign((size_t)cells * kMaxFound, -1);
  candH.resize((size_t)cells * kCandidates * 3);
  for (uint32_t c = 0; c < cells; ++c)
    for (int i = 0; i < kCandidates; ++i) candidate(g, c, i, candH.data() + ((size_t)c * kCandidates + (size_t)i) * 3);
  DevBuf<float> dPts, dCand;
  DevBuf<uint32_t> liveA, liveB, visible, nlive;
  TraceBufs T;
  int rc = traceInit(sc, T, kMaxRays);
  if (rc) return rc;
  HIP_TRY(dPts.alloc(pts.size()));
  HIP_TRY(dCand.alloc(candH.size()));
  HIP_TRY(hipMemcpy(dPts.p, pts.data(), pts.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dCand.p, candH.data(), candH.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(visible.alloc((size_t)cells * kCandidates));
  HIP_TRY(hipMemset(visible.p, 0, (size_t)cells * kCandidates * sizeof(uint32_t)));
  HIP_TRY(liveA.alloc((size_t)cells * 64));
  HIP_TRY(liveB.alloc((size_t)cells * 64));
  HIP_TRY(nlive.alloc(1));
  std::vector<uint32_t> liveH, visH((size_t)cells * kCandidates);
  for (int group = 0; group < kCandidates / 64; ++group) {
    liveH.clear();
    for (uint32_t c = 0; c < cells; ++c)
      if (nfound[c] < kMaxFound)
        for (int i = 0; i < 64; ++i) liveH.push_back(c * kCandidates + (uint32_t)(group * 64 + i));
    if (liveH.empty()) break;
    uint32_t nl = (uint32_t)liveH.size();
    HIP_TRY(hipMemcpy(liveA.p, liveH.data(), nl * sizeof(uint32_t), hipMemcpyHostToDevice));
    uint32_t *in = liveA.p, *out = liveB.p;
    uint32_t chunk = 64;
    for (uint32_t pos = 0; pos < npts && nl > 0; chunk = std::min(chunk * 4u, 4096u)) {
      const uint32_t n = std::min(chunk, npts - pos);
      const uint32_t perLaunch = std::max(1u, kMaxRays / n);  // candidates of one traversal launch
      for (uint32_t l0 = 0; l0 < nl; l0 += perLaunch) {
        const uint32_t m = std::min(perLaunch, nl - l0);
        const size_t total = (size_t)m * n;
        hipLaunchKernelGGL(k_cand_rays, blocks(total, 256), dim3(256), 0, nullptr, dPts.p, pos, n, dCand.p, in + l0, m, T.rays.p);
        rc = trace(sc, T, total, 1);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cand_reduce, blocks(total, 256), dim3(256), 0, nullptr, T.hits.p, n, in + l0, m, visible.p);
      }
      HIP_TRY(hipMemsetAsync(nlive.p, 0, sizeof(uint32_t), nullptr));
      hipLaunchKernelGGL(k_cand_compact, blocks(nl, 256), dim3(256), 0, nullptr, in, nl, visible.p, out, nlive.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(&nl, nlive.p, sizeof(uint32_t), hipMemcpyDeviceToHost));  // (the round's host wait: the next round's launches are sized by it)
      std::swap(in, out);
      pos += n;
    }
    HIP_TRY(hipMemcpy(visH.data(), visible.p, visH.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < cells; ++c)
      for (int i = group * 64; i < group * 64 + 64 && nfound[c] < kMaxFound; ++i)
        if (visH[(size_t)c * kCandidates + (size_t)i]) accepted[(size_t)c * kMaxFound + (size_t)nfound[c]++] = i;
  }
  return DR_OK;
}

// ---- stage 3 on the host side: coefficients out[cells][Terms][3] ----
int projectProbes(DrScene* sc, const Grid& g, int lmax, const std::vector<int32_t>& nfound, const std::vector<int32_t>& accepted, const std::vector<float>& candH,
                  float* outH) {
  const uint32_t cells = g.cells();
  const int terms = sh_terms(lmax), n3 = 3 * terms;
  const uint32_t nl = sc->d.nlights;
  std::vector<DLight> lights(nl);
  if (nl) HIP_TRY(hipMemcpy(lights.data(), sc->lights.p, nl * sizeof(DLight), hipMemcpyDeviceToHost));
  int nmc = 0;
  for (uint32_t li = 0; li < nl; ++li) nmc += lights[li].kind != DR_LIGHT_POINT;
  // the accepted candidates, cell by cell, and their draws: three randomUint per non-point light and candidate from RNG(cell), in scene order
  std::vector<uint32_t> cellFirst(cells), scrH;
  std::vector<float> ptsH;
  for (uint32_t c = 0; c < cells; ++c) {
    cellFirst[c] = (uint32_t)(ptsH.size() / 3);
    DartRandom rng;
    rng.seed((int64_t)c);
    for (int k = 0; k < nfound[c]; ++k) {
      const float* p = candH.data() + ((size_t)c * kCandidates + (size_t)accepted[(size_t)c * kMaxFound + (size_t)k]) * 3;
      ptsH.insert(ptsH.end(), p, p + 3);
      for (int q = 0; q < 3 * nmc; ++q) scrH.push_back(rng.randomUint());
    }
  }
  const uint32_t nprobes = (uint32_t)(ptsH.size() / 3);
  double K[DR_SH_MAX_TERMS];
  sh_K_table(lmax, K);
  DevBuf<double> dK;
  DevBuf<float> dPts, cd, contrib, dOut;
  DevBuf<uint32_t> dScr, dFirst;
  DevBuf<int32_t> dFound;
  TraceBufs T;
  HIP_TRY(dK.alloc(DR_SH_MAX_TERMS));
  HIP_TRY(hipMemcpy(dK.p, K, terms * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(dPts.alloc(ptsH.size()));
  HIP_TRY(dScr.alloc(scrH.size()));
  HIP_TRY(cd.alloc((size_t)nprobes * n3));
  HIP_TRY(dOut.alloc((size_t)cells * n3));
  HIP_TRY(dFirst.alloc(cells));
  HIP_TRY(dFound.alloc(cells));
  if (nprobes) {
    HIP_TRY(hipMemcpy(dPts.p, ptsH.data(), ptsH.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!scrH.empty()) HIP_TRY(hipMemcpy(dScr.p, scrH.data(), scrH.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(cd.p, 0, (size_t)nprobes * n3 * sizeof(float)));
  }
  HIP_TRY(hipMemcpy(dFirst.p, cellFirst.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dFound.p, nfound.data(), cells * sizeof(int32_t), hipMemcpyHostToDevice));
  constexpr uint32_t kSlice = 1u << 16;  // samples of one launch: the contribution table holds kSlice * 3 Terms floats
  int rc = traceInit(sc, T, kSlice);
  if (rc) return rc;
  HIP_TRY(contrib.alloc((size_t)kSlice * n3));
  ProbeProj a;
  memset(&a, 0, sizeof(a));
  a.lmax = lmax;
  a.K = dK.p;
  a.pts = dPts.p;
  a.scr = dScr.p;
  a.nmc = nmc;
  int mc = 0;
  for (uint32_t li = 0; li < nl && nprobes; ++li) {
    const DLight& L = lights[li];
    a.light = (int32_t)li;
    if (L.kind == DR_LIGHT_POINT) {
      a.mode = PROBE_POINT;
      a.ns = 1;
    } else {
      a.mode = PROBE_MC;
      uint32_t ns = 1;
      while (ns < (uint32_t)std::max(1, L.kind >= DR_LIGHT_POINT ? 1 : L.nsamples)) ns <<= 1;  // RoundUpPow2(nSamples)
      if (ns > kSlice) return fail(DR_ERR_UNSUPPORTED, "create probes: a light's nsamples above 65536");
      a.ns = (int32_t)ns;
      a.mc = mc++;
    }
    const uint32_t per = kSlice / (uint32_t)a.ns;  // probes of one launch
    for (uint32_t first = 0; first < nprobes; first += per) {
      const uint32_t count = std::min(per, nprobes - first);
      const size_t total = (size_t)count * (size_t)a.ns;
      hipLaunchKernelGGL(k_probe_contrib, blocks(total, 128), dim3(128), 0, nullptr, sc->d, a, first, count, contrib.p, T.rays.p);
      rc = trace(sc, T, total, 1);
      if (rc) return rc;
      hipLaunchKernelGGL(k_probe_sum, blocks((size_t)count * n3, 256), dim3(256), 0, nullptr, contrib.p, T.hits.p, first, count, a.ns, n3, cd.p);
    }
  }
  hipLaunchKernelGGL(k_probe_finish, blocks((size_t)cells * n3, 256), dim3(256), 0, nullptr, cd.p, dFirst.p, dFound.p, cells, lmax, dOut.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(outH, dOut.p, (size_t)cells * n3 * sizeof(float), hipMemcpyDeviceToHost));
  return DR_OK;
}

const char* bakeRefusal(const DrProbesDesc* d) {
  if (d->lmax < 1 || d->lmax > DR_SH_LMAX_MAX) return "create probes: lmax must be in 1 .. 8";
  if (d->include_indirect)
    return "create probes: indirectlighting is not supported (ProjectIncidentIndirectRadiance runs renderer.Li per probe direction: a full render per probe); "
           "bake with indirectlighting false";
  return nullptr;
}

}  // namespace

extern "C" {

int dr_probes_surface_points(DrScene* sc, const float camera_pos[3], double time, int32_t npoints, float* out, int32_t* count_out) {
  (void)time;  // (no shape of the device path moves)
  if (!sc || !camera_pos || !out || !count_out) return fail(DR_ERR_INVALID, "null argument");
  std::vector<float> pts;
  const int rc = surfacePoints(sc, camera_pos, npoints, pts);
  if (rc) return rc;
  memcpy(out, pts.data(), pts.size() * sizeof(float));  // at most npoints + 31 points
  *count_out = (int32_t)(pts.size() / 3);
  return DR_OK;
}

int dr_probes_grid(const DrScene* sc, const DrProbesDesc* desc, int32_t nprobes_out[3], float bounds_out[6]) {
  if (!sc || !desc || !nprobes_out) return fail(DR_ERR_INVALID, "null argument");
  Grid g;
  const int rc = makeGrid(sc, desc->has_bounds ? desc->bounds : nullptr, desc->spacing, &g);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k) nprobes_out[k] = g.n[k];
  if (bounds_out) memcpy(bounds_out, g.b, sizeof(g.b));
  return DR_OK;
}

int dr_probes_candidates(DrScene* sc, const DrProbesDesc* desc, const float* points, int32_t npoints, int32_t* nfound_out, int32_t* accepted_out) {
  if (!sc || !desc || !points || !nfound_out || !accepted_out) return fail(DR_ERR_INVALID, "null argument");
  if (npoints < 1 || npoints > (1 << 22) + 31) return fail(DR_ERR_INVALID, "create probes: npoints must be in 1 .. 2^22 (+ the walks' overshoot of 31)");
  Grid g;
  int rc = makeGrid(sc, desc->has_bounds ? desc->bounds : nullptr, desc->spacing, &g);
  if (rc) return rc;
  std::vector<float> pts(points, points + 3 * (size_t)npoints), cand;
  std::vector<int32_t> nfound, accepted;
  rc = acceptCandidates(sc, g, pts, nfound, accepted, cand);
  if (rc) return rc;
  memcpy(nfound_out, nfound.data(), nfound.size() * sizeof(int32_t));
  memcpy(accepted_out, accepted.data(), accepted.size() * sizeof(int32_t));
  return DR_OK;
}

int dr_probes_bake(DrScene* sc, const DrProbesDesc* desc, float* out, int64_t nfloats) {
  if (!desc) return fail(DR_ERR_INVALID, "null argument");
  if (const char* why = bakeRefusal(desc)) return fail(desc->lmax >= 1 && desc->lmax <= DR_SH_LMAX_MAX ? DR_ERR_UNSUPPORTED : DR_ERR_INVALID, why);  // (needs no scene)
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  Grid g;
  int rc = makeGrid(sc, desc->has_bounds ? desc->bounds : nullptr, desc->spacing, &g);
  if (rc) return rc;
  const int64_t need = 15 + (int64_t)g.cells() * sh_terms(desc->lmax) * 3;
  if (nfloats != need) return fail(DR_ERR_INVALID, "create probes: the output holds " + std::to_string(nfloats) + " floats, the grid needs " + std::to_string(need));
  std::vector<float> pts, cand;
  rc = surfacePoints(sc, desc->camera_pos, desc->npoints, pts);
  if (rc) return rc;
  std::vector<int32_t> nfound, accepted;
  rc = acceptCandidates(sc, g, pts, nfound, accepted, cand);
  if (rc) return rc;
  memset(out, 0, (size_t)need * sizeof(float));
  out[0] = (float)desc->lmax;
  out[1] = 1.f;  // includeDirectInProbes
  out[2] = 0.f;  // includeIndirectInProbes
  for (int k = 0; k < 3; ++k) out[3 + k] = (float)g.n[k];
  for (int k = 0; k < 6; ++k) out[6 + k] = g.b[k];
  return projectProbes(sc, g, desc->lmax, nfound, accepted, cand, out + 12);  // (the three floats behind the coefficients stay 0, as the reference leaves them)
}

int dr_scene_set_probes(DrScene* sc, const float* data, int64_t n) {
  // (the header first: what is wrong with a grid can be asked without a device or a scene)
  if (data)
    if (const char* why = probesHeaderRefusal(data, n)) return fail(DR_ERR_INVALID, why);
  if (!sc) return fail(DR_ERR_INVALID, "null argument");
  if (!data) {  // no grid
    sc->probes.lmax = 0;
    return DR_OK;
  }
  auto& P = sc->probes;
  P.lmax = 0;
  double K[DR_SH_MAX_TERMS];
  const int lmax = (int)data[0];
  sh_K_table(lmax, K);
  HIP_TRY(P.K.alloc(DR_SH_MAX_TERMS));
  HIP_TRY(hipMemcpy(P.K.p, K, sh_terms(lmax) * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(P.cin.alloc((size_t)(n - 15)));
  HIP_TRY(hipMemcpy(P.cin.p, data + 12, (size_t)(n - 15) * sizeof(float), hipMemcpyHostToDevice));
  P.includeDirect = (int)data[1];
  for (int k = 0; k < 3; ++k) P.n[k] = (int)data[3 + k];
  for (int k = 0; k < 6; ++k) P.b[k] = data[6 + k];
  P.lmax = lmax;
  return DR_OK;
}

}  // extern "C"
