// dr_prt_project.hip -- DiffusePRTIntegrator.preprocess (surface_integrators/diffuse_prt_integrator.dart:33-40) on the device:
// SphericalHarmonics.ProjectIncidentDirectRadiance (core/spherical_harmonics.dart:145-170) of every light's direct radiance at the centre of
// the scene's world bound, without visibility, into c_in[Terms(lmax)] (RGB, f32 Spectrum stores), then ReduceRinging.  Also the C entry points
// dr_prt_incident and dr_sh_evaluate.
//
// Every coefficient of the reference is a SERIAL f32 sum over a light's samples (or texels, or cube directions), so the order of the additions is
// part of the result.  Two kernels keep it:
//   k_prt_contrib   one lane per sample: the sample's rounded contribution to every (term, channel), contrib[sample][term * 3 + channel], for a
//                   CHUNK of samples (a 1024 x 512 map never needs its whole table at once);
//   k_prt_sum       one lane per (term, channel): walks the chunk's contributions in sample order, acc = f32(acc + contribution).
// A sample the reference skips (black radiance, pdf 0) contributes +0, which leaves an accumulator that started at +0 as it is.
// Per light kind:
//   PointLight         the analytic override (point_light.dart:75-97): Li * Ylm, Ylm in f64, no draws;
//   Spot / Distant / DiffuseArea   Light.shProject (light.dart:98-131): ns = RoundUpPow2(nSamples) samples, one randomUint for the 1-D scramble and
//                      two for the 2-D one (host, the one RNG(5489) of the preprocess, lights in scene order), sampleLAtPoint at the centre,
//                      Evaluate into a Float32List (every store of the recurrences rounds to f32);
//   InfiniteAreaLight  (infinite_area_light.dart:207-281) lat-long over the level-0 texels when both sides of the map exceed 50 -- f32 sine /
//                      cosine tables built on the host (the host libm's values), f32 Ylm -- else ProjectCube at resolution 200: six faces per
//                      (u, v) in the reference's order, f64 Ylm, Le of the direction, dA per (u, v) tabulated on the host (Math.pow).
// The light sampling is what k_shade_whitted does per light, with the device functions it calls (dr_device.h).
#include <string.h>

#include <vector>

#include "dr_host.h"
#include "dr_rng.h"
#include "dr_li_sampling.h"

using namespace dr_host;

namespace {

enum { PRT_POINT = 0, PRT_MC = 1, PRT_LATLONG = 2, PRT_CUBE = 3 };
struct PrtProj {
  int32_t mode, light, lmax, ns;
  uint32_t scr1, scr2[2];
  float p[3];
  const double* K;
  const float* trig;  // lat-long: sin theta [h], cos theta [h], sin phi [w], cos phi [w] (f32, host libm)
  const double* dA;   // cube: [res][res]
  double thetaPhiPi;  // lat-long: (pi / ntheta) * ((2 pi) / nphi)
  int32_t res;
};

__global__ void __launch_bounds__(128) k_prt_contrib(DScene sc, PrtProj a, uint32_t first, uint32_t count, float* contrib) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= count) return;
  const uint32_t i = first + tid;
  const int terms = sh_terms(a.lmax);
  float* out = contrib + (size_t)tid * (size_t)(3 * terms);
  const F3 p = F3{a.p[0], a.p[1], a.p[2]};
  auto put = [&](int j, C3 v) {
    out[3 * j] = v.r;
    out[3 * j + 1] = v.g;
    out[3 * j + 2] = v.b;
  };
  if (a.mode == PRT_POINT) {
    const DLight light = sc.lights[a.light];
    const F3 lp = F3{light.pos[0], light.pos[1], light.pos[2]};
    const F3 seg = vsub(lp, p);
    const F3 wi = vnormalize(seg);
    double Ylm[DR_SH_MAX_TERMS];
    sh_evaluate((double)wi.x, (double)wi.y, (double)wi.z, a.lmax, a.K, Ylm);
    const C3 Li = cdivD(C3{light.L[0], light.L[1], light.L[2]}, vlen2(seg));  // intensity / DistanceSquared(lightPos, p)
    for (int j = 0; j < terms; ++j) put(j, cmulD(Li, Ylm[j]));
  } else if (a.mode == PRT_MC) {
    const GlobalLights lv = GlobalLights{sc.lights, sc.ltris, sc.lcdf, sc.mats};
    const DLight light = sc.lights[a.light];
    double u[2];
    Sample02(i, a.scr2, u);
    const double uc = scrambled_radical(i, a.scr1, false);  // VanDerCorput(i, scramble1D)
    F3 wi = F3{0, 0, 0};
    double pdf = 0.0;
    C3 Li;
    if (light.kind >= DR_LIGHT_POINT) {  // SpotLight (spot_light.dart:54-85), DistantLight (distant_light.dart:54-61): pdf = 1
      const F3 lp = F3{light.pos[0], light.pos[1], light.pos[2]};
      pdf = 1.0;
      if (light.kind == DR_LIGHT_DISTANT) {
        wi = lp;
        Li = C3{light.L[0], light.L[1], light.L[2]};
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
      }
    } else {  // DiffuseAreaLight.sampleLAtPoint (diffuse_area_light.dart:60-70); the infinite light never comes here (prtIncident: lat-long / cube)
      F3 ns;
      const F3 ps = shapeset_sample<true>(sc, lv, light, u[0], u[1], uc, &ns, p);
      wi = vnormalize(vsub(ps, p));
      pdf = shapeset_pdf<true>(sc, lv, light, p, wi);
      Li = light_L(light, ns, vneg(wi));
    }
    if (!cblack(Li) && pdf > 0.0) {
      float Ylm[DR_SH_MAX_TERMS];
      sh_evaluate((double)wi.x, (double)wi.y, (double)wi.z, a.lmax, a.K, Ylm);
      const double den = pdf * a.ns;
      for (int j = 0; j < terms; ++j) put(j, cdivD(cmulD(Li, (double)Ylm[j]), den));  // Li * Ylm[j] / (pdf * ns)
    } else {
      for (int j = 0; j < terms; ++j) put(j, C3{0.f, 0.f, 0.f});
    }
  } else if (a.mode == PRT_LATLONG) {
    const DEnv& e = sc.env;
    const int theta = (int)(i / (uint32_t)e.w), phi = (int)(i % (uint32_t)e.w);
    const double st = a.trig[theta], ct = a.trig[e.h + theta], sp = a.trig[2 * e.h + phi], cp = a.trig[2 * e.h + e.w + phi];
    F3 w = f3(st * cp, st * sp, ct);
    w = vnormalize(xf3(e.l2w, w));
    const C3 Le = env_texel(e, phi, theta);  // radianceMap.texel(0, phi, theta)
    float Ylm[DR_SH_MAX_TERMS];
    sh_evaluate((double)w.x, (double)w.y, (double)w.z, a.lmax, a.K, Ylm);
    for (int j = 0; j < terms; ++j) put(j, cmulD(Le, (double)Ylm[j] * st * a.thetaPhiPi));  // Le * (Ylm[i] * sintheta * theta_phi_pi)
  } else {
    const uint32_t cell = i / 6u, face = i % 6u;
    const int res = a.res;
    const int u = (int)(cell / (uint32_t)res), v = (int)(cell % (uint32_t)res);
    const double fu = -1.0 + 2.0 * (u + 0.5) / res, fv = -1.0 + 2.0 * (v + 0.5) / res;
    F3 w;
    switch (face) {  // spherical_harmonics.dart:98-135
      case 0: w = f3(fu, fv, 1.0); break;
      case 1: w = f3(fu, fv, -1.0); break;
      case 2: w = f3(fu, 1.0, fv); break;
      case 3: w = f3(fu, -1.0, fv); break;
      case 4: w = f3(1.0, fu, fv); break;
      default: w = f3(-1.0, fu, fv); break;
    }
    const F3 wn = vnormalize(w);
    double Ylm[DR_SH_MAX_TERMS];
    sh_evaluate((double)wn.x, (double)wn.y, (double)wn.z, a.lmax, a.K, Ylm);
    const C3 f = env_Le(sc.env, w);  // light.Le(Ray(p, w))
    const double dA = a.dA[cell];
    const double k4 = 4.0 / (res * res);
    for (int j = 0; j < terms; ++j)
      put(j, face == 0 ? cmulD(cmulD(cmulD(f, dA), Ylm[j]), k4) : cmulD(cmulD(cmulD(f, Ylm[j]), dA), k4));  // f * dA * Ylm (+z) / f * Ylm * dA
  }
}

// acc[tc] = f32(acc[tc] + contrib[i][tc]) for i = 0 .. count - 1, in that order: one lane per (term, channel)
__global__ void __launch_bounds__(256) k_prt_sum(const float* contrib, uint32_t count, int n3, float* acc) {
  const int tc = (int)threadIdx.x;
  if (tc >= n3) return;
  float a = acc[tc];
  const float* p = contrib + tc;
  uint32_t i = 0;
  for (; i + 8 <= count; i += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[(size_t)(i + k) * n3];
#pragma unroll
    for (int k = 0; k < 8; ++k) a = a + v[k];
  }
  for (; i < count; ++i) a = a + p[(size_t)i * n3];
  acc[tc] = a;
}
// c_d[j] += c[j] (spherical_harmonics.dart:164-166); last: ReduceRinging (:219-226), c[Index(l, m)].scale(1 / (1 + lambda l^2 (l + 1)^2))
__global__ void __launch_bounds__(256) k_prt_add(const float* c, int n3, float* cd) {
  const int tc = (int)threadIdx.x;
  if (tc < n3) cd[tc] = cd[tc] + c[tc];
}
__global__ void __launch_bounds__(256) k_prt_ringing(float* cd, int lmax) {
  const int tc = (int)threadIdx.x;
  if (tc >= 3 * sh_terms(lmax)) return;
  const int j = tc / 3;
  int l = 0;
  while ((l + 1) * (l + 1) <= j) ++l;
  cd[tc] = (float)((double)cd[tc] * sh_ringing_scale(l, 0.005));
}

uint32_t roundUpPow2(uint32_t v) {
  uint32_t n = 1;
  while (n < v) n <<= 1;
  return n;
}

}  // namespace

namespace dr_host {

int prtIncident(DrScene* sc, int lmax, double shutterOpen, hipStream_t s) {
  (void)shutterOpen;  // (the time of sampleLAtPoint: no light of the device path reads it)
  const int terms = sh_terms(lmax), n3 = 3 * terms;
  if (sc->prt.lmax == lmax && sc->prt.cin.p) return DR_OK;
  sc->prt.lmax = 0;
  double K[DR_SH_MAX_TERMS];
  sh_K_table(lmax, K);
  HIP_TRY(sc->prt.K.alloc(DR_SH_MAX_TERMS));
  HIP_TRY(hipMemcpyAsync(sc->prt.K.p, K, terms * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(sc->prt.cin.alloc(3 * DR_SH_MAX_TERMS));
  HIP_TRY(hipMemsetAsync(sc->prt.cin.p, 0, n3 * sizeof(float), s));
  const uint32_t nl = sc->d.nlights;
  std::vector<DLight> lights(nl);
  if (nl) HIP_TRY(hipMemcpy(lights.data(), sc->lights.p, nl * sizeof(DLight), hipMemcpyDeviceToHost));
  constexpr uint32_t kChunk = 8192;
  DevBuf<float> contrib, acc, trig;
  DevBuf<double> dA;
  HIP_TRY(acc.alloc(n3));
  std::vector<float> trigH;  // (host staging outlives the asynchronous copies: the function waits for the stream before it returns)
  std::vector<double> dAH;
  // Point p = bbox.pMin * 0.5 + bbox.pMax * 0.5: Point stores are f32
  PrtProj a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < 3; ++k) a.p[k] = (float)((double)(float)((double)sc->d.rootBox[k] * 0.5) + (double)(float)((double)sc->d.rootBox[3 + k] * 0.5));
  a.lmax = lmax;
  a.K = sc->prt.K.p;
  DartRandom rng;
  rng.seed(5489);  // new RNG() (rng.dart:27-30)
  for (uint32_t li = 0; li < nl; ++li) {
    const DLight& L = lights[li];
    a.light = (int32_t)li;
    uint64_t total = 1;
    if (L.kind == DR_LIGHT_POINT) {
      a.mode = PRT_POINT;
    } else if (L.kind == DR_LIGHT_INFINITE) {
      const int w = sc->d.env.w, h = sc->d.env.h;
      if (std::min(w, h) > 50) {
        a.mode = PRT_LATLONG;
        trigH.resize(2 * (size_t)h + 2 * (size_t)w);
        for (int t = 0; t < h; ++t) {
          trigH[t] = (float)sin((t + 0.5) / h * DR_PI);
          trigH[h + t] = (float)cos((t + 0.5) / h * DR_PI);
        }
        for (int ph = 0; ph < w; ++ph) {
          trigH[2 * h + ph] = (float)sin((ph + 0.5) / w * 2.0 * DR_PI);
          trigH[2 * h + w + ph] = (float)cos((ph + 0.5) / w * 2.0 * DR_PI);
        }
        HIP_TRY(trig.alloc(trigH.size()));
        HIP_TRY(hipMemcpyAsync(trig.p, trigH.data(), trigH.size() * sizeof(float), hipMemcpyHostToDevice, s));
        a.trig = trig.p;
        a.thetaPhiPi = (DR_PI / h) * ((2.0 * DR_PI) / w);
        total = (uint64_t)w * (uint64_t)h;
      } else {
        a.mode = PRT_CUBE;
        a.res = 200;
        dAH.resize((size_t)a.res * a.res);
        for (int u = 0; u < a.res; ++u)
          for (int v = 0; v < a.res; ++v) {
            const double fu = (float)(-1.0 + 2.0 * (u + 0.5) / a.res), fv = (float)(-1.0 + 2.0 * (v + 0.5) / a.res);  // Vector(fu, fv, 1.0): f32 stores
            dAH[(size_t)u * a.res + v] = 1.0 / pow(fu * fu + fv * fv + 1.0 * 1.0, 3.0 / 2.0);
          }
        HIP_TRY(dA.alloc(dAH.size()));
        HIP_TRY(hipMemcpyAsync(dA.p, dAH.data(), dAH.size() * sizeof(double), hipMemcpyHostToDevice, s));
        a.dA = dA.p;
        total = (uint64_t)a.res * a.res * 6;
      }
    } else {
      a.mode = PRT_MC;
      a.ns = (int32_t)roundUpPow2((uint32_t)std::max(1, L.kind >= DR_LIGHT_POINT ? 1 : L.nsamples));
      a.scr1 = rng.randomUint();
      a.scr2[0] = rng.randomUint();
      a.scr2[1] = rng.randomUint();
      total = (uint64_t)a.ns;
    }
    HIP_TRY(hipMemsetAsync(acc.p, 0, n3 * sizeof(float), s));  // coeffs[i] = Spectrum(0): the scratch list, zeroed again by every light
    HIP_TRY(contrib.alloc((size_t)std::min<uint64_t>(total, kChunk) * n3));
    for (uint64_t first = 0; first < total; first += kChunk) {
      const uint32_t count = (uint32_t)std::min<uint64_t>(kChunk, total - first);
      hipLaunchKernelGGL(k_prt_contrib, dim3((count + 127) / 128), dim3(128), 0, s, sc->d, a, (uint32_t)first, count, contrib.p);
      hipLaunchKernelGGL(k_prt_sum, dim3(1), dim3(256), 0, s, contrib.p, count, n3, acc.p);
    }
    hipLaunchKernelGGL(k_prt_add, dim3(1), dim3(256), 0, s, acc.p, n3, sc->prt.cin.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));  // (the next light may rebuild the host tables and the chunk buffer)
  }
  hipLaunchKernelGGL(k_prt_ringing, dim3(1), dim3(256), 0, s, sc->prt.cin.p, lmax);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  sc->prt.lmax = lmax;
  return DR_OK;
}

}  // namespace dr_host

extern "C" {

int dr_prt_incident(DrScene* sc, int32_t lmax, double shutter_open, float* out) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  if (const char* why = prtRefusal(lmax, 1, false)) return fail(DR_ERR_INVALID, why);
  const int rc = prtIncident(sc, lmax, shutter_open, nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, sc->prt.cin.p, 3 * sh_terms(lmax) * sizeof(float), hipMemcpyDeviceToHost));
  return DR_OK;
}

int dr_sh_evaluate(const double* dirs, int64_t n, int32_t lmax, double* out) {
  if (!dirs || !out || n < 0) return fail(DR_ERR_INVALID, "null argument");
  if (const char* why = prtRefusal(lmax, 1, false)) return fail(DR_ERR_INVALID, why);
  double K[DR_SH_MAX_TERMS];
  sh_K_table(lmax, K);
  const int terms = sh_terms(lmax);
  for (int64_t i = 0; i < n; ++i) sh_evaluate(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], lmax, K, out + (size_t)i * terms);
  return DR_OK;
}

}  // extern "C"
