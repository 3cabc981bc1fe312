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
#include "dr_gprt.h"
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

// ---- the glossy PRT integrator's BSDF matrix ----
struct GprtBsdf {
  float Kd[3], Ks[3];
  double bexp, pdfN;
};
// w[i] = UniformSampleSphere(Sample02(i, scramble)) and Evaluate(w[i], lmax, Ylm, lmax_terms * i) into the Float32List: one lane per direction
__global__ void __launch_bounds__(128) k_gprt_dirs(uint32_t scr0, uint32_t scr1, int n, int lmax, const double* K, float* w, float* Y) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const uint32_t scramble[2] = {scr0, scr1};
  float v[3];
  sh_sample_sphere((uint32_t)i, scramble, v);
  float Yl[DR_SH_MAX_TERMS];
  sh_evaluate((double)v[0], (double)v[1], (double)v[2], lmax, K, Yl);
  const int terms = sh_terms(lmax);
  for (int k = 0; k < 3; ++k) w[3 * (size_t)i + k] = v[k];
  for (int k = 0; k < terms; ++k) Y[(size_t)i * terms + k] = Yl[k];
}
// f[osamp][isamp]: one lane per pair
__global__ void __launch_bounds__(256) k_gprt_pairs(GprtBsdf b, int n, const float* w, float* f) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (uint32_t)n * (uint32_t)n) return;
  const uint32_t o = idx / (uint32_t)n, i = idx % (uint32_t)n;
  sh_bsdf_pair(b.Kd, b.Ks, b.bexp, w + 3 * (size_t)o, w + 3 * (size_t)i, b.pdfN, f + 3 * (size_t)idx);
}
// B[i][j][ch] = the serial f32 sum over osamp, then isamp, of f * (Ylm[isamp][j] * Ylm[osamp][i]): one lane per (i, j, channel)
__global__ void __launch_bounds__(64) k_gprt_bsum(int n, int terms, const float* Y, const float* f, float* B) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= 3 * terms * terms) return;
  const int ch = t % 3, j = (t / 3) % terms, i = t / (3 * terms);
  float acc = 0.f;
  for (int o = 0; o < n; ++o) {
    const float Yoi = Y[(size_t)o * terms + i];
    const float* fo = f + (size_t)o * n * 3 + ch;
    int is = 0;
    for (; is + 8 <= n; is += 8) {
      float fv[8], yv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        fv[k] = fo[3 * (size_t)(is + k)];
        yv[k] = Y[(size_t)(is + k) * terms + j];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = sh_bsdf_step(acc, fv[k], yv[k], Yoi);
    }
    for (; is < n; ++is) acc = sh_bsdf_step(acc, fo[3 * (size_t)is], Y[(size_t)is * terms + j], Yoi);
  }
  B[t] = acc;
}
// dr_sh_rotate_device: sh_to_zyz and sh_rotate_channel by one lane per (frame, channel)
__global__ void __launch_bounds__(64) k_gprt_rotate(const float* c_in, const float* m16, int lmax, int nframes, float* out) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= 3 * nframes) return;
  const int fr = t / 3, ch = t % 3, terms = sh_terms(lmax);
  double alpha, beta, gamma;
  sh_to_zyz(m16 + 16 * (size_t)fr, &alpha, &beta, &gamma);
  sh_rotate_channel(c_in + (size_t)fr * terms * 3 + ch, 3, alpha, beta, gamma, lmax, out + (size_t)fr * terms * 3 + ch);
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
  // GlossyPRTIntegrator.preprocess hands the SAME RNG to ComputeBSDFMatrix (glossy_prt_integrator.dart:42-48): its scramble is the two draws behind
  // whatever the lights consumed (the draws do not depend on lmax)
  sc->prt.after[0] = rng.randomUint();
  sc->prt.after[1] = rng.randomUint();
  return DR_OK;
}

// ComputeBSDFMatrix (core/spherical_harmonics.dart:609-672) in the two-kernel pattern above: the directions and their Float32List harmonics, then
// f * |cos| / pdf_nSamples of every (osamp, isamp) pair (black: +0), then one lane per (i, j, channel) adding the pairs in the reference's order.
int gprtBsdfMatrix(DrScene* sc, int lmax, int ns, double shutterOpen, hipStream_t s) {
  int rc = prtIncident(sc, lmax, shutterOpen, s);
  if (rc) return rc;
  auto& g = sc->gprt;
  if (g.B.p && g.lmax == lmax && g.ns == ns && memcmp(g.keyKd, g.Kd, sizeof(g.Kd)) == 0 && memcmp(g.keyKs, g.Ks, sizeof(g.Ks)) == 0 &&
      memcmp(&g.keyRoughness, &g.roughness, sizeof(double)) == 0)
    return DR_OK;
  g.lmax = 0;
  const int terms = sh_terms(lmax);
  DevBuf<float> w, Y, f;
  HIP_TRY(w.alloc((size_t)ns * 3));
  HIP_TRY(Y.alloc((size_t)ns * terms));
  HIP_TRY(f.alloc((size_t)ns * ns * 3));
  HIP_TRY(g.B.alloc((size_t)3 * DR_GPRT_MAX_TERMS * DR_GPRT_MAX_TERMS));
  GprtBsdf b;
  memcpy(b.Kd, g.Kd, sizeof(b.Kd));
  memcpy(b.Ks, g.Ks, sizeof(b.Ks));
  b.bexp = sh_blinn_exponent(g.roughness);
  b.pdfN = sh_bsdf_pdf_nsamples(ns);
  hipLaunchKernelGGL(k_gprt_dirs, dim3((ns + 127) / 128), dim3(128), 0, s, sc->prt.after[0], sc->prt.after[1], ns, lmax, sc->prt.K.p, w.p, Y.p);
  const uint32_t npairs = (uint32_t)ns * (uint32_t)ns;
  hipLaunchKernelGGL(k_gprt_pairs, dim3((npairs + 255) / 256), dim3(256), 0, s, b, ns, w.p, f.p);
  const int nOut = 3 * terms * terms;
  hipLaunchKernelGGL(k_gprt_bsum, dim3((nOut + 63) / 64), dim3(64), 0, s, ns, terms, Y.p, f.p, g.B.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  g.lmax = lmax;
  g.ns = ns;
  memcpy(g.keyKd, g.Kd, sizeof(g.Kd));
  memcpy(g.keyKs, g.Ks, sizeof(g.Ks));
  g.keyRoughness = g.roughness;
  return DR_OK;
}

int gprtRotateDevice(const float* c_in, const float* m16, int lmax, int nframes, float* out) {
  const int terms = sh_terms(lmax);
  DevBuf<float> dc, dm, dout;
  HIP_TRY(dc.alloc((size_t)nframes * terms * 3));
  HIP_TRY(dm.alloc((size_t)nframes * 16));
  HIP_TRY(dout.alloc((size_t)nframes * terms * 3));
  HIP_TRY(hipMemcpy(dc.p, c_in, (size_t)nframes * terms * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dm.p, m16, (size_t)nframes * 16 * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_gprt_rotate, dim3((3 * nframes + 63) / 64), dim3(64), 0, nullptr, dc.p, dm.p, lmax, nframes, dout.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.p, (size_t)nframes * terms * 3 * sizeof(float), hipMemcpyDeviceToHost));
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

int dr_scene_set_glossy_prt(DrScene* sc, const DrGlossyPrtParams* p) {
  if (!sc || !p) return fail(DR_ERR_INVALID, "null argument");
  memcpy(sc->gprt.Kd, p->Kd, sizeof(p->Kd));
  memcpy(sc->gprt.Ks, p->Ks, sizeof(p->Ks));
  sc->gprt.roughness = p->roughness;
  return DR_OK;
}

int dr_prt_bsdf_matrix(DrScene* sc, int32_t lmax, int32_t nsamples_b, float* out) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  if (const char* why = gprtRefusal(lmax, 1, false)) return fail(DR_ERR_INVALID, why);
  if (nsamples_b < 1 || nsamples_b > 1024) return fail(DR_ERR_INVALID, "glossy PRT: the BSDF matrix's nsamples_b must be 1 to 1024");
  const int rc = gprtBsdfMatrix(sc, lmax, nsamples_b, 0.0, nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, sc->gprt.B.p, (size_t)3 * sh_terms(lmax) * sh_terms(lmax) * sizeof(float), hipMemcpyDeviceToHost));
  return DR_OK;
}

int dr_sh_rotate(const float* c_in, const float* m16, int32_t lmax, float* out) {
  if (!c_in || !m16 || !out) return fail(DR_ERR_INVALID, "null argument");
  if (const char* why = gprtRefusal(lmax, 1, false)) return fail(DR_ERR_INVALID, why);
  double alpha, beta, gamma;
  sh_to_zyz(m16, &alpha, &beta, &gamma);
  for (int ch = 0; ch < 3; ++ch) sh_rotate_channel(c_in + ch, 3, alpha, beta, gamma, lmax, out + ch);
  return DR_OK;
}

int dr_sh_rotate_device(const float* c_in, const float* m16, int32_t lmax, int32_t nframes, float* out) {
  if (!c_in || !m16 || !out || nframes < 1) return fail(DR_ERR_INVALID, "null argument");
  if (const char* why = gprtRefusal(lmax, 1, false)) return fail(DR_ERR_INVALID, why);
  return gprtRotateDevice(c_in, m16, lmax, nframes, out);
}

int dr_sh_bsdf_matrix_host(const float* Kd, const float* Ks, double roughness, const uint32_t* scramble, int32_t nsamples_b, int32_t lmax, float* out) {
  if (!Kd || !Ks || !scramble || !out) return fail(DR_ERR_INVALID, "null argument");
  if (const char* why = gprtRefusal(lmax, 1, false)) return fail(DR_ERR_INVALID, why);
  if (nsamples_b < 1 || nsamples_b > 1024) return fail(DR_ERR_INVALID, "glossy PRT: the BSDF matrix's nsamples_b must be 1 to 1024");
  const int terms = sh_terms(lmax), n = nsamples_b;
  double K[DR_SH_MAX_TERMS];
  sh_K_table(lmax, K);
  std::vector<float> w((size_t)n * 3), Y((size_t)n * terms);
  for (int i = 0; i < n; ++i) {
    sh_sample_sphere((uint32_t)i, scramble, &w[3 * (size_t)i]);
    sh_evaluate((double)w[3 * (size_t)i], (double)w[3 * (size_t)i + 1], (double)w[3 * (size_t)i + 2], lmax, K, &Y[(size_t)i * terms]);
  }
  const double bexp = sh_blinn_exponent(roughness), pdfN = sh_bsdf_pdf_nsamples(n);
  for (int k = 0; k < 3 * terms * terms; ++k) out[k] = 0.f;
  for (int o = 0; o < n; ++o)
    for (int is = 0; is < n; ++is) {
      float f[3];
      sh_bsdf_pair(Kd, Ks, bexp, &w[3 * (size_t)o], &w[3 * (size_t)is], pdfN, f);
      if (!(f[0] != 0.0f || f[1] != 0.0f || f[2] != 0.0f)) continue;
      for (int i = 0; i < terms; ++i)
        for (int j = 0; j < terms; ++j)
          for (int ch = 0; ch < 3; ++ch)
            out[(size_t)(i * terms + j) * 3 + ch] = sh_bsdf_step(out[(size_t)(i * terms + j) * 3 + ch], f[ch], Y[(size_t)is * terms + j], Y[(size_t)o * terms + i]);
    }
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
