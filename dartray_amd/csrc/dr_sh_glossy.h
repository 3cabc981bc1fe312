// dr_sh_glossy.h -- what GlossyPRTIntegrator (surface_integrators/glossy_prt_integrator.dart:23-134) adds to dr_sh.h, shared by host and device
// (DESIGN.md 2.17): SphericalHarmonics.Rotate with _toZYZ, RotateZ, RotateXPlus, RotateXMinus (core/spherical_harmonics.dart:228-347, 782-794) and
// one (wo, wi) pair of ComputeBSDFMatrix (:609-672).  Written from the reference's text, operator for operator, like dr_sh.h.
//
// lmax range: 1 <= lmax <= DR_GPRT_LMAX_MAX (4).  The x-rotation rows are restated band by band, and at lmax 4 the 325 distinct elements of a
// hit's transfer matrix fit one wave's registers (dr_shade_gprt.hip); bands 5 to 8 are not served.
//
// Rotate is NOT a rotation ("Reference quirks that are reproduced").  A Dart list holds object references: RotateXPlus stores its
// input's Spectrum OBJECTS for the rows that are one term with factor one (`c_out[oi++] = c_in[0]`, `= O(1, 0)`, `= O(1, 1)`, `= O(2, 1)`),
// RotateZ writes INTO existing objects for m = 0 (`c_out[Index(l, 0)].copy(..)`) and rebinds the other entries to fresh objects, RotateXMinus
// scales objects in place.  Inside Rotate the lists c_out and work therefore share objects, and a later `.copy` or `.scale` changes what an
// earlier row still reads.  The functions below keep the reference's object identity: a list is an array of POINTERS into a pool of values, an
// assignment rebinds a pointer, `.copy` and `.scale` write through one.  The three channels never mix, so a channel is rotated on its own.
#ifndef DR_SH_GLOSSY_H
#define DR_SH_GLOSSY_H

#include <stdint.h>

#include "dr_sh.h"

#define DR_GPRT_LMAX_MAX 4
#define DR_GPRT_MAX_TERMS ((DR_GPRT_LMAX_MAX + 1) * (DR_GPRT_LMAX_MAX + 1))
#define DR_SH_FLT_EPSILON 1.19209290e-07  // core/common.dart:27
#define DR_SH_INV_PI 0.31830988618379067154     // :23
#define DR_SH_INV_TWOPI 0.15915494309189533577  // :24
#define DR_SH_PI 3.14159265358979323846
// the objects one Rotate makes at lmax 4: c_out and work (25 each), RotateZ's 2 l per band three times (60), RotateXPlus's 21 rows that are not
// a bare reference twice (42)
#define DR_SH_ROT_POOL 160

// _toZYZ (:782-794) of the Matrix4x4 m (sixteen f32, row major)
DR_SH_FN void sh_to_zyz(const float* m, double* alpha, double* beta, double* gamma) {
  const double sy = sqrt((double)m[9] * (double)m[9] + (double)m[8] * (double)m[8]);
  if (sy > 16 * DR_SH_FLT_EPSILON) {
    *gamma = -atan2((double)m[6], -(double)m[2]);
    *beta = -atan2(sy, (double)m[10]);
    *alpha = -atan2((double)m[9], (double)m[8]);
  } else {
    *gamma = 0.0;
    *beta = -atan2(sy, (double)m[10]);
    *alpha = -atan2(-(double)m[4], (double)m[5]);
  }
}

struct ShRotPool {
  float v[DR_SH_ROT_POOL];
  int n;
};
DR_SH_FN float* sh_rot_new(ShRotPool& P, float x) {  // a fresh Spectrum (one channel of it)
  float* p = &P.v[P.n++];
  *p = x;
  return p;
}
DR_SH_FN float sh_mulD(float c, double s) { return (float)((double)c * s); }           // Spectrum * double: one f32 store
DR_SH_FN float sh_add(float a, float b) { return (float)((double)a + (double)b); }    // Spectrum + Spectrum

// RotateZ (:244-271): c_out[0] and c_out[Index(l, 0)] are written INTO (`.copy`); every other entry is rebound to a fresh object
DR_SH_FN void sh_rotate_z(float* const* in, float** out, double alpha, int lmax, ShRotPool& P) {
  *out[0] = *in[0];
  double ct[DR_GPRT_LMAX_MAX + 1], st[DR_GPRT_LMAX_MAX + 1];
  sh_sincos_indexed(sin(alpha), cos(alpha), lmax + 1, st, ct);
  for (int l = 1; l <= lmax; ++l) {
    for (int m = -l; m < 0; ++m) out[sh_index(l, m)] = sh_rot_new(P, sh_add(sh_mulD(*in[sh_index(l, m)], ct[-m]), sh_mulD(*in[sh_index(l, -m)], -st[-m])));
    *out[sh_index(l, 0)] = *in[sh_index(l, 0)];
    for (int m = 1; m <= l; ++m) out[sh_index(l, m)] = sh_rot_new(P, sh_add(sh_mulD(*in[sh_index(l, m)], ct[m]), sh_mulD(*in[sh_index(l, -m)], st[m])));
  }
}

// RotateXPlus (:291-347): `= O(l, m)` binds the input's object itself; a unary minus or an arithmetic expression makes a fresh one
DR_SH_FN void sh_rotate_x_plus(float* const* in, float** out, int lmax, ShRotPool& P) {
#define O(l, m) in[sh_index(l, m)]
#define NEG(a) sh_rot_new(P, -*(a))
#define LIN2(a, x, b, y) sh_rot_new(P, sh_add(sh_mulD(*(a), x), sh_mulD(*(b), y)))
#define LIN3(a, x, b, y, c, z) sh_rot_new(P, sh_add(sh_add(sh_mulD(*(a), x), sh_mulD(*(b), y)), sh_mulD(*(c), z)))
  int oi = 0;
  out[oi++] = in[0];
  if (lmax < 1) return;
  out[oi++] = O(1, 0);
  out[oi++] = NEG(O(1, -1));
  out[oi++] = O(1, 1);
  if (lmax < 2) return;
  out[oi++] = O(2, 1);
  out[oi++] = NEG(O(2, -1));
  out[oi++] = LIN2(O(2, 0), -0.5, O(2, 2), -0.8660254037844386);
  out[oi++] = NEG(O(2, -2));
  out[oi++] = LIN2(O(2, 0), -0.8660254037844386, O(2, 2), 0.5);
  if (lmax < 3) return;
  out[oi++] = LIN2(O(3, 0), -0.7905694150420949, O(3, 2), 0.6123724356957945);
  out[oi++] = NEG(O(3, -2));
  out[oi++] = LIN2(O(3, 0), -0.6123724356957945, O(3, 2), -0.7905694150420949);
  out[oi++] = LIN2(O(3, -3), 0.7905694150420949, O(3, -1), 0.6123724356957945);
  out[oi++] = LIN2(O(3, 1), -0.25, O(3, 3), -0.9682458365518543);
  out[oi++] = LIN2(O(3, -3), -0.6123724356957945, O(3, -1), 0.7905694150420949);
  out[oi++] = LIN2(O(3, 1), -0.9682458365518543, O(3, 3), 0.25);
  if (lmax < 4) return;
  out[oi++] = LIN2(O(4, 1), -0.9354143466934853, O(4, 3), 0.35355339059327373);
  out[oi++] = LIN2(O(4, -3), -0.75, O(4, -1), 0.6614378277661477);
  out[oi++] = LIN2(O(4, 1), -0.35355339059327373, O(4, 3), -0.9354143466934853);
  out[oi++] = LIN2(O(4, -3), 0.6614378277661477, O(4, -1), 0.75);
  out[oi++] = LIN3(O(4, 0), 0.375, O(4, 2), 0.5590169943749475, O(4, 4), 0.739509972887452);
  out[oi++] = LIN2(O(4, -4), 0.9354143466934853, O(4, -2), 0.35355339059327373);
  out[oi++] = LIN3(O(4, 0), 0.5590169943749475, O(4, 2), 0.5, O(4, 4), -0.6614378277661477);
  out[oi++] = LIN2(O(4, -4), -0.35355339059327373, O(4, -2), 0.9354143466934853);
  out[oi++] = LIN3(O(4, 0), 0.739509972887452, O(4, 2), -0.6614378277661477, O(4, 4), 0.125);
#undef O
#undef NEG
#undef LIN2
#undef LIN3
}

// RotateXMinus (:273-289): RotateXPlus, then `.scale` in place
DR_SH_FN void sh_rotate_x_minus(float* const* in, float** out, int lmax, ShRotPool& P) {
  sh_rotate_x_plus(in, out, lmax, P);
  for (int l = 1; l <= lmax; ++l) {
    double s = (l & 0x1) != 0 ? -1.0 : 1.0;
    *out[sh_index(l, 0)] = sh_mulD(*out[sh_index(l, 0)], s);
    for (int m = 1; m <= l; ++m) {
      s = -s;
      *out[sh_index(l, m)] = sh_mulD(*out[sh_index(l, m)], s);
      *out[sh_index(l, -m)] = sh_mulD(*out[sh_index(l, -m)], -s);
    }
  }
}

// Rotate (:228-242) of ONE channel: c_in[k * stride], k < Terms(lmax), into c_out[k * stride] -- the caller's c_l, every entry Spectrum(0) before
// the call (glossy_prt_integrator.dart:91-95), which this sets up itself.
DR_SH_FN void sh_rotate_channel(const float* c_in, int stride, double alpha, double beta, double gamma, int lmax, float* c_out) {
  const int terms = sh_terms(lmax);
  ShRotPool P;
  P.n = 0;
  float cin[DR_GPRT_MAX_TERMS];
  float *in[DR_GPRT_MAX_TERMS], *out[DR_GPRT_MAX_TERMS], *work[DR_GPRT_MAX_TERMS];
  for (int k = 0; k < terms; ++k) {
    cin[k] = c_in[k * stride];
    in[k] = &cin[k];
    out[k] = sh_rot_new(P, 0.f);
  }
  for (int k = 0; k < terms; ++k) work[k] = sh_rot_new(P, 0.f);  // Spectrum.AllocateList
  sh_rotate_z(in, out, gamma, lmax, P);
  sh_rotate_x_plus(out, work, lmax, P);
  sh_rotate_z(work, out, beta, lmax, P);
  sh_rotate_x_minus(out, work, lmax, P);
  sh_rotate_z(work, out, alpha, lmax, P);
  for (int k = 0; k < terms; ++k) c_out[k * stride] = *out[k];
}

// ---- ComputeBSDFMatrix (:609-672) ----
// VanDerCorput / Sobol2 under a scramble word (montecarlo.dart:486-504), Sample02 (:507-511), UniformSampleSphere (:113-120) into a Vector (three f32).
// SECOND COPIES, for the host build: scrambled_radical / Sample02 / UniformSampleSphere of dr_li_sampling.h and fresnel_dielectric of dr_device.h
// are device-only (DR_DEV, inside the layout namespace, in headers the path kernels' profiles pin).  k_shade_gprt and k_gprt_finish use
// those; k_gprt_dirs, k_gprt_pairs and dr_sh_bsdf_matrix_host use these.  A change to either copy goes into both; tests/test_gpu_glossy_prt.py
// holds them together (the films restate w_i with the restatement's own functions; the device B equals the host B bit for bit).
DR_SH_FN double sh_radical(uint32_t n, uint32_t scramble, bool sobol) {
  if (!sobol) return (double)((float)((__builtin_bitreverse32(n) ^ scramble) >> 8) * 5.9604644775390625e-8f);
  for (uint32_t v = 1u << 31; n != 0; n >>= 1, v ^= v >> 1)
    if (n & 1u) scramble ^= v;
  return (double)((float)(scramble >> 8) * 5.9604644775390625e-8f);
}
DR_SH_FN void sh_sample_sphere(uint32_t i, const uint32_t scramble[2], float w[3]) {
  const double u1 = sh_radical(i, scramble[0], false), u2 = sh_radical(i, scramble[1], true);
  const double z = 1.0 - 2.0 * u1;
  const double r = sqrt(fmax(0.0, 1.0 - z * z));
  const double phi = 2.0 * DR_SH_PI * u2;
  w[0] = (float)(r * cos(phi));
  w[1] = (float)(r * sin(phi));
  w[2] = (float)z;
}
// FresnelDielectric(1.5, 1.0).evaluate (fresnel_dielectric.dart:30-64): three equal f32 channels
DR_SH_FN float sh_fresnel_dielectric(double cosi, double eta_i, double eta_t) {
  cosi = cosi < -1.0 ? -1.0 : (cosi > 1.0 ? 1.0 : cosi);
  const bool entering = cosi > 0.0;
  const double ei = entering ? eta_i : eta_t, et = entering ? eta_t : eta_i;
  const double sint = ei / et * sqrt(fmax(0.0, 1.0 - cosi * cosi));
  if (sint >= 1.0) return 1.0f;
  const double cost = sqrt(fmax(0.0, 1.0 - sint * sint));
  cosi = fabs(cosi);
  const double Rparl = ((et * cosi) - (ei * cost)) / ((et * cosi) + (ei * cost));
  const double Rperp = ((ei * cosi) - (et * cost)) / ((ei * cosi) + (et * cost));
  return (float)((Rparl * Rparl + Rperp * Rperp) / 2.0);
}
DR_SH_FN double sh_blinn_exponent(double roughness) {  // Blinn(1.0 / roughness) (blinn.dart:24-28)
  double e = 1.0 / roughness;
  if (e > 10000.0 || e != e) e = 10000.0;
  return e;
}
// One (osamp, isamp) pair: f = bsdf.f(wo, wi) of Lambertian(Kd) + Microfacet(Ks, FresnelDielectric(1.5, 1.0), Blinn(bexp)) on the identity frame
// with ng = (0, 0, 1) (bsdf.dart:187-211, lambertian.dart:35-37, microfacet.dart:27-56, blinn.dart:30-33), then `f *= |CosTheta(wi)| / pdf_nSamples`.
// A black f -- the pair the reference skips -- is +0, which leaves every sum as it is.
DR_SH_FN void sh_bsdf_pair(const float* Kd, const float* Ks, double bexp, const float* wo, const float* wi, double pdf_nSamples, float* f) {
  f[0] = f[1] = f[2] = 0.f;
  // Dot(wiW, ng) * Dot(woW, ng) > 0: the BRDFs; else only BTDFs, and the BSDF has none
  const double di = (double)wi[0] * 0.0 + (double)wi[1] * 0.0 + (double)wi[2] * 1.0, dout = (double)wo[0] * 0.0 + (double)wo[1] * 0.0 + (double)wo[2] * 1.0;
  if (!(di * dout > 0)) return;
  for (int c = 0; c < 3; ++c) f[c] = sh_add(f[c], sh_mulD(Kd[c], DR_SH_INV_PI));
  float mf[3] = {0.f, 0.f, 0.f};
  const double cosThetaO = fabs((double)wo[2]), cosThetaI = fabs((double)wi[2]);
  float wh[3] = {(float)((double)wi[0] + (double)wo[0]), (float)((double)wi[1] + (double)wo[1]), (float)((double)wi[2] + (double)wo[2])};
  if (!(cosThetaI == 0.0 || cosThetaO == 0.0) && !(wh[0] == 0.0f && wh[1] == 0.0f && wh[2] == 0.0f)) {
    const double len = sqrt((double)wh[0] * (double)wh[0] + (double)wh[1] * (double)wh[1] + (double)wh[2] * (double)wh[2]);
    for (int c = 0; c < 3; ++c) wh[c] = (float)((double)wh[c] / len);
    const double cosThetaH = (double)wi[0] * (double)wh[0] + (double)wi[1] * (double)wh[1] + (double)wi[2] * (double)wh[2];
    const float F = sh_fresnel_dielectric(cosThetaH, 1.5, 1.0);
    const double d = (bexp + 2.0) * DR_SH_INV_TWOPI * pow(fabs((double)wh[2]), bexp);
    const double NdotWh = fabs((double)wh[2]);
    const double WOdotWh = fabs((double)wo[0] * (double)wh[0] + (double)wo[1] * (double)wh[1] + (double)wo[2] * (double)wh[2]);
    const double g = fmin(1.0, fmin((2.0 * NdotWh * cosThetaO / WOdotWh), (2.0 * NdotWh * cosThetaI / WOdotWh)));
    for (int c = 0; c < 3; ++c) mf[c] = (float)((double)(float)((double)sh_mulD(Ks[c], d * g) * (double)F) / (4.0 * cosThetaI * cosThetaO));
  }
  for (int c = 0; c < 3; ++c) f[c] = sh_add(f[c], mf[c]);
  if (!(f[0] != 0.0f || f[1] != 0.0f || f[2] != 0.0f)) {  // isBlack
    f[0] = f[1] = f[2] = 0.f;
    return;
  }
  const double k = fabs((double)wi[2]) / pdf_nSamples;
  for (int c = 0; c < 3; ++c) f[c] = sh_mulD(f[c], k);
}
DR_SH_FN double sh_bsdf_pdf_nsamples(int nSamples) {
  const double pdf = (1.0 / (4.0 * DR_SH_PI)) * (1.0 / (4.0 * DR_SH_PI));  // UniformSpherePdf() * UniformSpherePdf() (montecarlo.dart:122-124)
  return pdf * nSamples * nSamples;
}
// B[i][j] += f * (Ylm[isamp][j] * Ylm[osamp][i]): one element's step (Ylm: the Float32List)
DR_SH_FN float sh_bsdf_step(float B, float f, float Yij, float Yoi) { return sh_add(B, sh_mulD(f, (double)Yij * (double)Yoi)); }

#endif
