// dr_denoise_pair.h -- the variance-guided a-trous filter over two half-sample renders (SVGF's variance-scaled luminance
// term, Schied et al. 2017, on the dual-buffer variance estimate of Rousselle et al. 2012, with the rational weights of 2.15): the pack
// rule, the 3 x 3 variance prefilter, one pixel's share of a level and the parameter check, written once for the host loop
// (dr_denoise_pair_host.cpp) and the device kernels (dr_denoise_device.hip).
//
// A level reads two planes of 16-byte texels, colour = (r, g, b, v) and guide = (nx, ny, nz, z).  v is the variance of the pixel's
// luminance, >= 0, where the pixel is valid, and -1 where it is not: the sign is the validity flag, so a tap stays two 16-byte loads of
// which the first decides whether the second is made (dr_denoise.h).
//
// Arithmetic: dr_denoise.h's -- + - * / in f32, one operation and one rounding per operator, in the order DESIGN.md 2.19 writes them.
#ifndef DR_DENOISE_PAIR_H
#define DR_DENOISE_PAIR_H

#include "dr_denoise.h"

// g[a] * g[b] of g = [1/4, 1/2, 1/4], row dy + 1, column dx + 1: multiples of 1/16, exact in f32
DR_DN_HD float dnp_gauss(int row, int col) {
  static constexpr float G[3][3] = {{1 / 16.f, 2 / 16.f, 1 / 16.f}, {2 / 16.f, 4 / 16.f, 2 / 16.f}, {1 / 16.f, 2 / 16.f, 1 / 16.f}};
  return G[row][col];
}

// 0.5 * (a + b); a NaN comes out as the one quiet NaN 0x7fc00000 (which NaN an operation returns differs between processors, and an
// invalid pixel's mean is an output)
DR_DN_HD float dnp_mean(float a, float b) {
  const float m = 0.5f * (a + b);
  uint32_t u;
  __builtin_memcpy(&u, &m, sizeof(u));
  if ((u & 0x7fffffffu) > 0x7f800000u) {
    u = 0x7fc00000u;
    float q;
    __builtin_memcpy(&q, &u, sizeof(q));
    return q;
  }
  return m;
}

DR_DN_HD DnTexel dnp_pack_colour(const float* a, const float* b, const float* normal, const float* depth, size_t p) {
  const float mr = dnp_mean(a[3 * p], b[3 * p]), mg = dnp_mean(a[3 * p + 1], b[3 * p + 1]), mb = dnp_mean(a[3 * p + 2], b[3 * p + 2]);
  const float ld = img_lum(a[3 * p] - b[3 * p], a[3 * p + 1] - b[3 * p + 1], a[3 * p + 2] - b[3 * p + 2]);
  const float v0 = 0.25f * (ld * ld);
  const bool valid = dn_finite(mr) && dn_finite(mg) && dn_finite(mb) && dn_finite(v0) && dn_finite(normal[3 * p]) &&
                     dn_finite(normal[3 * p + 1]) && dn_finite(normal[3 * p + 2]) && dn_finite(depth[p]);
  return DnTexel{mr, mg, mb, valid ? v0 : -1.0f};
}

// The four images the planes are packed from
struct DnpInputs {
  const float *a, *b, *normal, *depth;
  DR_DN_HD DnTexel colour(size_t p) const { return dnp_pack_colour(a, b, normal, depth, p); }
  DR_DN_HD DnTexel guide(size_t p) const { return dn_pack_guide(normal, depth, p); }
};

// One pixel of one level: step s, sharpness kc (the same at every level), kn, kz, and the variance floor.  Every tap's coordinates,
// the prefilter's too, are checked against the image before its loads (64-bit, as in dn_pixel).
DR_DN_HD DnTexel dnp_pixel(const DnTexel* colour, const DnTexel* guide, int32_t w, int32_t h, int32_t x, int32_t y, int32_t s, float kc,
                           float kn, float kz, float var_floor) {
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const DnTexel cp = colour[p];
  if (cp.w < 0.0f) return cp;  // not valid: the input texel, bit for bit
  const DnTexel gp = guide[p];
  // the variance around p, at unit distance at every level; the centre is always taken: sumg >= 1/4
  float sumgv = 0.0f, sumg = 0.0f;
  for (int dy = -1; dy <= 1; ++dy) {
    const int64_t qy = (int64_t)y + dy;
    if (qy < 0 || qy >= h) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int64_t qx = (int64_t)x + dx;
      if (qx < 0 || qx >= w) continue;
      const float vq = colour[(size_t)qy * (size_t)w + (size_t)qx].w;
      if (vq < 0.0f) continue;
      const float g = dnp_gauss(dy + 1, dx + 1);
      sumgv = sumgv + g * vq;
      sumg = sumg + g;
    }
  }
  const float den = sumgv / sumg + var_floor;
  const bool colourTerm = kc != 0.0f && dn_finite(den);
  const float lp = img_lum(cp.x, cp.y, cp.z);
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sumv = 0.0f, sumw = 0.0f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t qy = (int64_t)y + (int64_t)dy * s;
    if (qy < 0 || qy >= h) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t qx = (int64_t)x + (int64_t)dx * s;
      if (qx < 0 || qx >= w) continue;
      const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
      const DnTexel cq = colour[q];
      if (cq.w < 0.0f) continue;
      const DnTexel gq = guide[q];
      const float dl = img_lum(cq.x, cq.y, cq.z) - lp, dc = dl * dl;
      const float dn = dn_dist2(gq, gp);
      const float dd = gq.w - gp.w, dz = dd * dd;
      float wt = dn_tap(dy + 2, dx + 2);
      if (colourTerm) wt = wt / (1.0f + kc * (dc / den));
      if (kn != 0.0f) wt = wt / (1.0f + kn * dn);
      if (kz != 0.0f) wt = wt / (1.0f + kz * dz);
      sr = sr + wt * cq.x;
      sg = sg + wt * cq.y;
      sb = sb + wt * cq.z;
      sumv = sumv + (wt * wt) * cq.w;
      sumw = sumw + wt;
    }
  }
  const float r = sr / sumw, g = sg / sumw, b = sb / sumw, v = sumv / (sumw * sumw);  // the centre tap is always taken: sumw >= 9/64
  return DnTexel{r, g, b, (dn_finite(r) && dn_finite(g) && dn_finite(b) && dn_finite(v)) ? v : -1.0f};
}

// The arguments every entry point checks the same way: NULL, or the refusal's text
inline const char* dnp_check(int32_t w, int32_t h, const DrDenoisePairParams* p) {
  if (!p) return "a null pointer";
  if (const char* why = img_check_dims(w, h)) return why;
  if (p->iterations < 1 || p->iterations > DR_DN_MAX_ITERATIONS) return "iterations must be in 1..8";
  const float k[3] = {p->k_color, p->k_normal, p->k_depth};
  for (int i = 0; i < 3; ++i)
    if (!dn_finite(k[i]) || k[i] < 0.0f) return "k_color, k_normal and k_depth must be finite and not negative";
  if (!dn_finite(p->var_floor) || !(p->var_floor > 0.0f)) return "var_floor must be finite and positive";
  return nullptr;
}

// dnp_check, the null pointers and the overlaps of `out` and `out_var` (which may be NULL) with an input and with each other, as a
// refusal (`who` prefixes the message).  dr_denoise_pair_host.cpp.
int dnp_check_images(const char* who, const void* a, const void* b, const void* normal, const void* depth, int32_t w, int32_t h,
                     const DrDenoisePairParams* params, const void* out, const void* out_var);

// The pair form's DnRule (dr_denoise.h): kc is the same at every level, the variance floor rides along, and w is the variance, an output
struct DnpRule {
  typedef DrDenoisePairParams Params;
  typedef DnpInputs Inputs;
  static constexpr bool kVariance = true;
  float kc, kn, kz, var_floor;
  static DnpRule level(const Params& p, int) { return DnpRule{p.k_color, p.k_normal, p.k_depth, p.var_floor}; }
  DR_DN_HD DnTexel pixel(const DnTexel* colour, const DnTexel* guide, int32_t w, int32_t h, int32_t x, int32_t y, int32_t s) const {
    return dnp_pixel(colour, guide, w, h, x, y, s, kc, kn, kz, var_floor);
  }
};

#endif
