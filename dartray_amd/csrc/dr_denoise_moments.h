// dr_denoise_moments.h -- the variance-guided a-trous filter fed by the temporal history's luminance moments (the
// variance estimate of SVGF's section 4.2, Schied et al. 2017, in front of the levels of 2.19): the pack rule, one pixel's variance
// estimate and the parameter check, written once for the host loop (dr_denoise_moments_host.cpp) and the device kernels
// (dr_denoise_device.hip).  The levels are dr_denoise_pair.h's dnp_pixel and nothing else.
//
// The pack gives colour = (r, g, b, len) and guide = (nx, ny, nz, z); len is the history length, > 0, where the pixel is valid, and -1
// where it is not.  The estimate reads those two planes and the pixel's own m2 and writes the plane the first level reads,
// colour = (r, g, b, v) with v the variance of the accumulated luminance, >= 0, or -1: the texel of dr_denoise_pair.h.
//
// Arithmetic: dr_denoise.h's -- + - * / in f32, one operation and one rounding per operator, in the order DESIGN.md 2.24 writes them.
#ifndef DR_DENOISE_MOMENTS_H
#define DR_DENOISE_MOMENTS_H

#include "dr_denoise_pair.h"

#define DR_DNM_MAX_RADIUS 3
#define DR_DNM_MAX_HISTORY 4096

DR_DN_HD DnTexel dnm_pack_colour(const float* rgb, const float* m2, const float* len, const float* normal, const float* depth, size_t p) {
  const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2], n = len[p];
  const bool valid = dn_finite(r) && dn_finite(g) && dn_finite(b) && dn_finite(m2[p]) && dn_finite(n) && dn_finite(normal[3 * p]) &&
                     dn_finite(normal[3 * p + 1]) && dn_finite(normal[3 * p + 2]) && dn_finite(depth[p]) && n > 0.0f;
  return DnTexel{r, g, b, valid ? n : -1.0f};
}

// The five images of a temporal history that the planes are packed from; m2 is read once more by the estimate
struct DnmInputs {
  const float *rgb, *m2, *len, *normal, *depth;
  DR_DN_HD DnTexel colour(size_t p) const { return dnm_pack_colour(rgb, m2, len, normal, depth, p); }
  DR_DN_HD DnTexel guide(size_t p) const { return dn_pack_guide(normal, depth, p); }
};

// One pixel's variance estimate: `colour` is the pack's plane, (r, g, b, len or -1).  A history of min_history frames or more gives the
// temporal estimate from the pixel's own moments; a shorter one the spatial estimate over the valid pixels of the (2 radius + 1)^2
// window, weighted by the guides.  Every tap's coordinates are checked against the image before its loads (64-bit, as in dnp_pixel).
DR_DN_HD DnTexel dnm_variance(const DnTexel* colour, const DnTexel* guide, const float* m2, int32_t w, int32_t h, int32_t x, int32_t y,
                              int32_t min_history, int32_t radius, float kn, float kz) {
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const DnTexel cp = colour[p];
  if (cp.w < 0.0f) return cp;  // not valid: the input texel, bit for bit
  const float lp = img_lum(cp.x, cp.y, cp.z);
  float v;
  if (cp.w >= (float)min_history) {
    const float d = m2[p] - lp * lp;
    v = (d < 0.0f ? 0.0f : d) / (cp.w - 1.0f);  // min_history >= 2: the divisor is >= 1
  } else {
    const DnTexel gp = guide[p];
    float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
    for (int dy = -radius; dy <= radius; ++dy) {
      const int64_t qy = (int64_t)y + dy;
      if (qy < 0 || qy >= h) continue;
      for (int dx = -radius; dx <= radius; ++dx) {
        const int64_t qx = (int64_t)x + dx;
        if (qx < 0 || qx >= w) continue;
        const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
        const DnTexel cq = colour[q];
        if (cq.w < 0.0f) continue;
        const DnTexel gq = guide[q];
        const float lq = img_lum(cq.x, cq.y, cq.z);
        const float dn = dn_dist2(gq, gp);
        const float dd = gq.w - gp.w, dz = dd * dd;
        float wt = 1.0f;
        if (kn != 0.0f) wt = wt / (1.0f + kn * dn);
        if (kz != 0.0f) wt = wt / (1.0f + kz * dz);
        s1 = s1 + wt * lq;
        s2 = s2 + wt * (lq * lq);
        sw = sw + wt;
      }
    }
    const float mean = s1 / sw;  // the centre is always a tap, with weight 1: sw >= 1
    const float e = s2 / sw - mean * mean;
    v = e < 0.0f ? 0.0f : e;
  }
  return DnTexel{cp.x, cp.y, cp.z, dn_finite(v) ? v : -1.0f};
}

// The arguments every entry point checks the same way: NULL, or the refusal's text
inline const char* dnm_check(int32_t w, int32_t h, const DrDenoiseMomentsParams* p) {
  if (!p) return "a null pointer";
  if (const char* why = img_check_dims(w, h)) return why;
  if (p->iterations < 1 || p->iterations > DR_DN_MAX_ITERATIONS) return "iterations must be in 1..8";
  const float k[3] = {p->k_color, p->k_normal, p->k_depth};
  for (int i = 0; i < 3; ++i)
    if (!dn_finite(k[i]) || k[i] < 0.0f) return "k_color, k_normal and k_depth must be finite and not negative";
  if (!dn_finite(p->var_floor) || !(p->var_floor > 0.0f)) return "var_floor must be finite and positive";
  if (p->min_history < 2 || p->min_history > DR_DNM_MAX_HISTORY) return "min_history must be in 2..4096";
  if (p->radius < 0 || p->radius > DR_DNM_MAX_RADIUS) return "radius must be in 0..3";
  return nullptr;
}

// The images of one call: five inputs, `out`, and the two optional outputs
struct DnmImages {
  const void *rgb, *m2, *len, *normal, *depth;
  void *out, *out_var, *out_var0;
};

// dnm_check, the null pointers and the overlaps of the outputs with an input and with each other, as a refusal (`who` prefixes the
// message).  dr_denoise_moments_host.cpp.
int dnm_check_images(const char* who, const DnmImages& im, int32_t w, int32_t h, const DrDenoiseMomentsParams* params);

// The moments form's level rule: dnp_pixel with the scalars of its own parameter struct
struct DnmRule {
  typedef DrDenoiseMomentsParams Params;
  typedef DnmInputs Inputs;
  static constexpr bool kVariance = true;
  float kc, kn, kz, var_floor;
  static DnmRule level(const Params& p, int) { return DnmRule{p.k_color, p.k_normal, p.k_depth, p.var_floor}; }
  DR_DN_HD DnTexel pixel(const DnTexel* colour, const DnTexel* guide, int32_t w, int32_t h, int32_t x, int32_t y, int32_t s) const {
    return dnp_pixel(colour, guide, w, h, x, y, s, kc, kn, kz, var_floor);
  }
};

#endif
