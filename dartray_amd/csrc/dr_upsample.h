// dr_upsample.h -- the joint bilateral upsampler (Kopf et al. 2007 with the rational edge-stopping weights of dr_denoise.h; DESIGN.md 2.22;
// the reference has no such stage): the packed low-resolution planes, one full-resolution pixel's rule and the parameter check, written
// once for the host loop (dr_upsample_host.cpp) and the device kernels (dr_upsample_device.hip).
//
// A call reads two low-resolution planes of 16-byte texels, colour = (r, g, b, valid) and guide = (nx, ny, nz, z) -- dn_pack_colour and
// dn_pack_guide of the three low-resolution images -- and the full-resolution guides as they stand, and gives every full-resolution pixel
// its colour.  `valid` is 1 where the low-resolution pixel's three colour values, its three normal values and its depth are all finite.
//
// Arithmetic: + - * / in f32, one operation and one rounding per operator, in the order DESIGN.md 2.22 writes them; the units that
// include this header are compiled with -ffp-contract=off and without fast-math, and `/` is the correctly rounded division.
#ifndef DR_UPSAMPLE_H
#define DR_UPSAMPLE_H

#include "dr_image.h"

// One full-resolution pixel (x, y) of an image w = f * wl wide: its three colour values to out3.  Every tap's coordinates are checked
// against the low-resolution image before its two loads.
DR_DN_HD void ups_pixel(const DnTexel* colour, const DnTexel* guide, int32_t wl, int32_t hl, const float* normal, const float* depth, int32_t w,
                        int32_t f, int32_t taps, float kn, float kz, int32_t x, int32_t y, float* out3) {
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const DnTexel gp = DnTexel{normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], depth[p]};
  const bool edges = dn_finite(gp.x) && dn_finite(gp.y) && dn_finite(gp.z) && dn_finite(gp.w);
  const int32_t r = taps / 2;
  const float ff = (float)f, rf = (float)r;
  const float u = ((float)x + 0.5f) / ff - 0.5f, v = ((float)y + 0.5f) / ff - 0.5f;
  const int64_t bx = (int64_t)__builtin_floorf(u), by = (int64_t)__builtin_floorf(v);
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sumw = 0.0f;
  for (int64_t j = by - r + 1; j <= by + r; ++j) {
    if (j < 0 || j >= hl) continue;
    const float wy = 1.0f - __builtin_fabsf(v - (float)j) / rf;
    for (int64_t i = bx - r + 1; i <= bx + r; ++i) {
      if (i < 0 || i >= wl) continue;
      const size_t q = (size_t)j * (size_t)wl + (size_t)i;
      const DnTexel cq = colour[q];
      if (cq.w == 0.0f) continue;
      const float wx = 1.0f - __builtin_fabsf(u - (float)i) / rf;
      float wt = wx * wy;
      if (edges) {
        const DnTexel gq = guide[q];
        const float dn = dn_dist2(gq, gp);
        const float dd = gq.w - gp.w, dz = dd * dd;
        if (kn != 0.0f) wt = wt / (1.0f + kn * dn);
        if (kz != 0.0f) wt = wt / (1.0f + kz * dz);
      }
      sr = sr + wt * cq.x;
      sg = sg + wt * cq.y;
      sb = sb + wt * cq.z;
      sumw = sumw + wt;
    }
  }
  if (sumw == 0.0f) {  // no valid tap, or every weight underflowed: the nearest low-resolution pixel, bit for bit
    const DnTexel c = colour[(size_t)(y / f) * (size_t)wl + (size_t)(x / f)];
    out3[0] = c.x;
    out3[1] = c.y;
    out3[2] = c.z;
    return;
  }
  out3[0] = sr / sumw;
  out3[1] = sg / sumw;
  out3[2] = sb / sumw;
}

// The arguments every entry point checks the same way: NULL, or the refusal's text
inline const char* ups_check(int32_t wl, int32_t hl, const DrUpsampleParams* p) {
  if (!p) return "a null pointer";
  if (p->factor != 2 && p->factor != 4) return "factor must be 2 or 4";
  if (p->taps != 2 && p->taps != 4) return "taps must be 2 or 4";
  if (wl < 1 || hl < 1) return "wl and hl must be at least 1";
  // w * h = factor^2 * wl * hl, compared without forming it: wl * hl < 2^62, and 2^31 / factor^2 is exact
  if ((int64_t)wl * (int64_t)hl >= ((int64_t)1 << 31) / ((int64_t)p->factor * p->factor)) return "the image has 2^31 or more pixels";
  const float k[2] = {p->k_normal, p->k_depth};
  for (int i = 0; i < 2; ++i)
    if (!dn_finite(k[i]) || k[i] < 0.0f) return "k_normal and k_depth must be finite and not negative";
  return nullptr;
}

// ups_check, the null pointers and the overlap of `out` with an input, as a refusal (`who` prefixes the message).  dr_upsample_host.cpp.
int ups_check_images(const char* who, const void* rgb_lo, const void* normal_lo, const void* depth_lo, int32_t wl, int32_t hl,
                     const void* normal, const void* depth, const DrUpsampleParams* params, const void* out);

#endif
