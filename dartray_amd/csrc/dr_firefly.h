// dr_firefly.h -- firefly suppression (the reference has no such stage): a guide-aware outlier clamp ahead of the filters
// and of the temporal history.  One pixel's rule and the parameter check, written once for the host loop (dr_firefly_host.cpp) and the
// device kernel (dr_firefly_device.hip).
//
// A pixel is compared with the members of its (2 radius + 1)^2 window: the valid pixels that show the same surface by tp_history's test of
// depth and encoded normal.  Where its luminance exceeds threshold * m + floor, m the rank-th largest member luminance, its colour is
// scaled down to that limit; every other pixel is copied bit for bit.
//
// The rule is written over a TAP SOURCE, a type with
//     bool tap(int64_t x, int64_t y, FireTap* t) const
// that is false where (x, y) lies outside the image or the pixel there is not valid, and else fills t with the pixel's guide and luminance.
// The host's source reads the three images (FireImageSource below); the device's reads the workgroup's LDS tile, in which a texel outside
// the image was staged as invalid (dr_firefly_device.hip).  Both compute a texel with fire_texel, so the bytes are the same.
//
// Arithmetic: f32 + - * / and comparisons, one operation and one rounding per operator, in the order DESIGN.md 2.25 writes them; the
// units that include this header are compiled with -ffp-contract=off and without fast-math, and `/` is the correctly rounded division.
#ifndef DR_FIREFLY_H
#define DR_FIREFLY_H

#include "dr_image.h"

#define DR_FIRE_MAX_RADIUS 2
#define DR_FIRE_MAX_RANK 4

// The images of one call; removed may be NULL
struct FireImages {
  const float *rgb, *normal, *depth;
  float *out, *removed;
};

// What a tap is judged by: the guide (nx, ny, nz, z) and the luminance
struct FireTap {
  DnTexel guide;
  float lum;
};

// Step 1 for pixel p of the three images: false where it is not valid.  t is written either way; an invalid texel's lum is a NaN, which
// is how the device's tile marks it.
DR_DN_HD bool fire_texel(const float* rgb, const float* normal, const float* depth, size_t p, FireTap* t) {
  const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
  t->guide = dn_pack_guide(normal, depth, p);
  const float l = img_lum(r, g, b);
  const bool valid = dn_finite(r) && dn_finite(g) && dn_finite(b) && dn_finite(t->guide.x) && dn_finite(t->guide.y) && dn_finite(t->guide.z) &&
                     dn_finite(t->guide.w) && dn_finite(l);
  t->lum = valid ? l : __builtin_nanf("");
  return valid;
}

// The host's tap source, and the one a check of the device's is made against: the three images, every coordinate tested before its loads
struct FireImageSource {
  const float *rgb, *normal, *depth;
  int32_t w, h;
  DR_DN_HD bool tap(int64_t x, int64_t y, FireTap* t) const {
    if (x < 0 || x >= w || y < 0 || y >= h) return false;
    return fire_texel(rgb, normal, depth, (size_t)y * (size_t)w + (size_t)x, t);
  }
};

// v goes into the descending list (t0, t1, t2, t3) of the largest values seen: four registers and comparisons, no indexed array
DR_DN_HD void fire_insert(float v, float& t0, float& t1, float& t2, float& t3) {
  float hi = v > t0 ? v : t0;
  v = v > t0 ? t0 : v;
  t0 = hi;
  hi = v > t1 ? v : t1;
  v = v > t1 ? t1 : v;
  t1 = hi;
  hi = v > t2 ? v : t2;
  v = v > t2 ? t2 : v;
  t2 = hi;
  t3 = v > t3 ? v : t3;
}

// One pixel (x, y) of a w x h image: its out and, where given, its removed.  `radius` is prm.radius, a template argument so that the
// window unrolls.
template <int radius, class Source>
DR_DN_HD void fire_pixel(const Source& src, const FireImages& im, int32_t w, const DrFireflyParams& prm, int32_t x, int32_t y) {
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const float r = im.rgb[3 * p], g = im.rgb[3 * p + 1], b = im.rgb[3 * p + 2];
  float o0 = r, o1 = g, o2 = b, gone = 0.0f;
  FireTap c;
  if (src.tap(x, y, &c)) {
    const float band = prm.depth_tol * c.guide.w;
    const float none = -__builtin_inff();  // below every member's finite luminance
    float t0 = none, t1 = none, t2 = none, t3 = none;
    int32_t n = 0;
#pragma unroll
    for (int dy = -radius; dy <= radius; ++dy) {
#pragma unroll
      for (int dx = -radius; dx <= radius; ++dx) {
        if (dx == 0 && dy == 0) continue;
        FireTap q;
        if (!src.tap((int64_t)x + dx, (int64_t)y + dy, &q)) continue;
        if (!(__builtin_fabsf(q.guide.w - c.guide.w) <= band)) continue;  // a NaN fails
        if (!(dn_dist2(q.guide, c.guide) <= prm.normal_tol)) continue;
        ++n;
        fire_insert(q.lum, t0, t1, t2, t3);
      }
    }
    if (n >= prm.rank) {
      const float m = prm.rank == 1 ? t0 : prm.rank == 2 ? t1 : prm.rank == 3 ? t2 : t3;
      const float lim = prm.threshold * m + prm.floor;
      const float lim0 = lim > 0.0f ? lim : 0.0f;  // one zero, whatever the sign of a zero m
      if (c.lum > lim0) {
        const float s = lim0 / c.lum;
        o0 = r * s;
        o1 = g * s;
        o2 = b * s;
        gone = c.lum - lim0;
      }
    }
  }
  im.out[3 * p] = o0;
  im.out[3 * p + 1] = o1;
  im.out[3 * p + 2] = o2;
  if (im.removed) im.removed[p] = gone;
}

// The arguments every entry point checks the same way: NULL, or the refusal's text
inline const char* fire_check(int32_t w, int32_t h, const DrFireflyParams* p) {
  if (!p) return "a null pointer";
  if (const char* why = img_check_dims(w, h)) return why;
  if (p->radius < 1 || p->radius > DR_FIRE_MAX_RADIUS) return "radius must be 1 or 2";
  if (p->rank < 1 || p->rank > DR_FIRE_MAX_RANK) return "rank must be in 1..4";
  if (!dn_finite(p->threshold) || !(p->threshold >= 0.0f)) return "threshold must be finite and not negative";
  if (!dn_finite(p->floor) || p->floor < 0.0f) return "floor must be finite and not negative";
  if (!dn_finite(p->depth_tol) || p->depth_tol < 0.0f || !dn_finite(p->normal_tol) || p->normal_tol < 0.0f)
    return "depth_tol and normal_tol must be finite and not negative";
  return nullptr;
}

// fire_check, the null pointers (removed excepted) and the overlap of out or removed with an input or with each other -- the taps read
// the original image, so the stage cannot run in place -- as a refusal (`who` prefixes the message).  dr_firefly_host.cpp.
int fire_check_images(const char* who, const FireImages& im, int32_t w, int32_t h, const DrFireflyParams* params);

#endif
