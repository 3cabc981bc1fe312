// dr_demodulate.h -- demodulation: the two per-pixel rules, written once for the host loop (dr_demodulate_host.cpp) and the
// kernels (dr_demodulate_device.hip), and their checks.  An image stage in the sense of DESIGN.md 2.15: device, host loop and numpy
// restatement (tests/demodulate_restatement.py) write the same bytes.
//
//   demodulate:  out = max(0, rgb - e) / (a + eps)     before any other image stage
//   remodulate:  out = f * (a + eps) + e               after the last one (f: the filtered demodulated image, passed as `rgb`)
//
// per colour channel, f32 `+ - * /` and comparisons, one rounding per operator (-ffp-contract=off: `f * d + e` is a product and a sum).
// e: the emission image, 0 where the pointer is NULL; a: the albedo image, and where the pointer is NULL the divisor is 1.0f, not 1 + eps.
// A pixel with a value of rgb, e or a that is not finite passes through both with its rgb bits.
#ifndef DR_DEMODULATE_H
#define DR_DEMODULATE_H

#include "dr_image.h"

struct DemodImages {
  const float *rgb, *emission, *albedo;  // emission, albedo: may be NULL
  float* out;
};

// the pixel's three rgb values, and e / d = a + eps per channel; false: a value is not finite, and the pixel is copied
DR_DN_HD bool demod_load(const DemodImages& im, float eps, size_t p, float c[3], float e[3], float d[3]) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    c[k] = im.rgb[3 * p + k];
    e[k] = im.emission ? im.emission[3 * p + k] : 0.0f;
    const float a = im.albedo ? im.albedo[3 * p + k] : 0.0f;
    ok = ok && dn_finite(c[k]) && dn_finite(e[k]) && dn_finite(a);
    d[k] = im.albedo ? a + eps : 1.0f;
  }
  return ok;
}

DR_DN_HD void demod_pixel(const DemodImages& im, float eps, size_t p) {
  float c[3], e[3], d[3];
  const bool ok = demod_load(im, eps, p, c, e, d);
  for (int k = 0; k < 3; ++k) {
    const float s = c[k] - e[k];
    // (a wide-filter film is summed by f32 atomics in no fixed order: at a pure-emitter pixel rgb - e can be a rounding below zero)
    im.out[3 * p + k] = ok ? (s > 0.0f ? s : 0.0f) / d[k] : c[k];
  }
}

DR_DN_HD void remod_pixel(const DemodImages& im, float eps, size_t p) {
  float c[3], e[3], d[3];
  const bool ok = demod_load(im, eps, p, c, e, d);
  for (int k = 0; k < 3; ++k) im.out[3 * p + k] = ok ? c[k] * d[k] + e[k] : c[k];
}

// What dr_demodulate_check refuses: NULL, or the refusal's text
inline const char* demod_check(int32_t w, int32_t h, const DrDemodulateParams* prm) {
  if (!prm) return "a null pointer";
  if (const char* why = img_check_dims(w, h)) return why;
  if (!dn_finite(prm->eps) || !(prm->eps > 0.0f)) return "eps must be finite and positive";
  return nullptr;
}
// ... and what an entry point adds: the null pointers (emission and albedo may be NULL) and the overlaps.  dr_demodulate_host.cpp
int demod_check_images(const char* who, const DemodImages& im, int32_t w, int32_t h, const DrDemodulateParams* params);

#endif
