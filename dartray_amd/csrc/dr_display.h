// dr_display.h -- the display transform: a linear f32 image becomes an RGBA8 one through an exposure scale (given, or the
// percentile of a luminance histogram), a tone curve (extended Reinhard on luminance, Reinhard et al. 2002; or Narkowicz's rational fit of
// the ACES curve, 2016) and an 8-bit encode (sRGB or gamma 2.2 by a search in 255 thresholds, or ImageFilm's table of the reference,
// film/image_film.dart:53-58 and :174-177).  The per-pixel rules, the histogram bin, the exposure pick and the parameter check, written once
// for the host loop (dr_display_host.cpp) and the device kernels (dr_display_device.hip).
//
// Arithmetic: dr_image.h's -- + - * / and comparisons in f32, one operation and one rounding per operator, in the order DESIGN.md 2.20
// writes them (the reference encode alone widens to f64 for one product and its floor, as the reference does).  Nothing transcendental runs
// per pixel: every pow is spent on the host, once, in the 256-word table of dsp_fill_table (dr_display_host.cpp).
#ifndef DR_DISPLAY_H
#define DR_DISPLAY_H

#include "dr_image.h"

#define DR_DISPLAY_TABLE 256  // words of an encode table

struct DspTable {  // by value into a kernel: 1 KiB of its arguments
  uint32_t w[DR_DISPLAY_TABLE];
};

DR_DN_HD float dsp_from_bits(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, sizeof(f));
  return f;
}
DR_DN_HD uint32_t dsp_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, sizeof(u));
  return u;
}

DR_DN_HD bool dsp_valid(float r, float g, float b) { return dn_finite(r) && dn_finite(g) && dn_finite(b); }

DR_DN_HD float dsp_floor0(float c) { return c < 0.0f ? 0.0f : c; }

// The histogram bin of a pixel, or DR_DISPLAY_BINS when it is not counted: it is invalid, or its luminance is zero or subnormal (the upper
// bound is a guard: the weights sum to 1 + 7e-9, so no finite pixel has an infinite luminance).  Eight bins per octave: the exponent and
// the three leading bits of the mantissa.
DR_DN_HD uint32_t dsp_bin(float r, float g, float b) {
  if (!dsp_valid(r, g, b)) return DR_DISPLAY_BINS;
  const uint32_t u = dsp_bits(img_lum(dsp_floor0(r), dsp_floor0(g), dsp_floor0(b)));
  return (u >= 0x00800000u && u < 0x7f800000u) ? (u >> 20) : DR_DISPLAY_BINS;
}

// rank of n counted pixels (n >= 1) at `permille`
DR_DN_HD uint64_t dsp_rank(uint64_t n, uint32_t permille) { return ((n - 1) * (uint64_t)permille) / 1000u; }

// key over the centre of bin b
DR_DN_HD float dsp_scale_of_bin(uint32_t b, float key) { return key / dsp_from_bits((b << 20) | (1u << 19)); }

// The scale auto-exposure picks from 2048 counts (the serial form; k_display_pick scans the same counts in parallel)
inline float dsp_pick(const uint32_t* hist, uint32_t permille, float key) {
  uint64_t n = 0;
  for (uint32_t b = 0; b < DR_DISPLAY_BINS; ++b) n += hist[b];
  if (n == 0) return 1.0f;
  const uint64_t rank = dsp_rank(n, permille);
  uint64_t run = 0;
  for (uint32_t b = 0; b < DR_DISPLAY_BINS; ++b) {
    run += hist[b];
    if (run > rank) return dsp_scale_of_bin(b, key);
  }
  return 1.0f;  // not reached: run ends at n > rank
}

// One value through an encode table.  A NaN -- which only an overflow on the way here makes, inf / inf or 0 * inf -- is taken as +inf.
DR_DN_HD uint32_t dsp_encode(const uint32_t* table, uint32_t encode, float x) {
  if (x != x) x = dsp_from_bits(0x7f800000u);
  if (encode == DR_ENCODE_REFERENCE) {
    const double v = __builtin_floor((double)x * 255.0);
    const uint32_t q = v < 0.0 ? 0u : (v > 255.0 ? 255u : (uint32_t)v);
    return table[q];
  }
  uint32_t code = 0;  // the number of thresholds T[1..255] that are <= x: eight steps, no branch
  for (uint32_t step = 128; step != 0; step >>= 1) {
    const uint32_t t = code + step;
    code = dsp_from_bits(table[t]) <= x ? t : code;
  }
  return code;
}

// One pixel: r | g << 8 | b << 16 | 255 << 24, or invalid_rgba
DR_DN_HD uint32_t dsp_pixel(const uint32_t* table, const DrDisplayParams& p, float scale, float r, float g, float b) {
  if (!dsp_valid(r, g, b)) return p.invalid_rgba;
  r = dsp_floor0(r) * scale;
  g = dsp_floor0(g) * scale;
  b = dsp_floor0(b) * scale;
  if (p.curve == DR_TONE_REINHARD) {
    const float y = img_lum(r, g, b);
    if (y == 0.0f) {
      r = g = b = 0.0f;
    } else {
      const float yd = (y * (1.0f + y * p.inv_white2)) / (1.0f + y);
      const float m = yd / y;
      r = r * m;
      g = g * m;
      b = b * m;
    }
  } else if (p.curve == DR_TONE_FILMIC) {
    r = (r * (2.51f * r + 0.03f)) / (r * (2.43f * r + 0.59f) + 0.14f);
    g = (g * (2.51f * g + 0.03f)) / (g * (2.43f * g + 0.59f) + 0.14f);
    b = (b * (2.51f * b + 0.03f)) / (b * (2.43f * b + 0.59f) + 0.14f);
  }
  return dsp_encode(table, p.encode, r) | (dsp_encode(table, p.encode, g) << 8) | (dsp_encode(table, p.encode, b) << 16) | 0xff000000u;
}

// The arguments every entry point checks the same way: NULL, or the refusal's text
inline const char* dsp_check(const DrDisplayParams* p, int32_t w, int32_t h) {
  if (!p) return "a null pointer";
  if (p->curve > DR_TONE_FILMIC) return "curve must be DR_TONE_CLAMP, DR_TONE_REINHARD or DR_TONE_FILMIC";
  if (p->encode > DR_ENCODE_REFERENCE) return "encode must be DR_ENCODE_SRGB, DR_ENCODE_GAMMA22 or DR_ENCODE_REFERENCE";
  if (p->permille > 1000u) return "permille must be in 0..1000";
  if (!dn_finite(p->exposure) || !(p->exposure > 0.0f)) return "exposure must be finite and positive";
  if (!dn_finite(p->key) || !(p->key > 0.0f)) return "key must be finite and positive";
  if (!dn_finite(p->inv_white2) || p->inv_white2 < 0.0f) return "inv_white2 must be finite and not negative";
  return img_check_dims(w, h);
}

// dr_display_host.cpp.  The table of an encode (valid for the process's life; filled once), and the checks of the entry points that take
// images, as a refusal (`who` prefixes the message): dsp_check, the null pointers, `out` (4 * w * h bytes; may be NULL where the entry
// point has none) overlapping `rgb`.
const DspTable& dsp_table(uint32_t encode);
int dsp_check_images(const char* who, const void* rgb, int32_t w, int32_t h, const DrDisplayParams* params, const void* out, bool has_out);

#endif
