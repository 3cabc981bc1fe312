// dr_image.h -- what the image-space stages beside the render path share on the host and on the device ("what an image
// stage is made of"): the 16-byte texel and the two pack rules, the finite test, the squared distance and the luminance their per-pixel
// rules use, the byte-range overlap, the two refusals of an image's size and the refusal itself.  The stages are the a-trous denoiser
// (dr_denoise.h), its pair form (dr_denoise_pair.h), the display transform (dr_display.h), the upsampler (dr_upsample.h) and temporal
// accumulation (dr_temporal.h).  Everything here is inline, so a unit that includes it needs no other translation unit but dr_fail's.
//
// Arithmetic: + - * / in f32, one operation and one rounding per operator; the units that include this header are compiled with
// -ffp-contract=off and without fast-math, and `/` is the correctly rounded division.
#ifndef DR_IMAGE_H
#define DR_IMAGE_H

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/dartray_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DR_DN_HD __host__ __device__ inline
#else
#define DR_DN_HD inline
#endif

int dr_fail(int code, const std::string& msg);  // dr_api.hip: sets dr_last_error()

struct alignas(16) DnTexel {
  float x, y, z, w;
};

DR_DN_HD bool dn_finite(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, sizeof(u));
  return (u & 0x7f800000u) != 0x7f800000u;
}

// (a - b)^2 summed over three components, left to right
DR_DN_HD float dn_dist2(const DnTexel& a, const DnTexel& b) {
  const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

DR_DN_HD float img_lum(float r, float g, float b) { return (0.212671f * r + 0.715160f * g) + 0.072169f * b; }

// colour = (r, g, b, valid): valid is 1 where the pixel's three colour values, its three normal values and its depth are all finite
DR_DN_HD DnTexel dn_pack_colour(const float* rgb, const float* normal, const float* depth, size_t p) {
  const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
  const bool valid = dn_finite(r) && dn_finite(g) && dn_finite(b) && dn_finite(normal[3 * p]) && dn_finite(normal[3 * p + 1]) &&
                     dn_finite(normal[3 * p + 2]) && dn_finite(depth[p]);
  return DnTexel{r, g, b, valid ? 1.0f : 0.0f};
}
// guide = (nx, ny, nz, z)
DR_DN_HD DnTexel dn_pack_guide(const float* normal, const float* depth, size_t p) {
  return DnTexel{normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], depth[p]};
}

// The three images a colour plane and a guide plane are packed from (the a-trous filter's and the upsampler's low-resolution ones); the
// pair filter has its own (DnpInputs)
struct DnInputs {
  const float *rgb, *normal, *depth;
  DR_DN_HD DnTexel colour(size_t p) const { return dn_pack_colour(rgb, normal, depth, p); }
  DR_DN_HD DnTexel guide(size_t p) const { return dn_pack_guide(normal, depth, p); }
};

// [a, a + na) and [b, b + nb) share a byte
inline bool dn_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// What every stage refuses in a w x h image: NULL, or the refusal's text
inline const char* img_check_dims(int32_t w, int32_t h) {
  if (w < 1 || h < 1) return "w and h must be at least 1";
  if ((int64_t)w * (int64_t)h >= ((int64_t)1 << 31)) return "the image has 2^31 or more pixels";
  return nullptr;
}

// A *_check's answer as an entry point's: DR_OK, or the refusal "who: why"
inline int img_refuse(const char* who, const char* why) { return why ? dr_fail(DR_ERR_INVALID, std::string(who) + ": " + why) : DR_OK; }

#endif
