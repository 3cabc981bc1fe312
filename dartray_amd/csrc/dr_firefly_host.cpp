// dr_firefly_host.cpp -- firefly suppression on the host: dr_firefly_host, a serial loop over the per-pixel rule of
// dr_firefly.h with the three images as its tap source -- the rule the kernel of dr_firefly_device.hip runs over its LDS tile, so the two
// write the same bytes -- and dr_firefly_check.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here needs
// the HIP runtime, so the file also builds as plain C++.
#include "dr_firefly.h"

int fire_check_images(const char* who, const FireImages& im, int32_t w, int32_t h, const DrFireflyParams* params) {
  if (!im.rgb || !im.normal || !im.depth || !im.out || !params) return img_refuse(who, "a null pointer");
  if (const char* why = fire_check(w, h, params)) return img_refuse(who, why);
  const size_t n = (size_t)w * (size_t)h * sizeof(float);
  const void* out[2] = {im.out, im.removed};
  const size_t out_bytes[2] = {3 * n, n};
  const void* in[3] = {im.rgb, im.normal, im.depth};
  const size_t in_bytes[3] = {3 * n, 3 * n, n};
  for (int o = 0; o < 2; ++o) {
    if (!out[o]) continue;
    for (int i = 0; i < 3; ++i)
      if (dn_overlap(out[o], out_bytes[o], in[i], in_bytes[i])) return img_refuse(who, "an output overlaps an input");
  }
  if (im.removed && dn_overlap(im.out, 3 * n, im.removed, n)) return img_refuse(who, "an output overlaps another output");
  return DR_OK;
}

extern "C" int dr_firefly_check(const DrFireflyParams* params, int32_t w, int32_t h) { return img_refuse("dr_firefly_check", fire_check(w, h, params)); }

extern "C" int dr_firefly_host(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h, const DrFireflyParams* params,
                               float* out, float* removed) {
  const FireImages im = {rgb, normal, depth, out, removed};
  const int rc = fire_check_images("dr_firefly_host", im, w, h, params);
  if (rc != DR_OK) return rc;
  const FireImageSource src = {rgb, normal, depth, w, h};
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      if (params->radius == 1) fire_pixel<1>(src, im, w, *params, x, y);
      else fire_pixel<2>(src, im, w, *params, x, y);
    }
  return DR_OK;
}
