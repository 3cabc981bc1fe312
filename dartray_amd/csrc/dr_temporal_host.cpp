// dr_temporal_host.cpp -- temporal accumulation with reprojection on the host: dr_temporal_host, a serial loop over the
// per-pixel rule of dr_temporal.h -- the one the kernel of dr_temporal_device.hip runs, one lane per pixel, so the two write the same bytes --
// and dr_temporal_check.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here needs the HIP runtime, so the file
// also builds as plain C++.
#include "dr_temporal.h"

int tp_check_images(const char* who, const TpImages& im, int32_t w, int32_t h, const DrTemporalParams* params) {
  if (!im.rgb || !im.normal || !im.depth || !im.out_rgb || !im.out_m2 || !im.out_len || !params) return img_refuse(who, "a null pointer");
  const int nhist = (im.h_rgb != nullptr) + (im.h_m2 != nullptr) + (im.h_len != nullptr) + (im.h_normal != nullptr) + (im.h_depth != nullptr);
  if (nhist != 0 && nhist != 5) return img_refuse(who, "the history is only partly NULL");
  if (const char* why = tp_check(w, h, params)) return img_refuse(who, why);
  const size_t n = (size_t)w * (size_t)h * sizeof(float);
  const void* out[3] = {im.out_rgb, im.out_m2, im.out_len};
  const size_t out_bytes[3] = {3 * n, n, n};
  const void* in[8] = {im.rgb, im.normal, im.depth, im.h_rgb, im.h_m2, im.h_len, im.h_normal, im.h_depth};
  const size_t in_bytes[8] = {3 * n, 3 * n, n, 3 * n, n, n, 3 * n, n};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 8; ++i)
      if (in[i] && dn_overlap(out[o], out_bytes[o], in[i], in_bytes[i])) return img_refuse(who, "an output overlaps an input");
    for (int o2 = 0; o2 < o; ++o2)
      if (dn_overlap(out[o], out_bytes[o], out[o2], out_bytes[o2])) return img_refuse(who, "an output overlaps another output");
  }
  return DR_OK;
}

extern "C" int dr_temporal_check(const DrTemporalParams* params, int32_t w, int32_t h) { return img_refuse("dr_temporal_check", tp_check(w, h, params)); }

extern "C" int dr_temporal_host(const float* rgb, const float* normal, const float* depth, const float* h_rgb, const float* h_m2, const float* h_len,
                                const float* h_normal, const float* h_depth, int32_t w, int32_t h, const DrTemporalParams* params, float* out_rgb,
                                float* out_m2, float* out_len) {
  const TpImages im = {rgb, normal, depth, h_rgb, h_m2, h_len, h_normal, h_depth, out_rgb, out_m2, out_len};
  const int rc = tp_check_images("dr_temporal_host", im, w, h, params);
  if (rc != DR_OK) return rc;
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) tp_pixel(im, w, h, *params, x, y);
  return DR_OK;
}
