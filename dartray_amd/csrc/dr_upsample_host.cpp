// dr_upsample_host.cpp -- the joint bilateral upsampler on the host: dr_upsample_host, a serial loop over the per-pixel
// rule of dr_upsample.h -- the one the kernel of dr_upsample_device.hip runs, one lane per pixel, so the two write the same bytes -- and
// dr_upsample_check.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here needs the HIP runtime, so the file
// also builds as plain C++.
#include <vector>

#include "dr_upsample.h"

int ups_check_images(const char* who, const void* rgb_lo, const void* normal_lo, const void* depth_lo, int32_t wl, int32_t hl,
                     const void* normal, const void* depth, const DrUpsampleParams* params, const void* out) {
  if (!rgb_lo || !normal_lo || !depth_lo || !normal || !depth || !out || !params) return img_refuse(who, "a null pointer");
  if (const char* why = ups_check(wl, hl, params)) return img_refuse(who, why);
  const size_t nl = (size_t)wl * (size_t)hl, n = nl * (size_t)params->factor * (size_t)params->factor, f = sizeof(float);
  if (dn_overlap(out, 3 * n * f, rgb_lo, 3 * nl * f) || dn_overlap(out, 3 * n * f, normal_lo, 3 * nl * f) ||
      dn_overlap(out, 3 * n * f, depth_lo, nl * f) || dn_overlap(out, 3 * n * f, normal, 3 * n * f) || dn_overlap(out, 3 * n * f, depth, n * f))
    return img_refuse(who, "out overlaps an input");
  return DR_OK;
}

extern "C" int dr_upsample_check(const DrUpsampleParams* params, int32_t wl, int32_t hl) { return img_refuse("dr_upsample_check", ups_check(wl, hl, params)); }

extern "C" int dr_upsample_host(const float* rgb_lo, const float* normal_lo, const float* depth_lo, int32_t wl, int32_t hl, const float* normal,
                                const float* depth, const DrUpsampleParams* params, float* out) {
  const int rc = ups_check_images("dr_upsample_host", rgb_lo, normal_lo, depth_lo, wl, hl, normal, depth, params, out);
  if (rc != DR_OK) return rc;
  const size_t nl = (size_t)wl * (size_t)hl;
  std::vector<DnTexel> colour(nl), guide(nl);
  const DnInputs lo = {rgb_lo, normal_lo, depth_lo};
  for (size_t q = 0; q < nl; ++q) {
    colour[q] = lo.colour(q);
    guide[q] = lo.guide(q);
  }
  const int32_t f = params->factor, w = f * wl, h = f * hl;
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x)
      ups_pixel(colour.data(), guide.data(), wl, hl, normal, depth, w, f, params->taps, params->k_normal, params->k_depth, x, y,
                out + 3 * ((size_t)y * (size_t)w + (size_t)x));
  return DR_OK;
}
