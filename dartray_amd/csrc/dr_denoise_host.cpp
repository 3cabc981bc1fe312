// dr_denoise_host.cpp -- the edge-avoiding a-trous filter on the host: dr_denoise_atrous_host, a serial loop over
// the per-pixel rule of dr_denoise.h -- the one the kernels of dr_denoise_device.hip run, one lane per pixel, so the two write the
// same bytes.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here needs the HIP runtime, so the file
// also builds as plain C++ (the sanitizer check of tests/denoise_host_check.cpp).
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dartray_hip.h"

#include "dr_denoise.h"

int dn_check_images(const char* who, const void* rgb, const void* normal, const void* depth, int32_t w, int32_t h,
                    const DrDenoiseParams* params, const void* out) {
  const std::string pre = std::string(who) + ": ";
  if (!rgb || !normal || !depth || !out || !params) return dr_fail(DR_ERR_INVALID, pre + "a null pointer");
  if (const char* why = dn_check(w, h, params)) return dr_fail(DR_ERR_INVALID, pre + why);
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  if (dn_overlap(out, 3 * n * f, rgb, 3 * n * f) || dn_overlap(out, 3 * n * f, normal, 3 * n * f) || dn_overlap(out, 3 * n * f, depth, n * f))
    return dr_fail(DR_ERR_INVALID, pre + "out overlaps an input");
  return DR_OK;
}

extern "C" int dr_denoise_atrous_host(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h,
                                      const DrDenoiseParams* params, float* out) {
  const int rc = dn_check_images("dr_denoise_atrous_host", rgb, normal, depth, w, h, params, out);
  if (rc != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  std::vector<DnTexel> guide(n), a(n), b(params->iterations > 1 ? n : 0);
  for (size_t p = 0; p < n; ++p) {
    a[p] = dn_pack_colour(rgb, normal, depth, p);
    guide[p] = dn_pack_guide(normal, depth, p);
  }
  DnTexel* src = a.data();
  DnTexel* dst = b.data();
  for (int i = 0; i < params->iterations; ++i) {
    const bool last = i == params->iterations - 1;
    const float kc = dn_level_kc(params->k_color, i);
    const int32_t s = 1 << i;
    for (int32_t y = 0; y < h; ++y)
      for (int32_t x = 0; x < w; ++x) {
        const DnTexel t = dn_pixel(src, guide.data(), w, h, x, y, s, kc, params->k_normal, params->k_depth);
        const size_t p = (size_t)y * (size_t)w + (size_t)x;
        if (last) {
          out[3 * p] = t.x;
          out[3 * p + 1] = t.y;
          out[3 * p + 2] = t.z;
        } else {
          dst[p] = t;
        }
      }
    DnTexel* t = src;
    src = dst;
    dst = t;
  }
  return DR_OK;
}
