// dr_denoise_host.cpp -- the edge-avoiding a-trous filter on the host: dr_denoise_atrous_host, the serial level loop of
// dr_denoise.h (dn_levels_host) over its per-pixel rule -- the one the kernels of dr_denoise_device.hip run, one lane per pixel, so the
// two write the same bytes.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here needs the HIP runtime, so
// the file also builds as plain C++ (the sanitizer check of tests/denoise_host_check.cpp).
#include "dr_denoise.h"

int dn_check_images(const char* who, const void* rgb, const void* normal, const void* depth, int32_t w, int32_t h,
                    const DrDenoiseParams* params, const void* out) {
  if (!rgb || !normal || !depth || !out || !params) return img_refuse(who, "a null pointer");
  if (const char* why = dn_check(w, h, params)) return img_refuse(who, why);
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  if (dn_overlap(out, 3 * n * f, rgb, 3 * n * f) || dn_overlap(out, 3 * n * f, normal, 3 * n * f) || dn_overlap(out, 3 * n * f, depth, n * f))
    return img_refuse(who, "out overlaps an input");
  return DR_OK;
}

extern "C" int dr_denoise_atrous_host(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h,
                                      const DrDenoiseParams* params, float* out) {
  const int rc = dn_check_images("dr_denoise_atrous_host", rgb, normal, depth, w, h, params, out);
  if (rc != DR_OK) return rc;
  dn_levels_host<DnRule>(DnInputs{rgb, normal, depth}, w, h, *params, out, nullptr);
  return DR_OK;
}
