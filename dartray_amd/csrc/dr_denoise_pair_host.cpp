// dr_denoise_pair_host.cpp -- the variance-guided a-trous filter on the host: dr_denoise_pair_host, the serial level loop
// of dr_denoise.h (dn_levels_host) over the per-pixel rule of dr_denoise_pair.h -- the one the kernels of dr_denoise_device.hip run, one
// lane per pixel, so the two write the same bytes.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here
// needs the HIP runtime.
#include "dr_denoise_pair.h"

int dnp_check_images(const char* who, const void* a, const void* b, const void* normal, const void* depth, int32_t w, int32_t h,
                     const DrDenoisePairParams* params, const void* out, const void* out_var) {
  if (!a || !b || !normal || !depth || !out || !params) return img_refuse(who, "a null pointer");
  if (const char* why = dnp_check(w, h, params)) return img_refuse(who, why);
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  const void* in[4] = {a, b, normal, depth};
  const size_t bytes[4] = {3 * n * f, 3 * n * f, 3 * n * f, n * f};
  for (int i = 0; i < 4; ++i) {
    if (dn_overlap(out, 3 * n * f, in[i], bytes[i])) return img_refuse(who, "out overlaps an input");
    if (out_var && dn_overlap(out_var, n * f, in[i], bytes[i])) return img_refuse(who, "out_var overlaps an input");
  }
  if (out_var && dn_overlap(out, 3 * n * f, out_var, n * f)) return img_refuse(who, "out overlaps out_var");
  return DR_OK;
}

extern "C" int dr_denoise_pair_host(const float* a, const float* b, const float* normal, const float* depth, int32_t w, int32_t h,
                                    const DrDenoisePairParams* params, float* out, float* out_var) {
  const int rc = dnp_check_images("dr_denoise_pair_host", a, b, normal, depth, w, h, params, out, out_var);
  if (rc != DR_OK) return rc;
  dn_levels_host<DnpRule>(DnpInputs{a, b, normal, depth}, w, h, *params, out, out_var);
  return DR_OK;
}
