// dr_denoise_pair_host.cpp -- the variance-guided a-trous filter on the host: dr_denoise_pair_host, a serial loop over
// the per-pixel rule of dr_denoise_pair.h -- the one the kernels of dr_denoise_pair_device.hip run, one lane per pixel, so the two write
// the same bytes.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here needs the HIP runtime.
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dartray_hip.h"

#include "dr_denoise_pair.h"

int dnp_check_images(const char* who, const void* a, const void* b, const void* normal, const void* depth, int32_t w, int32_t h,
                     const DrDenoisePairParams* params, const void* out, const void* out_var) {
  const std::string pre = std::string(who) + ": ";
  if (!a || !b || !normal || !depth || !out || !params) return dr_fail(DR_ERR_INVALID, pre + "a null pointer");
  if (const char* why = dnp_check(w, h, params)) return dr_fail(DR_ERR_INVALID, pre + why);
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  const void* in[4] = {a, b, normal, depth};
  const size_t bytes[4] = {3 * n * f, 3 * n * f, 3 * n * f, n * f};
  for (int i = 0; i < 4; ++i) {
    if (dn_overlap(out, 3 * n * f, in[i], bytes[i])) return dr_fail(DR_ERR_INVALID, pre + "out overlaps an input");
    if (out_var && dn_overlap(out_var, n * f, in[i], bytes[i])) return dr_fail(DR_ERR_INVALID, pre + "out_var overlaps an input");
  }
  if (out_var && dn_overlap(out, 3 * n * f, out_var, n * f)) return dr_fail(DR_ERR_INVALID, pre + "out overlaps out_var");
  return DR_OK;
}

extern "C" int dr_denoise_pair_host(const float* a, const float* b, const float* normal, const float* depth, int32_t w, int32_t h,
                                    const DrDenoisePairParams* params, float* out, float* out_var) {
  const int rc = dnp_check_images("dr_denoise_pair_host", a, b, normal, depth, w, h, params, out, out_var);
  if (rc != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  std::vector<DnTexel> guide(n), c0(n), c1(params->iterations > 1 ? n : 0);
  for (size_t p = 0; p < n; ++p) {
    c0[p] = dnp_pack_colour(a, b, normal, depth, p);
    guide[p] = dn_pack_guide(normal, depth, p);
  }
  DnTexel* src = c0.data();
  DnTexel* dst = c1.data();
  for (int i = 0; i < params->iterations; ++i) {
    const bool last = i == params->iterations - 1;
    const int32_t s = 1 << i;
    for (int32_t y = 0; y < h; ++y)
      for (int32_t x = 0; x < w; ++x) {
        const DnTexel t = dnp_pixel(src, guide.data(), w, h, x, y, s, params->k_color, params->k_normal, params->k_depth, params->var_floor);
        const size_t p = (size_t)y * (size_t)w + (size_t)x;
        if (last) {
          out[3 * p] = t.x;
          out[3 * p + 1] = t.y;
          out[3 * p + 2] = t.z;
          if (out_var) out_var[p] = t.w;
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
