// dr_denoise_moments_host.cpp -- the variance-guided a-trous filter over a temporal history on the host:
// dr_denoise_moments_host, the pack, the variance estimate and the serial level loop of dr_denoise.h (dn_run_levels_host) over the
// per-pixel rules of dr_denoise_moments.h -- the ones the kernels of dr_denoise_device.hip run, one lane per pixel, so the two write the
// same bytes -- and dr_denoise_moments_check.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here needs
// the HIP runtime, so the file also builds as plain C++.
#include "dr_denoise_moments.h"

int dnm_check_images(const char* who, const DnmImages& im, int32_t w, int32_t h, const DrDenoiseMomentsParams* params) {
  if (!im.rgb || !im.m2 || !im.len || !im.normal || !im.depth || !im.out || !params) return img_refuse(who, "a null pointer");
  if (const char* why = dnm_check(w, h, params)) return img_refuse(who, why);
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  const void* in[5] = {im.rgb, im.m2, im.len, im.normal, im.depth};
  const size_t bytes[5] = {3 * n * f, n * f, n * f, 3 * n * f, n * f};
  for (int i = 0; i < 5; ++i) {
    if (dn_overlap(im.out, 3 * n * f, in[i], bytes[i])) return img_refuse(who, "out overlaps an input");
    if (im.out_var && dn_overlap(im.out_var, n * f, in[i], bytes[i])) return img_refuse(who, "out_var overlaps an input");
    if (im.out_var0 && dn_overlap(im.out_var0, n * f, in[i], bytes[i])) return img_refuse(who, "out_var0 overlaps an input");
  }
  if (im.out_var && dn_overlap(im.out, 3 * n * f, im.out_var, n * f)) return img_refuse(who, "out overlaps out_var");
  if (im.out_var0 && dn_overlap(im.out, 3 * n * f, im.out_var0, n * f)) return img_refuse(who, "out overlaps out_var0");
  if (im.out_var && im.out_var0 && dn_overlap(im.out_var, n * f, im.out_var0, n * f)) return img_refuse(who, "out_var overlaps out_var0");
  return DR_OK;
}

extern "C" int dr_denoise_moments_check(const DrDenoiseMomentsParams* params, int32_t w, int32_t h) {
  return img_refuse("dr_denoise_moments_check", dnm_check(w, h, params));
}

extern "C" int dr_denoise_moments_host(const float* rgb, const float* m2, const float* len, const float* normal, const float* depth, int32_t w,
                                       int32_t h, const DrDenoiseMomentsParams* params, float* out, float* out_var, float* out_var0) {
  const int rc = dnm_check_images("dr_denoise_moments_host", DnmImages{rgb, m2, len, normal, depth, out, out_var, out_var0}, w, h, params);
  if (rc != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  // the pack's colour plane is the estimate's input and then the levels' second plane
  std::vector<DnTexel> guide(n), first(n), packed(n);
  dn_pack_host(DnmInputs{rgb, m2, len, normal, depth}, n, packed.data(), guide.data());
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t p = (size_t)y * (size_t)w + (size_t)x;
      first[p] = dnm_variance(packed.data(), guide.data(), m2, w, h, x, y, params->min_history, params->radius, params->k_normal, params->k_depth);
      if (out_var0) out_var0[p] = first[p].w;
    }
  dn_run_levels_host<DnmRule>(first.data(), packed.data(), guide.data(), w, h, *params, out, out_var);
  return DR_OK;
}
