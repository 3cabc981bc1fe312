// dr_demodulate_host.cpp -- demodulation on the host: dr_demodulate_host and dr_remodulate_host, serial loops over the
// per-pixel rules of dr_demodulate.h -- the rules the kernels of dr_demodulate_device.hip run, so the two write the same bytes -- and
// dr_demodulate_check.  Runs without a GPU: the fallback, and the device version's checker.  Nothing here needs the HIP runtime, so the
// file also builds as plain C++.
#include "dr_demodulate.h"

int demod_check_images(const char* who, const DemodImages& im, int32_t w, int32_t h, const DrDemodulateParams* params) {
  if (!im.rgb || !im.out || !params) return img_refuse(who, "a null pointer");
  if (const char* why = demod_check(w, h, params)) return img_refuse(who, why);
  const size_t n = 3 * (size_t)w * (size_t)h * sizeof(float);
  const void* in[3] = {im.rgb, im.emission, im.albedo};
  for (int i = 0; i < 3; ++i)
    if (in[i] && dn_overlap(im.out, n, in[i], n)) return img_refuse(who, "an output overlaps an input");
  return DR_OK;
}

extern "C" int dr_demodulate_check(const DrDemodulateParams* params, int32_t w, int32_t h) {
  return img_refuse("dr_demodulate_check", demod_check(w, h, params));
}

extern "C" int dr_demodulate_host(const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h,
                                  const DrDemodulateParams* params, float* out) {
  const DemodImages im = {rgb, emission, albedo, out};
  const int rc = demod_check_images("dr_demodulate_host", im, w, h, params);
  if (rc != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  for (size_t p = 0; p < n; ++p) demod_pixel(im, params->eps, p);
  return DR_OK;
}

extern "C" int dr_remodulate_host(const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h,
                                  const DrDemodulateParams* params, float* out) {
  const DemodImages im = {rgb, emission, albedo, out};
  const int rc = demod_check_images("dr_remodulate_host", im, w, h, params);
  if (rc != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  for (size_t p = 0; p < n; ++p) remod_pixel(im, params->eps, p);
  return DR_OK;
}
