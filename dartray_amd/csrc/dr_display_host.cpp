// dr_display_host.cpp -- the display transform on the host: the encode tables (the only place a pow is spent),
// dr_display_check, dr_display_table, dr_display_exposure_host and dr_display_host, a serial loop over the per-pixel rules of dr_display.h --
// the ones the kernels of dr_display_device.hip run, one lane per pixel, so the two write the same bytes.  Runs without a GPU: the fallback,
// and the device version's checker.  Nothing here needs the HIP runtime.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dartray_hip.h"

#include "dr_display.h"

namespace {

// Thresholds: word 0 is 0 (never read by the search), word k the f32 of the linear value whose encoded value times 255 is k - 0.5.
// Reference: word i is ImageFilm's _gamma[i] (film/image_film.dart:55-58), with the C library's pow.
DspTable fill_table(uint32_t encode) {
  DspTable t;
  for (int k = 0; k < DR_DISPLAY_TABLE; ++k) {
    if (encode == DR_ENCODE_REFERENCE) {
      const double g = std::floor(std::pow(k / 255.0, 1.0 / 2.2) * 255.0);
      t.w[k] = g < 0.0 ? 0u : (g > 255.0 ? 255u : (uint32_t)g);
    } else if (k == 0) {
      t.w[k] = 0u;
    } else {
      const double v = (k - 0.5) / 255.0;
      const double lin = encode == DR_ENCODE_SRGB ? (v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4)) : std::pow(v, 2.2);
      t.w[k] = dsp_bits((float)lin);
    }
  }
  return t;
}

}  // namespace

const DspTable& dsp_table(uint32_t encode) {
  static const DspTable srgb = fill_table(DR_ENCODE_SRGB), gamma22 = fill_table(DR_ENCODE_GAMMA22), reference = fill_table(DR_ENCODE_REFERENCE);
  return encode == DR_ENCODE_SRGB ? srgb : encode == DR_ENCODE_GAMMA22 ? gamma22 : reference;
}

int dsp_check_images(const char* who, const void* rgb, int32_t w, int32_t h, const DrDisplayParams* params, const void* out, bool has_out) {
  if (!rgb || !params || (has_out && !out)) return img_refuse(who, "a null pointer");
  if (const char* why = dsp_check(params, w, h)) return img_refuse(who, why);
  const size_t n = (size_t)w * (size_t)h;
  if (has_out && dn_overlap(out, 4 * n, rgb, 3 * n * sizeof(float))) return img_refuse(who, "out overlaps an input");
  return DR_OK;
}

extern "C" int dr_display_check(const DrDisplayParams* params, int32_t w, int32_t h) { return img_refuse("dr_display_check", dsp_check(params, w, h)); }

extern "C" int dr_display_table(uint32_t encode, uint32_t* out, uint32_t n) {
  const std::string pre = "dr_display_table: ";
  if (!out) return dr_fail(DR_ERR_INVALID, pre + "a null pointer");
  if (encode > DR_ENCODE_REFERENCE) return dr_fail(DR_ERR_INVALID, pre + "encode must be DR_ENCODE_SRGB, DR_ENCODE_GAMMA22 or DR_ENCODE_REFERENCE");
  if (n != DR_DISPLAY_TABLE) return dr_fail(DR_ERR_INVALID, pre + "n must be 256");
  const DspTable& t = dsp_table(encode);
  for (int k = 0; k < DR_DISPLAY_TABLE; ++k) out[k] = t.w[k];
  return DR_OK;
}

extern "C" int dr_display_exposure_host(const float* rgb, int32_t w, int32_t h, const DrDisplayParams* params, float* scale, uint32_t* hist) {
  const int rc = dsp_check_images("dr_display_exposure_host", rgb, w, h, params, nullptr, false);
  if (rc != DR_OK) return rc;
  if (!scale) return dr_fail(DR_ERR_INVALID, "dr_display_exposure_host: a null pointer");
  std::vector<uint32_t> counts(DR_DISPLAY_BINS, 0u);
  const size_t n = (size_t)w * (size_t)h;
  for (size_t p = 0; p < n; ++p) {
    const uint32_t b = dsp_bin(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
    if (b < DR_DISPLAY_BINS) ++counts[b];
  }
  *scale = dsp_pick(counts.data(), params->permille, params->key);
  if (hist)
    for (uint32_t b = 0; b < DR_DISPLAY_BINS; ++b) hist[b] = counts[b];
  return DR_OK;
}

extern "C" int dr_display_host(const float* rgb, int32_t w, int32_t h, const DrDisplayParams* params, uint8_t* out) {
  const int rc = dsp_check_images("dr_display_host", rgb, w, h, params, out, true);
  if (rc != DR_OK) return rc;
  float scale = params->exposure;
  if (params->auto_exposure) {
    const int rc2 = dr_display_exposure_host(rgb, w, h, params, &scale, nullptr);
    if (rc2 != DR_OK) return rc2;
  }
  const DspTable& table = dsp_table(params->encode);
  const size_t n = (size_t)w * (size_t)h;
  for (size_t p = 0; p < n; ++p) {
    const uint32_t px = dsp_pixel(table.w, *params, scale, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
    out[4 * p] = (uint8_t)(px & 0xffu);
    out[4 * p + 1] = (uint8_t)((px >> 8) & 0xffu);
    out[4 * p + 2] = (uint8_t)((px >> 16) & 0xffu);
    out[4 * p + 3] = (uint8_t)(px >> 24);
  }
  return DR_OK;
}
