// dr_denoise_device.hip -- the three a-trous filters ON THE GPU: the edge-avoiding one, dr_denoise_atrous (host buffers)
// and dr_denoise_atrous_device (device buffers, asynchronous on a stream), the variance-guided one over two half renders (DESIGN.md
// 2.19), dr_denoise_pair and dr_denoise_pair_device, and the variance-guided one over a temporal history,
// dr_denoise_moments and dr_denoise_moments_device.  One pack kernel and one level kernel, each compiled once per rule (DnRule of
// dr_denoise.h, DnpRule of dr_denoise_pair.h, DnmRule of dr_denoise_moments.h), and the moments form's variance estimate:
//   k_image_pack<Inputs>     dr_image_device.h.  The pair filter's colour is (mean r, g, b, variance or -1), the moments form's
//                            (r, g, b, history length or -1)
//   k_moments_variance       lane = pixel on the tile walk of the level kernel: the pack's colour plane becomes the first plane the levels
//                            read, (r, g, b, variance or -1).  A lane with a long history reads its own texel and its m2; a lane with a
//                            short one gathers up to 7 x 7 texel pairs by direct 16-byte loads, as a level does and for the same reason
//                            (below): the window's rows are the wave's own 1 KiB run shifted by at most three pixels.  Only those lanes
//                            run the gather, so a wave that holds one diverges for its length; in a camera animation they are the
//                            disocclusion bands.  No LDS tile: none has been measured against this form (MEASUREMENTS.md).
//   k_denoise_level<Rule>    lane = pixel, one launch per level: 64 x 4 tiles whose rows are contiguous in x -- a wave is 64 neighbours of
//                            one image row, and its tap at dx * s is the same 1 KiB run shifted, so every tap load stays coalesced at every
//                            step; the nine loads of the variance prefilter are the same run shifted by one pixel and one row.  The levels
//                            take turns between two colour planes; the last one writes [h][w][3] and, for the two variance-guided forms
//                            when asked, [h][w].
// A call is two halves: make the two planes (the pack; for the moments form the pack and the estimate), then run the levels (run_levels,
// shared by the three rules).  The per-pixel rules are the ones the host loops run: the outputs are byte-identical
// (tests/test_gpu_denoise.py, tests/test_gpu_denoise_pair.py, tests/test_gpu_denoise_moments.py).  Every tap's coordinates are checked
// against w and h before its loads (dn_pixel, dnp_pixel, dnm_variance); the tile walk is dr_image_device.h's.  No LDS: a level's 25 taps
// per pixel hit lines its neighbours in the tile and the tiles around it have just brought into L2, and the traffic that reaches HBM is
// the 32 B read + 16 B written per pixel.
#include "dr_denoise_moments.h"
#include "dr_image_device.h"

namespace {

// dst: the next level's colour plane; or out3: the image, with outv: the variance image or NULL (the last level)
template <class Rule>
__global__ void __launch_bounds__(DR_IMG_TILE_X* DR_IMG_TILE_Y) k_denoise_level(const DnTexel* colour, const DnTexel* guide, int32_t w, int32_t h,
                                                                               int32_t s, Rule rule, uint64_t tilesX, uint64_t ntiles,
                                                                               DnTexel* dst, float* out3, float* outv) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t x, y;
    if (!img_tile_pixel(t, tilesX, w, h, &x, &y)) continue;
    const DnTexel r = rule.pixel(colour, guide, w, h, (int32_t)x, (int32_t)y, s);
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    if (out3) {
      out3[3 * p] = r.x;
      out3[3 * p + 1] = r.y;
      out3[3 * p + 2] = r.z;
      if (Rule::kVariance && outv) outv[p] = r.w;
    } else {
      dst[p] = r;
    }
  }
}

// the guide plane and the two colour planes the levels take turns between
uint64_t scratch_need(int32_t w, int32_t h) { return 3ull * sizeof(DnTexel) * (uint64_t)w * (uint64_t)h; }

// The second half of a call: the levels, on the two planes the first half has made.  `src` is read first
template <class Rule>
int run_levels(const char* who, DnTexel* src, DnTexel* dst, const DnTexel* guide, int32_t w, int32_t h, const typename Rule::Params& prm,
               float* out, float* out_var, hipStream_t s) {
  const ImgTiles tl = img_tiles(w, h);
  for (int i = 0; i < prm.iterations; ++i) {
    const bool last = i == prm.iterations - 1;
    hipLaunchKernelGGL(k_denoise_level<Rule>, dim3(tl.grid), dim3(DR_IMG_TILE_X, DR_IMG_TILE_Y), 0, s, (const DnTexel*)src, guide, w, h,
                       (int32_t)(1 << i), Rule::level(prm, i), tl.tilesX, tl.ntiles, last ? (DnTexel*)nullptr : dst,
                       last ? out : (float*)nullptr, last ? out_var : (float*)nullptr);
    ST(hipGetLastError());
    std::swap(src, dst);
  }
  return DR_OK;
}

// The launches of one call of the a-trous filter or its pair form, on device buffers that the caller has checked: the pack, the levels
template <class Rule>
int run(const char* who, const typename Rule::Inputs& in, int32_t w, int32_t h, const typename Rule::Params& prm, float* out, float* out_var,
        void* scratch, hipStream_t s) {
  const uint64_t n = (uint64_t)w * (uint64_t)h;
  DnTexel* guide = (DnTexel*)scratch;
  DnTexel* src = guide + n;
  DnTexel* dst = src + n;
  const int rc = img_pack(who, in, n, src, guide, s);
  if (rc != DR_OK) return rc;
  return run_levels<Rule>(who, src, dst, guide, w, h, prm, out, out_var, s);
}

// The moments form's variance estimate: packed (r, g, b, len or -1) -> first (r, g, b, v or -1), and outv0: v as an image, or NULL
__global__ void __launch_bounds__(DR_IMG_TILE_X* DR_IMG_TILE_Y) k_moments_variance(const DnTexel* packed, const DnTexel* guide, const float* m2,
                                                                                  int32_t w, int32_t h, int32_t min_history, int32_t radius,
                                                                                  float kn, float kz, uint64_t tilesX, uint64_t ntiles,
                                                                                  DnTexel* first, float* outv0) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t x, y;
    if (!img_tile_pixel(t, tilesX, w, h, &x, &y)) continue;
    const DnTexel r = dnm_variance(packed, guide, m2, w, h, (int32_t)x, (int32_t)y, min_history, radius, kn, kz);
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    first[p] = r;
    if (outv0) outv0[p] = r.w;
  }
}

// The launches of one call of the moments form: the pack into the levels' second plane, the estimate from it into their first, the levels
int run_moments(const char* who, const DnmInputs& in, int32_t w, int32_t h, const DrDenoiseMomentsParams& prm, float* out, float* out_var,
                float* out_var0, void* scratch, hipStream_t s) {
  const uint64_t n = (uint64_t)w * (uint64_t)h;
  DnTexel* guide = (DnTexel*)scratch;
  DnTexel* first = guide + n;
  DnTexel* packed = first + n;
  const int rc = img_pack(who, in, n, packed, guide, s);
  if (rc != DR_OK) return rc;
  const ImgTiles tl = img_tiles(w, h);
  hipLaunchKernelGGL(k_moments_variance, dim3(tl.grid), dim3(DR_IMG_TILE_X, DR_IMG_TILE_Y), 0, s, (const DnTexel*)packed, (const DnTexel*)guide,
                     in.m2, w, h, prm.min_history, prm.radius, prm.k_normal, prm.k_depth, tl.tilesX, tl.ntiles, first, out_var0);
  ST(hipGetLastError());
  return run_levels<DnmRule>(who, first, packed, guide, w, h, prm, out, out_var, s);
}

}  // namespace

extern "C" int dr_denoise_atrous_device(const void* rgb_dev, const void* normal_dev, const void* depth_dev, int32_t w, int32_t h,
                                        const DrDenoiseParams* params, void* out_dev, void* scratch_dev, uint64_t* scratch_bytes,
                                        void* hip_stream) {
  const char* who = "dr_denoise_atrous_device";
  if (!scratch_bytes || !params) return img_refuse(who, "a null pointer");
  int rc = scratch_dev ? dn_check_images(who, rgb_dev, normal_dev, depth_dev, w, h, params, out_dev) : img_refuse(who, dn_check(w, h, params));
  if (rc != DR_OK) return rc;
  const uint64_t need = scratch_need(w, h);
  if (img_scratch(who, scratch_dev, scratch_bytes, need, &rc)) return rc;
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  if (dn_overlap(out_dev, 3 * n * f, scratch_dev, (size_t)need)) return img_refuse(who, "out overlaps the scratch buffer");
  if ((rc = img_device_ready(who)) != DR_OK) return rc;
  return run<DnRule>(who, DnInputs{(const float*)rgb_dev, (const float*)normal_dev, (const float*)depth_dev}, w, h, *params, (float*)out_dev,
                     nullptr, scratch_dev, (hipStream_t)hip_stream);
}

extern "C" int dr_denoise_atrous(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h, const DrDenoiseParams* params,
                                 float* out) {
  const char* who = "dr_denoise_atrous";
  int rc = dn_check_images(who, rgb, normal, depth, w, h, params, out);
  if (rc != DR_OK || (rc = img_device_ready(who)) != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  Buf<float> dRgb, dNormal, dDepth, dOut;
  Buf<DnTexel> scratch;
  ST(dRgb.alloc(3 * n));
  ST(dNormal.alloc(3 * n));
  ST(dDepth.alloc(n));
  ST(dOut.alloc(3 * n));
  ST(scratch.alloc(3 * n));
  hipStream_t s = 0;
  ST(dRgb.upload(rgb, 3 * n, s));
  ST(dNormal.upload(normal, 3 * n, s));
  ST(dDepth.upload(depth, n, s));
  if ((rc = run<DnRule>(who, DnInputs{dRgb.p, dNormal.p, dDepth.p}, w, h, *params, dOut.p, nullptr, scratch.p, s)) != DR_OK) return rc;
  ST(dOut.download(out, 3 * n, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}

extern "C" int dr_denoise_pair_device(const void* a_dev, const void* b_dev, const void* normal_dev, const void* depth_dev, int32_t w, int32_t h,
                                      const DrDenoisePairParams* params, void* out_dev, void* out_var_dev, void* scratch_dev,
                                      uint64_t* scratch_bytes, void* hip_stream) {
  const char* who = "dr_denoise_pair_device";
  if (!scratch_bytes || !params) return img_refuse(who, "a null pointer");
  int rc = scratch_dev ? dnp_check_images(who, a_dev, b_dev, normal_dev, depth_dev, w, h, params, out_dev, out_var_dev)
                       : img_refuse(who, dnp_check(w, h, params));
  if (rc != DR_OK) return rc;
  const uint64_t need = scratch_need(w, h);
  if (img_scratch(who, scratch_dev, scratch_bytes, need, &rc)) return rc;
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  if (dn_overlap(out_dev, 3 * n * f, scratch_dev, (size_t)need)) return img_refuse(who, "out overlaps the scratch buffer");
  if (out_var_dev && dn_overlap(out_var_dev, n * f, scratch_dev, (size_t)need)) return img_refuse(who, "out_var overlaps the scratch buffer");
  if ((rc = img_device_ready(who)) != DR_OK) return rc;
  return run<DnpRule>(who, DnpInputs{(const float*)a_dev, (const float*)b_dev, (const float*)normal_dev, (const float*)depth_dev}, w, h, *params,
                      (float*)out_dev, (float*)out_var_dev, scratch_dev, (hipStream_t)hip_stream);
}

extern "C" int dr_denoise_pair(const float* a, const float* b, const float* normal, const float* depth, int32_t w, int32_t h,
                               const DrDenoisePairParams* params, float* out, float* out_var) {
  const char* who = "dr_denoise_pair";
  int rc = dnp_check_images(who, a, b, normal, depth, w, h, params, out, out_var);
  if (rc != DR_OK || (rc = img_device_ready(who)) != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  Buf<float> dA, dB, dNormal, dDepth, dOut, dVar;
  Buf<DnTexel> scratch;
  ST(dA.alloc(3 * n));
  ST(dB.alloc(3 * n));
  ST(dNormal.alloc(3 * n));
  ST(dDepth.alloc(n));
  ST(dOut.alloc(3 * n));
  if (out_var) ST(dVar.alloc(n));
  ST(scratch.alloc(3 * n));
  hipStream_t s = 0;
  ST(dA.upload(a, 3 * n, s));
  ST(dB.upload(b, 3 * n, s));
  ST(dNormal.upload(normal, 3 * n, s));
  ST(dDepth.upload(depth, n, s));
  if ((rc = run<DnpRule>(who, DnpInputs{dA.p, dB.p, dNormal.p, dDepth.p}, w, h, *params, dOut.p, dVar.p, scratch.p, s)) != DR_OK) return rc;
  ST(dOut.download(out, 3 * n, s));
  if (out_var) ST(dVar.download(out_var, n, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}

extern "C" int dr_denoise_moments_device(const void* rgb_dev, const void* m2_dev, const void* len_dev, const void* normal_dev,
                                         const void* depth_dev, int32_t w, int32_t h, const DrDenoiseMomentsParams* params, void* out_dev,
                                         void* out_var_dev, void* out_var0_dev, void* scratch_dev, uint64_t* scratch_bytes, void* hip_stream) {
  const char* who = "dr_denoise_moments_device";
  if (!scratch_bytes || !params) return img_refuse(who, "a null pointer");
  int rc = scratch_dev ? dnm_check_images(who, DnmImages{rgb_dev, m2_dev, len_dev, normal_dev, depth_dev, out_dev, out_var_dev, out_var0_dev}, w, h,
                                          params)
                       : img_refuse(who, dnm_check(w, h, params));
  if (rc != DR_OK) return rc;
  const uint64_t need = scratch_need(w, h);
  if (img_scratch(who, scratch_dev, scratch_bytes, need, &rc)) return rc;
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  if (dn_overlap(out_dev, 3 * n * f, scratch_dev, (size_t)need)) return img_refuse(who, "out overlaps the scratch buffer");
  if (out_var_dev && dn_overlap(out_var_dev, n * f, scratch_dev, (size_t)need)) return img_refuse(who, "out_var overlaps the scratch buffer");
  if (out_var0_dev && dn_overlap(out_var0_dev, n * f, scratch_dev, (size_t)need)) return img_refuse(who, "out_var0 overlaps the scratch buffer");
  if ((rc = img_device_ready(who)) != DR_OK) return rc;
  return run_moments(who, DnmInputs{(const float*)rgb_dev, (const float*)m2_dev, (const float*)len_dev, (const float*)normal_dev, (const float*)depth_dev},
                     w, h, *params, (float*)out_dev, (float*)out_var_dev, (float*)out_var0_dev, scratch_dev, (hipStream_t)hip_stream);
}

extern "C" int dr_denoise_moments(const float* rgb, const float* m2, const float* len, const float* normal, const float* depth, int32_t w, int32_t h,
                                  const DrDenoiseMomentsParams* params, float* out, float* out_var, float* out_var0) {
  const char* who = "dr_denoise_moments";
  int rc = dnm_check_images(who, DnmImages{rgb, m2, len, normal, depth, out, out_var, out_var0}, w, h, params);
  if (rc != DR_OK || (rc = img_device_ready(who)) != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  Buf<float> dRgb, dM2, dLen, dNormal, dDepth, dOut, dVar, dVar0;
  Buf<DnTexel> scratch;
  ST(dRgb.alloc(3 * n));
  ST(dM2.alloc(n));
  ST(dLen.alloc(n));
  ST(dNormal.alloc(3 * n));
  ST(dDepth.alloc(n));
  ST(dOut.alloc(3 * n));
  if (out_var) ST(dVar.alloc(n));
  if (out_var0) ST(dVar0.alloc(n));
  ST(scratch.alloc(3 * n));
  hipStream_t s = 0;
  ST(dRgb.upload(rgb, 3 * n, s));
  ST(dM2.upload(m2, n, s));
  ST(dLen.upload(len, n, s));
  ST(dNormal.upload(normal, 3 * n, s));
  ST(dDepth.upload(depth, n, s));
  if ((rc = run_moments(who, DnmInputs{dRgb.p, dM2.p, dLen.p, dNormal.p, dDepth.p}, w, h, *params, dOut.p, dVar.p, dVar0.p, scratch.p, s)) != DR_OK) return rc;
  ST(dOut.download(out, 3 * n, s));
  if (out_var) ST(dVar.download(out_var, n, s));
  if (out_var0) ST(dVar0.download(out_var0, n, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}
