// dr_temporal_device.hip -- temporal accumulation with reprojection ON THE GPU: dr_temporal (host buffers) and
// dr_temporal_device (device buffers, asynchronous on a stream).
//   k_temporal   lane = pixel, one launch: 64 x 4 tiles whose rows are contiguous in x -- a wave is 64 neighbours of one image row, so its
//                reads of rgb / normal / depth and its writes of out_rgb / out_m2 / out_len are coalesced; the 2 x 2 history taps are a
//                gather whose addresses follow the camera move, neighbouring lanes to neighbouring previous pixels for any smooth one.
// The per-pixel rule is dr_temporal.h's, the one the host loop runs (dr_temporal_host.cpp): the outputs are byte-identical
// (tests/test_gpu_temporal.py).  Every tap's coordinates are checked against w and h before its loads (tp_history); the tile walk is
// dr_image_device.h's.  The three matrices and the eleven image pointers travel as kernel arguments (uniform: scalar registers).  No LDS,
// no atomics, no scratch buffer: a pixel reads 28 B of its own frame, up to 4 x 36 B of history that its neighbours share (36 B per pixel
// where the move is smooth) and writes 20 B.
#include "dr_image_device.h"
#include "dr_temporal.h"

namespace {

__global__ void __launch_bounds__(DR_IMG_TILE_X* DR_IMG_TILE_Y) k_temporal(TpImages im, int32_t w, int32_t h, DrTemporalParams prm, uint64_t tilesX,
                                                                          uint64_t ntiles) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t x, y;
    if (!img_tile_pixel(t, tilesX, w, h, &x, &y)) continue;
    tp_pixel(im, w, h, prm, (int32_t)x, (int32_t)y);
  }
}

// The launch of one call, on device buffers that the caller has checked
int run(const char* who, const TpImages& im, int32_t w, int32_t h, const DrTemporalParams& prm, hipStream_t s) {
  const ImgTiles tl = img_tiles(w, h);
  hipLaunchKernelGGL(k_temporal, dim3(tl.grid), dim3(DR_IMG_TILE_X, DR_IMG_TILE_Y), 0, s, im, w, h, prm, tl.tilesX, tl.ntiles);
  ST(hipGetLastError());
  return DR_OK;
}

}  // namespace

extern "C" int dr_temporal_device(const void* rgb_dev, const void* normal_dev, const void* depth_dev, const void* h_rgb_dev, const void* h_m2_dev,
                                  const void* h_len_dev, const void* h_normal_dev, const void* h_depth_dev, int32_t w, int32_t h,
                                  const DrTemporalParams* params, void* out_rgb_dev, void* out_m2_dev, void* out_len_dev, void* hip_stream) {
  const char* who = "dr_temporal_device";
  const TpImages im = {(const float*)rgb_dev,      (const float*)normal_dev,  (const float*)depth_dev, (const float*)h_rgb_dev,
                       (const float*)h_m2_dev,     (const float*)h_len_dev,   (const float*)h_normal_dev, (const float*)h_depth_dev,
                       (float*)out_rgb_dev,        (float*)out_m2_dev,        (float*)out_len_dev};
  int rc = tp_check_images(who, im, w, h, params);
  if (rc != DR_OK || (rc = img_device_ready(who)) != DR_OK) return rc;
  return run(who, im, w, h, *params, (hipStream_t)hip_stream);
}

extern "C" int dr_temporal(const float* rgb, const float* normal, const float* depth, const float* h_rgb, const float* h_m2, const float* h_len,
                           const float* h_normal, const float* h_depth, int32_t w, int32_t h, const DrTemporalParams* params, float* out_rgb,
                           float* out_m2, float* out_len) {
  const char* who = "dr_temporal";
  const TpImages host = {rgb, normal, depth, h_rgb, h_m2, h_len, h_normal, h_depth, out_rgb, out_m2, out_len};
  int rc = tp_check_images(who, host, w, h, params);
  if (rc != DR_OK || (rc = img_device_ready(who)) != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  const bool hist = h_rgb != nullptr;
  Buf<float> dRgb, dNormal, dDepth, dHRgb, dHM2, dHLen, dHNormal, dHDepth, dOutRgb, dOutM2, dOutLen;
  ST(dRgb.alloc(3 * n));
  ST(dNormal.alloc(3 * n));
  ST(dDepth.alloc(n));
  ST(dOutRgb.alloc(3 * n));
  ST(dOutM2.alloc(n));
  ST(dOutLen.alloc(n));
  hipStream_t s = 0;
  ST(dRgb.upload(rgb, 3 * n, s));
  ST(dNormal.upload(normal, 3 * n, s));
  ST(dDepth.upload(depth, n, s));
  if (hist) {
    ST(dHRgb.alloc(3 * n));
    ST(dHM2.alloc(n));
    ST(dHLen.alloc(n));
    ST(dHNormal.alloc(3 * n));
    ST(dHDepth.alloc(n));
    ST(dHRgb.upload(h_rgb, 3 * n, s));
    ST(dHM2.upload(h_m2, n, s));
    ST(dHLen.upload(h_len, n, s));
    ST(dHNormal.upload(h_normal, 3 * n, s));
    ST(dHDepth.upload(h_depth, n, s));
  }
  const TpImages im = {dRgb.p, dNormal.p, dDepth.p, dHRgb.p, dHM2.p, dHLen.p, dHNormal.p, dHDepth.p, dOutRgb.p, dOutM2.p, dOutLen.p};
  if ((rc = run(who, im, w, h, *params, s)) != DR_OK) return rc;
  ST(dOutRgb.download(out_rgb, 3 * n, s));
  ST(dOutM2.download(out_m2, n, s));
  ST(dOutLen.download(out_len, n, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}
