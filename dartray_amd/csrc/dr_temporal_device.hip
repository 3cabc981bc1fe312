// dr_temporal_device.hip -- temporal accumulation with reprojection ON THE GPU: dr_temporal (host buffers) and
// dr_temporal_device (device buffers, asynchronous on a stream).
//   k_temporal   lane = pixel, one launch: 64 x 4 tiles whose rows are contiguous in x -- a wave is 64 neighbours of one image row, so its
//                reads of rgb / normal / depth and its writes of out_rgb / out_m2 / out_len are coalesced; the 2 x 2 history taps are a
//                gather whose addresses follow the camera move, neighbouring lanes to neighbouring previous pixels for any smooth one.
// The per-pixel rule is dr_temporal.h's, the one the host loop runs (dr_temporal_host.cpp): the outputs are byte-identical
// (tests/test_gpu_temporal.py).  Every tap's coordinates are checked against w and h before its loads (tp_history); a workgroup walks the
// tiles t = blockIdx.x, + gridDim.x, ... so that no image shape needs more workgroups than a launch may have, and a lane whose pixel lies
// outside the image skips the tile before any access.  The three matrices and the eleven image pointers travel as kernel arguments (uniform:
// scalar registers).  No LDS, no atomics, no scratch buffer: a pixel reads 28 B of its own frame, up to 4 x 36 B of history that its
// neighbours share (36 B per pixel where the move is smooth) and writes 20 B.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/dartray_hip.h"

#include "dr_temporal.h"

namespace {

#define DR_TP_TILE_X 64  // one wave = one row of the tile
#define DR_TP_TILE_Y 4
#define DR_TP_MAX_GRID (1u << 20)

__global__ void __launch_bounds__(DR_TP_TILE_X* DR_TP_TILE_Y) k_temporal(TpImages im, int32_t w, int32_t h, DrTemporalParams prm, uint64_t tilesX,
                                                                        uint64_t ntiles) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t x = (t % tilesX) * DR_TP_TILE_X + threadIdx.x, y = (t / tilesX) * DR_TP_TILE_Y + threadIdx.y;
    if (x >= (uint64_t)w || y >= (uint64_t)h) continue;
    tp_pixel(im, w, h, prm, (int32_t)x, (int32_t)y);
  }
}

template <class T>
struct Buf {
  T* p = nullptr;
  hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};
#define ST(x)                                                                                                  \
  do {                                                                                                         \
    hipError_t e_ = (x);                                                                                       \
    if (e_ != hipSuccess) return dr_fail(DR_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e_)); \
  } while (0)

// The launch of one call, on device buffers that the caller has checked
int run(const char* who, const TpImages& im, int32_t w, int32_t h, const DrTemporalParams& prm, hipStream_t s) {
  const uint64_t tilesX = ((uint64_t)w + DR_TP_TILE_X - 1) / DR_TP_TILE_X, tilesY = ((uint64_t)h + DR_TP_TILE_Y - 1) / DR_TP_TILE_Y;
  const uint64_t ntiles = tilesX * tilesY;
  const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, DR_TP_MAX_GRID);
  hipLaunchKernelGGL(k_temporal, dim3(grid), dim3(DR_TP_TILE_X, DR_TP_TILE_Y), 0, s, im, w, h, prm, tilesX, ntiles);
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
  const int rc = tp_check_images(who, im, w, h, params);
  if (rc != DR_OK) return rc;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, std::string(who) + ": called before dr_init");
  return run(who, im, w, h, *params, (hipStream_t)hip_stream);
}

extern "C" int dr_temporal(const float* rgb, const float* normal, const float* depth, const float* h_rgb, const float* h_m2, const float* h_len,
                           const float* h_normal, const float* h_depth, int32_t w, int32_t h, const DrTemporalParams* params, float* out_rgb,
                           float* out_m2, float* out_len) {
  const char* who = "dr_temporal";
  const TpImages host = {rgb, normal, depth, h_rgb, h_m2, h_len, h_normal, h_depth, out_rgb, out_m2, out_len};
  const int rc = tp_check_images(who, host, w, h, params);
  if (rc != DR_OK) return rc;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, std::string(who) + ": called before dr_init");
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  const bool hist = h_rgb != nullptr;
  Buf<float> dRgb, dNormal, dDepth, dHRgb, dHM2, dHLen, dHNormal, dHDepth, dOutRgb, dOutM2, dOutLen;
  ST(dRgb.alloc(3 * n));
  ST(dNormal.alloc(3 * n));
  ST(dDepth.alloc(n));
  ST(dOutRgb.alloc(3 * n));
  ST(dOutM2.alloc(n));
  ST(dOutLen.alloc(n));
  hipStream_t s = 0;
  ST(hipMemcpyAsync(dRgb.p, rgb, 3 * n * f, hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dNormal.p, normal, 3 * n * f, hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dDepth.p, depth, n * f, hipMemcpyHostToDevice, s));
  if (hist) {
    ST(dHRgb.alloc(3 * n));
    ST(dHM2.alloc(n));
    ST(dHLen.alloc(n));
    ST(dHNormal.alloc(3 * n));
    ST(dHDepth.alloc(n));
    ST(hipMemcpyAsync(dHRgb.p, h_rgb, 3 * n * f, hipMemcpyHostToDevice, s));
    ST(hipMemcpyAsync(dHM2.p, h_m2, n * f, hipMemcpyHostToDevice, s));
    ST(hipMemcpyAsync(dHLen.p, h_len, n * f, hipMemcpyHostToDevice, s));
    ST(hipMemcpyAsync(dHNormal.p, h_normal, 3 * n * f, hipMemcpyHostToDevice, s));
    ST(hipMemcpyAsync(dHDepth.p, h_depth, n * f, hipMemcpyHostToDevice, s));
  }
  const TpImages im = {dRgb.p, dNormal.p, dDepth.p, dHRgb.p, dHM2.p, dHLen.p, dHNormal.p, dHDepth.p, dOutRgb.p, dOutM2.p, dOutLen.p};
  const int rc2 = run(who, im, w, h, *params, s);
  if (rc2 != DR_OK) return rc2;
  ST(hipMemcpyAsync(out_rgb, dOutRgb.p, 3 * n * f, hipMemcpyDeviceToHost, s));
  ST(hipMemcpyAsync(out_m2, dOutM2.p, n * f, hipMemcpyDeviceToHost, s));
  ST(hipMemcpyAsync(out_len, dOutLen.p, n * f, hipMemcpyDeviceToHost, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}
