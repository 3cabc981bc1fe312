// dr_upsample_device.hip -- the joint bilateral upsampler ON THE GPU: dr_upsample (host buffers) and dr_upsample_device
// (device buffers, asynchronous on a stream).
//   k_upsample_pack   lane = low-resolution pixel: the three low-resolution images become two planes of 16-byte texels, colour =
//                     (r, g, b, valid) and guide = (nx, ny, nz, z), so that a tap is two 16-byte loads
//   k_upsample        lane = full-resolution pixel, one launch: 64 x 4 tiles whose rows are contiguous in x -- a wave is 64 neighbours of one
//                     image row, which read 64 / factor + taps - 1 neighbouring texels of each of `taps` low-resolution rows.  It reads the
//                     pixel's own guide straight from normal / depth (each is read once) and writes its 12 bytes of [h][w][3].
// The per-pixel rule is dr_upsample.h's, the one the host loop runs (dr_upsample_host.cpp): the outputs are byte-identical
// (tests/test_gpu_upsample.py).  Every tap's coordinates are checked against wl and hl before its loads (ups_pixel); a workgroup walks the
// tiles t = blockIdx.x, + gridDim.x, ... so that no image shape needs more workgroups than a launch may have, and a lane whose pixel lies
// outside the image skips the tile before any access.  No LDS: the low-resolution planes are 1/4 or 1/16 of the frame, a tile's taps are
// lines its own lanes and the tiles beside it have just brought into L1 / L2, and the traffic that reaches HBM is the 16 B read and 12 B
// written per pixel plus 32 B per low-resolution pixel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/dartray_hip.h"

#include "dr_upsample.h"

namespace {

#define DR_UPS_TILE_X 64  // one wave = one row of the tile
#define DR_UPS_TILE_Y 4
#define DR_UPS_MAX_GRID (1u << 20)

__global__ void __launch_bounds__(256) k_upsample_pack(const float* rgb_lo, const float* normal_lo, const float* depth_lo, uint64_t nl,
                                                      DnTexel* colour, DnTexel* guide) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nl; q += (uint64_t)gridDim.x * 256u) {
    colour[q] = dn_pack_colour(rgb_lo, normal_lo, depth_lo, (size_t)q);
    guide[q] = dn_pack_guide(normal_lo, depth_lo, (size_t)q);
  }
}

__global__ void __launch_bounds__(DR_UPS_TILE_X* DR_UPS_TILE_Y) k_upsample(const DnTexel* colour, const DnTexel* guide, int32_t wl, int32_t hl,
                                                                          const float* normal, const float* depth, int32_t w, int32_t h,
                                                                          int32_t f, int32_t taps, float kn, float kz, uint64_t tilesX,
                                                                          uint64_t ntiles, float* out) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t x = (t % tilesX) * DR_UPS_TILE_X + threadIdx.x, y = (t / tilesX) * DR_UPS_TILE_Y + threadIdx.y;
    if (x >= (uint64_t)w || y >= (uint64_t)h) continue;
    float c[3];
    ups_pixel(colour, guide, wl, hl, normal, depth, w, f, taps, kn, kz, (int32_t)x, (int32_t)y, c);
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    out[3 * p] = c[0];
    out[3 * p + 1] = c[1];
    out[3 * p + 2] = c[2];
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

uint64_t scratch_need(int32_t wl, int32_t hl) { return 2ull * sizeof(DnTexel) * (uint64_t)wl * (uint64_t)hl; }

// The launches of one call, on device buffers that the caller has checked
int run(const char* who, const float* rgb_lo, const float* normal_lo, const float* depth_lo, int32_t wl, int32_t hl, const float* normal,
        const float* depth, const DrUpsampleParams& prm, float* out, void* scratch, hipStream_t s) {
  const uint64_t nl = (uint64_t)wl * (uint64_t)hl;
  DnTexel* guide = (DnTexel*)scratch;
  DnTexel* colour = guide + nl;
  const unsigned packGrid = (unsigned)std::min<uint64_t>((nl + 255u) / 256u, DR_UPS_MAX_GRID);
  hipLaunchKernelGGL(k_upsample_pack, dim3(packGrid), dim3(256), 0, s, rgb_lo, normal_lo, depth_lo, nl, colour, guide);
  ST(hipGetLastError());
  const int32_t w = prm.factor * wl, h = prm.factor * hl;
  const uint64_t tilesX = ((uint64_t)w + DR_UPS_TILE_X - 1) / DR_UPS_TILE_X, tilesY = ((uint64_t)h + DR_UPS_TILE_Y - 1) / DR_UPS_TILE_Y;
  const uint64_t ntiles = tilesX * tilesY;
  const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, DR_UPS_MAX_GRID);
  hipLaunchKernelGGL(k_upsample, dim3(grid), dim3(DR_UPS_TILE_X, DR_UPS_TILE_Y), 0, s, (const DnTexel*)colour, (const DnTexel*)guide, wl, hl, normal,
                     depth, w, h, prm.factor, prm.taps, prm.k_normal, prm.k_depth, tilesX, ntiles, out);
  ST(hipGetLastError());
  return DR_OK;
}

}  // namespace

extern "C" int dr_upsample_device(const void* rgb_lo_dev, const void* normal_lo_dev, const void* depth_lo_dev, int32_t wl, int32_t hl,
                                  const void* normal_dev, const void* depth_dev, const DrUpsampleParams* params, void* out_dev, void* scratch_dev,
                                  uint64_t* scratch_bytes, void* hip_stream) {
  const char* who = "dr_upsample_device";
  const std::string pre = std::string(who) + ": ";
  if (!scratch_bytes || !params) return dr_fail(DR_ERR_INVALID, pre + "a null pointer");
  if (!scratch_dev) {  // the size query
    if (const char* why = ups_check(wl, hl, params)) return dr_fail(DR_ERR_INVALID, pre + why);
    *scratch_bytes = scratch_need(wl, hl);
    return DR_OK;
  }
  const int rc = ups_check_images(who, rgb_lo_dev, normal_lo_dev, depth_lo_dev, wl, hl, normal_dev, depth_dev, params, out_dev);
  if (rc != DR_OK) return rc;
  const uint64_t need = scratch_need(wl, hl);
  if (*scratch_bytes < need) return dr_fail(DR_ERR_INVALID, pre + "the scratch buffer is too small");
  if ((uintptr_t)scratch_dev % sizeof(DnTexel) != 0) return dr_fail(DR_ERR_INVALID, pre + "the scratch buffer is not 16-byte aligned");
  const size_t n = (size_t)wl * (size_t)hl * (size_t)params->factor * (size_t)params->factor, f = sizeof(float);
  if (dn_overlap(out_dev, 3 * n * f, scratch_dev, (size_t)need)) return dr_fail(DR_ERR_INVALID, pre + "out overlaps the scratch buffer");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, pre + "called before dr_init");
  return run(who, (const float*)rgb_lo_dev, (const float*)normal_lo_dev, (const float*)depth_lo_dev, wl, hl, (const float*)normal_dev,
             (const float*)depth_dev, *params, (float*)out_dev, scratch_dev, (hipStream_t)hip_stream);
}

extern "C" int dr_upsample(const float* rgb_lo, const float* normal_lo, const float* depth_lo, int32_t wl, int32_t hl, const float* normal,
                           const float* depth, const DrUpsampleParams* params, float* out) {
  const char* who = "dr_upsample";
  const int rc = ups_check_images(who, rgb_lo, normal_lo, depth_lo, wl, hl, normal, depth, params, out);
  if (rc != DR_OK) return rc;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, std::string(who) + ": called before dr_init");
  const size_t nl = (size_t)wl * (size_t)hl, n = nl * (size_t)params->factor * (size_t)params->factor;
  Buf<float> dRgbLo, dNormalLo, dDepthLo, dNormal, dDepth, dOut;
  Buf<DnTexel> scratch;
  ST(dRgbLo.alloc(3 * nl));
  ST(dNormalLo.alloc(3 * nl));
  ST(dDepthLo.alloc(nl));
  ST(dNormal.alloc(3 * n));
  ST(dDepth.alloc(n));
  ST(dOut.alloc(3 * n));
  ST(scratch.alloc(2 * nl));
  hipStream_t s = 0;
  ST(hipMemcpyAsync(dRgbLo.p, rgb_lo, 3 * nl * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dNormalLo.p, normal_lo, 3 * nl * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dDepthLo.p, depth_lo, nl * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dNormal.p, normal, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dDepth.p, depth, n * sizeof(float), hipMemcpyHostToDevice, s));
  const int rc2 = run(who, dRgbLo.p, dNormalLo.p, dDepthLo.p, wl, hl, dNormal.p, dDepth.p, *params, dOut.p, scratch.p, s);
  if (rc2 != DR_OK) return rc2;
  ST(hipMemcpyAsync(out, dOut.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}
