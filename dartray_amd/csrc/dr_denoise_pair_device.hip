// dr_denoise_pair_device.hip -- the variance-guided a-trous filter ON THE GPU: dr_denoise_pair (host buffers) and
// dr_denoise_pair_device (device buffers, asynchronous on a stream).
//   k_denoise_pair_pack    lane = pixel: the two half renders and the two guides become two planes of 16-byte texels, colour =
//                          (mean r, g, b, variance or -1) and guide = (nx, ny, nz, z), so that a tap is two 16-byte loads
//   k_denoise_pair_level   lane = pixel, one launch per level, with the geometry of k_denoise_atrous (dr_denoise_device.hip): 64 x 4
//                          tiles whose rows are contiguous in x -- a wave is 64 neighbours of one image row, and its tap at dx * s is
//                          the same 1 KiB run shifted, so every tap load stays coalesced at every step; the nine loads of the variance
//                          prefilter are the same run shifted by one pixel and one row.  The levels take turns between two colour planes;
//                          the last one writes [h][w][3] and, when asked, [h][w].
// The per-pixel rule is dr_denoise_pair.h's, the one the host loop runs (dr_denoise_pair_host.cpp): the outputs are byte-identical
// (tests/test_gpu_denoise_pair.py).  Every tap's coordinates are checked against w and h before its loads (dnp_pixel); a workgroup walks
// the tiles t = blockIdx.x, + gridDim.x, ... and a lane whose pixel lies outside the image skips the tile before any access.  No LDS,
// for k_denoise_atrous's reason: the taps hit lines the neighbouring lanes and tiles have just brought into the caches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/dartray_hip.h"

#include "dr_denoise_pair.h"

namespace {

#define DR_DNP_TILE_X 64  // one wave = one row of the tile
#define DR_DNP_TILE_Y 4
#define DR_DNP_MAX_GRID (1u << 20)

__global__ void __launch_bounds__(256) k_denoise_pair_pack(const float* a, const float* b, const float* normal, const float* depth, uint64_t n,
                                                          DnTexel* colour, DnTexel* guide) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256u) {
    colour[p] = dnp_pack_colour(a, b, normal, depth, (size_t)p);
    guide[p] = dn_pack_guide(normal, depth, (size_t)p);
  }
}

// dst: the next level's colour plane; or out3: the image, with outv: the variance image or NULL (the last level)
__global__ void __launch_bounds__(DR_DNP_TILE_X* DR_DNP_TILE_Y) k_denoise_pair_level(const DnTexel* colour, const DnTexel* guide, int32_t w,
                                                                                    int32_t h, int32_t s, float kc, float kn, float kz,
                                                                                    float var_floor, uint64_t tilesX, uint64_t ntiles,
                                                                                    DnTexel* dst, float* out3, float* outv) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t x = (t % tilesX) * DR_DNP_TILE_X + threadIdx.x, y = (t / tilesX) * DR_DNP_TILE_Y + threadIdx.y;
    if (x >= (uint64_t)w || y >= (uint64_t)h) continue;
    const DnTexel r = dnp_pixel(colour, guide, w, h, (int32_t)x, (int32_t)y, s, kc, kn, kz, var_floor);
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    if (out3) {
      out3[3 * p] = r.x;
      out3[3 * p + 1] = r.y;
      out3[3 * p + 2] = r.z;
      if (outv) outv[p] = r.w;
    } else {
      dst[p] = r;
    }
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
#define ST(x)                                                                                          \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess) return dr_fail(DR_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e_)); \
  } while (0)

uint64_t scratch_need(int32_t w, int32_t h) { return 3ull * sizeof(DnTexel) * (uint64_t)w * (uint64_t)h; }

// The launches of one call, on device buffers that the caller has checked
int run(const char* who, const float* a, const float* b, const float* normal, const float* depth, int32_t w, int32_t h,
        const DrDenoisePairParams& prm, float* out, float* out_var, void* scratch, hipStream_t s) {
  const uint64_t n = (uint64_t)w * (uint64_t)h;
  DnTexel* guide = (DnTexel*)scratch;
  DnTexel* src = guide + n;
  DnTexel* dst = src + n;
  const unsigned packGrid = (unsigned)std::min<uint64_t>((n + 255u) / 256u, DR_DNP_MAX_GRID);
  hipLaunchKernelGGL(k_denoise_pair_pack, dim3(packGrid), dim3(256), 0, s, a, b, normal, depth, n, src, guide);
  ST(hipGetLastError());
  const uint64_t tilesX = ((uint64_t)w + DR_DNP_TILE_X - 1) / DR_DNP_TILE_X, tilesY = ((uint64_t)h + DR_DNP_TILE_Y - 1) / DR_DNP_TILE_Y;
  const uint64_t ntiles = tilesX * tilesY;
  const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, DR_DNP_MAX_GRID);
  for (int i = 0; i < prm.iterations; ++i) {
    const bool last = i == prm.iterations - 1;
    hipLaunchKernelGGL(k_denoise_pair_level, dim3(grid), dim3(DR_DNP_TILE_X, DR_DNP_TILE_Y), 0, s, (const DnTexel*)src, (const DnTexel*)guide, w,
                       h, (int32_t)(1 << i), prm.k_color, prm.k_normal, prm.k_depth, prm.var_floor, tilesX, ntiles,
                       last ? (DnTexel*)nullptr : dst, last ? out : (float*)nullptr, last ? out_var : (float*)nullptr);
    ST(hipGetLastError());
    std::swap(src, dst);
  }
  return DR_OK;
}

}  // namespace

extern "C" int dr_denoise_pair_device(const void* a_dev, const void* b_dev, const void* normal_dev, const void* depth_dev, int32_t w, int32_t h,
                                      const DrDenoisePairParams* params, void* out_dev, void* out_var_dev, void* scratch_dev,
                                      uint64_t* scratch_bytes, void* hip_stream) {
  const char* who = "dr_denoise_pair_device";
  const std::string pre = std::string(who) + ": ";
  if (!scratch_bytes || !params) return dr_fail(DR_ERR_INVALID, pre + "a null pointer");
  if (!scratch_dev) {  // the size query
    if (const char* why = dnp_check(w, h, params)) return dr_fail(DR_ERR_INVALID, pre + why);
    *scratch_bytes = scratch_need(w, h);
    return DR_OK;
  }
  const int rc = dnp_check_images(who, a_dev, b_dev, normal_dev, depth_dev, w, h, params, out_dev, out_var_dev);
  if (rc != DR_OK) return rc;
  const uint64_t need = scratch_need(w, h);
  if (*scratch_bytes < need) return dr_fail(DR_ERR_INVALID, pre + "the scratch buffer is too small");
  if ((uintptr_t)scratch_dev % sizeof(DnTexel) != 0) return dr_fail(DR_ERR_INVALID, pre + "the scratch buffer is not 16-byte aligned");
  const size_t n = (size_t)w * (size_t)h, f = sizeof(float);
  if (dn_overlap(out_dev, 3 * n * f, scratch_dev, (size_t)need)) return dr_fail(DR_ERR_INVALID, pre + "out overlaps the scratch buffer");
  if (out_var_dev && dn_overlap(out_var_dev, n * f, scratch_dev, (size_t)need))
    return dr_fail(DR_ERR_INVALID, pre + "out_var overlaps the scratch buffer");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, pre + "called before dr_init");
  return run(who, (const float*)a_dev, (const float*)b_dev, (const float*)normal_dev, (const float*)depth_dev, w, h, *params, (float*)out_dev,
             (float*)out_var_dev, scratch_dev, (hipStream_t)hip_stream);
}

extern "C" int dr_denoise_pair(const float* a, const float* b, const float* normal, const float* depth, int32_t w, int32_t h,
                               const DrDenoisePairParams* params, float* out, float* out_var) {
  const char* who = "dr_denoise_pair";
  const int rc = dnp_check_images(who, a, b, normal, depth, w, h, params, out, out_var);
  if (rc != DR_OK) return rc;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, std::string(who) + ": called before dr_init");
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
  ST(hipMemcpyAsync(dA.p, a, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dB.p, b, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dNormal.p, normal, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(dDepth.p, depth, n * sizeof(float), hipMemcpyHostToDevice, s));
  const int rc2 = run(who, dA.p, dB.p, dNormal.p, dDepth.p, w, h, *params, dOut.p, dVar.p, scratch.p, s);
  if (rc2 != DR_OK) return rc2;
  ST(hipMemcpyAsync(out, dOut.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (out_var) ST(hipMemcpyAsync(out_var, dVar.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}
