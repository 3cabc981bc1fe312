// dr_upsample_device.hip -- the joint bilateral upsampler ON THE GPU: dr_upsample (host buffers) and dr_upsample_device
// (device buffers, asynchronous on a stream).
//   k_image_pack<DnInputs>   dr_image_device.h, lane = low-resolution pixel: the three low-resolution images become two planes of 16-byte
//                            texels, colour = (r, g, b, valid) and guide = (nx, ny, nz, z), so that a tap is two 16-byte loads
//   k_upsample               lane = full-resolution pixel, one launch: 64 x 4 tiles whose rows are contiguous in x -- a wave is 64 neighbours
//                            of one image row, which read 64 / factor + taps - 1 neighbouring texels of each of `taps` low-resolution rows.
//                            It reads the pixel's own guide straight from normal / depth (each is read once) and writes its 12 bytes of
//                            [h][w][3].
// The per-pixel rule is dr_upsample.h's, the one the host loop runs (dr_upsample_host.cpp): the outputs are byte-identical
// (tests/test_gpu_upsample.py).  Every tap's coordinates are checked against wl and hl before its loads (ups_pixel); the tile walk is
// dr_image_device.h's.  No LDS: the low-resolution planes are 1/4 or 1/16 of the frame, a tile's taps are lines its own lanes and the
// tiles beside it have just brought into L1 / L2, and the traffic that reaches HBM is the 16 B read and 12 B written per pixel plus 32 B
// per low-resolution pixel.
#include "dr_image_device.h"
#include "dr_upsample.h"

namespace {

__global__ void __launch_bounds__(DR_IMG_TILE_X* DR_IMG_TILE_Y) k_upsample(const DnTexel* colour, const DnTexel* guide, int32_t wl, int32_t hl,
                                                                          const float* normal, const float* depth, int32_t w, int32_t h,
                                                                          int32_t f, int32_t taps, float kn, float kz, uint64_t tilesX,
                                                                          uint64_t ntiles, float* out) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t x, y;
    if (!img_tile_pixel(t, tilesX, w, h, &x, &y)) continue;
    float c[3];
    ups_pixel(colour, guide, wl, hl, normal, depth, w, f, taps, kn, kz, (int32_t)x, (int32_t)y, c);
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    out[3 * p] = c[0];
    out[3 * p + 1] = c[1];
    out[3 * p + 2] = c[2];
  }
}

// the two low-resolution planes
uint64_t scratch_need(int32_t wl, int32_t hl) { return 2ull * sizeof(DnTexel) * (uint64_t)wl * (uint64_t)hl; }

// The launches of one call, on device buffers that the caller has checked
int run(const char* who, const DnInputs& lo, int32_t wl, int32_t hl, const float* normal, const float* depth, const DrUpsampleParams& prm,
        float* out, void* scratch, hipStream_t s) {
  const uint64_t nl = (uint64_t)wl * (uint64_t)hl;
  DnTexel* guide = (DnTexel*)scratch;
  DnTexel* colour = guide + nl;
  const int rc = img_pack(who, lo, nl, colour, guide, s);
  if (rc != DR_OK) return rc;
  const int32_t w = prm.factor * wl, h = prm.factor * hl;
  const ImgTiles tl = img_tiles(w, h);
  hipLaunchKernelGGL(k_upsample, dim3(tl.grid), dim3(DR_IMG_TILE_X, DR_IMG_TILE_Y), 0, s, (const DnTexel*)colour, (const DnTexel*)guide, wl, hl,
                     normal, depth, w, h, prm.factor, prm.taps, prm.k_normal, prm.k_depth, tl.tilesX, tl.ntiles, out);
  ST(hipGetLastError());
  return DR_OK;
}

}  // namespace

extern "C" int dr_upsample_device(const void* rgb_lo_dev, const void* normal_lo_dev, const void* depth_lo_dev, int32_t wl, int32_t hl,
                                  const void* normal_dev, const void* depth_dev, const DrUpsampleParams* params, void* out_dev, void* scratch_dev,
                                  uint64_t* scratch_bytes, void* hip_stream) {
  const char* who = "dr_upsample_device";
  if (!scratch_bytes || !params) return img_refuse(who, "a null pointer");
  int rc = scratch_dev ? ups_check_images(who, rgb_lo_dev, normal_lo_dev, depth_lo_dev, wl, hl, normal_dev, depth_dev, params, out_dev)
                       : img_refuse(who, ups_check(wl, hl, params));
  if (rc != DR_OK) return rc;
  const uint64_t need = scratch_need(wl, hl);
  if (img_scratch(who, scratch_dev, scratch_bytes, need, &rc)) return rc;
  const size_t n = (size_t)wl * (size_t)hl * (size_t)params->factor * (size_t)params->factor, f = sizeof(float);
  if (dn_overlap(out_dev, 3 * n * f, scratch_dev, (size_t)need)) return img_refuse(who, "out overlaps the scratch buffer");
  if ((rc = img_device_ready(who)) != DR_OK) return rc;
  return run(who, DnInputs{(const float*)rgb_lo_dev, (const float*)normal_lo_dev, (const float*)depth_lo_dev}, wl, hl, (const float*)normal_dev,
             (const float*)depth_dev, *params, (float*)out_dev, scratch_dev, (hipStream_t)hip_stream);
}

extern "C" int dr_upsample(const float* rgb_lo, const float* normal_lo, const float* depth_lo, int32_t wl, int32_t hl, const float* normal,
                           const float* depth, const DrUpsampleParams* params, float* out) {
  const char* who = "dr_upsample";
  int rc = ups_check_images(who, rgb_lo, normal_lo, depth_lo, wl, hl, normal, depth, params, out);
  if (rc != DR_OK || (rc = img_device_ready(who)) != DR_OK) return rc;
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
  ST(dRgbLo.upload(rgb_lo, 3 * nl, s));
  ST(dNormalLo.upload(normal_lo, 3 * nl, s));
  ST(dDepthLo.upload(depth_lo, nl, s));
  ST(dNormal.upload(normal, 3 * n, s));
  ST(dDepth.upload(depth, n, s));
  if ((rc = run(who, DnInputs{dRgbLo.p, dNormalLo.p, dDepthLo.p}, wl, hl, dNormal.p, dDepth.p, *params, dOut.p, scratch.p, s)) != DR_OK) return rc;
  ST(dOut.download(out, 3 * n, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}
