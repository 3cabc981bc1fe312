// dr_firefly_device.hip -- firefly suppression ON THE GPU: dr_firefly (host buffers) and dr_firefly_device (device
// buffers, asynchronous on a stream).
//   k_firefly<R>   lane = pixel, one launch: the 64 x 4 tile walk of dr_image_device.h, with the tile and its halo of R pixels staged in
//                  LDS once per workgroup.  The window is dense at step 1 -- (2 R + 1)^2 - 1 = 8 or 24 taps whose footprints overlap all
//                  but one column from lane to lane -- so a texel that 9 or 25 lanes read is loaded, tested and weighed (img_lum) once.
// The per-pixel rule is dr_firefly.h's, the one the host loop runs (dr_firefly_host.cpp), over another tap source: the outputs are
// byte-identical (tests/test_gpu_firefly.py).
//
// STAGING.  Every lane of the workgroup helps: texel i = lane, lane + 256, ... of the (64 + 2 R) x (4 + 2 R) tile is computed by
// fire_texel -- validity and luminance while it is loaded -- and written to five f32 planes (nx, ny, nz, z, lum: 20 bytes per texel).  An
// invalid texel's lum is a NaN, and a halo texel outside the image is staged the same way without any load, so the rule needs no bounds
// test of its own here.  The three images travel as kernel arguments; there is no pack pass and no scratch buffer.
//
// BARRIERS.  The other image kernels `continue` out of a tile when their pixel lies outside the image; with a barrier in the loop that
// would hang.  Here the loop bounds depend on blockIdx, gridDim and ntiles alone, so they are uniform per workgroup, and EVERY lane reaches
// both barriers of every iteration: the one after staging, and the one before the next tile is staged over this one.  Only the rule and its
// stores are skipped for a lane whose pixel lies outside the image; such a lane still stages its share of the tile.
//
// LDS LAYOUT.  Planes, not 20-byte records: a wave is one row of the tile, so a tap is 64 consecutive dwords of one plane row for any row
// stride (66 or 68 dwords), and the staging writes are 64 consecutive dwords too.  ds_read_b32 and ds_write_b32 are served in two 32-lane
// groups over (address / 4) mod 32 banks: 32 consecutive dwords are 32 distinct banks, so neither has a conflict and no padding is needed.
// (Records of five dwords would also be conflict-free, 5 being odd, but would make every tap five strided reads a lane.)
//
// OCCUPANCY.  The tile is 5 x 66 x 6 x 4 = 7920 bytes at R = 1 and 5 x 68 x 8 x 4 = 10880 bytes at R = 2: 20 and 15 workgroups of a CU's
// 160 KiB, more than the 8 workgroups of four waves that its 32 wave slots admit, so LDS never limits residency.  The top-rank list is four
// registers updated by an unrolled compare-and-swap chain (fire_insert): no private array indexed at run time, no scratch memory.
#include "dr_firefly.h"
#include "dr_image_device.h"

namespace dr_host {
extern int g_device;  // dr_api.hip: dr_init's device, -1 before it
}

namespace {

// The last check of both entries.  img_device_ready asks the HIP runtime for its current device, which a process with a visible GPU has
// without ever calling dr_init; this stage asks dr_init's own record first, so that such a process is refused too.
int ready(const char* who) {
  if (dr_host::g_device < 0) return dr_fail(DR_ERR_NO_DEVICE, std::string(who) + ": called before dr_init");
  return img_device_ready(who);
}

template <int R>
struct FireTile {
  static constexpr int W = DR_IMG_TILE_X + 2 * R, H = DR_IMG_TILE_Y + 2 * R, N = W * H;
};

// The device's tap source: the workgroup's tile, whose texel (0, 0) is image pixel (ox, oy).  Every tap of a pixel of the tile's core lies
// inside the tile, and one outside the image was staged as invalid.
template <int R>
struct FireTileSource {
  const float* tile;  // [5][N]
  int64_t ox, oy;
  DR_DN_HD bool tap(int64_t x, int64_t y, FireTap* t) const {
    constexpr int N = FireTile<R>::N;
    const int i = (int)(y - oy) * FireTile<R>::W + (int)(x - ox);
    t->lum = tile[4 * N + i];
    if (!dn_finite(t->lum)) return false;
    t->guide = DnTexel{tile[i], tile[N + i], tile[2 * N + i], tile[3 * N + i]};
    return true;
  }
};

template <int R>
__global__ void __launch_bounds__(DR_IMG_TILE_X* DR_IMG_TILE_Y) k_firefly(FireImages im, int32_t w, int32_t h, DrFireflyParams prm, uint64_t tilesX,
                                                                         uint64_t ntiles) {
  constexpr int W = FireTile<R>::W, N = FireTile<R>::N;
  __shared__ float tile[5 * N];
  const int lane = (int)(threadIdx.y * DR_IMG_TILE_X + threadIdx.x);
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // uniform per workgroup: see BARRIERS
    const int64_t ox = (int64_t)((t % tilesX) * DR_IMG_TILE_X) - R, oy = (int64_t)((t / tilesX) * DR_IMG_TILE_Y) - R;
    for (int i = lane; i < N; i += DR_IMG_TILE_X * DR_IMG_TILE_Y) {
      const int64_t gx = ox + i % W, gy = oy + i / W;
      FireTap q = {DnTexel{0.0f, 0.0f, 0.0f, 0.0f}, __builtin_nanf("")};
      if (gx >= 0 && gx < w && gy >= 0 && gy < h) (void)fire_texel(im.rgb, im.normal, im.depth, (size_t)gy * (size_t)w + (size_t)gx, &q);
      tile[i] = q.guide.x;
      tile[N + i] = q.guide.y;
      tile[2 * N + i] = q.guide.z;
      tile[3 * N + i] = q.guide.w;
      tile[4 * N + i] = q.lum;
    }
    __syncthreads();
    uint64_t x, y;
    if (img_tile_pixel(t, tilesX, w, h, &x, &y)) {
      const FireTileSource<R> src = {tile, ox, oy};
      fire_pixel<R>(src, im, w, prm, (int32_t)x, (int32_t)y);
    }
    __syncthreads();
  }
}

// The launch of one call, on device buffers that the caller has checked
int run(const char* who, const FireImages& im, int32_t w, int32_t h, const DrFireflyParams& prm, hipStream_t s) {
  const ImgTiles tl = img_tiles(w, h);
  const dim3 block(DR_IMG_TILE_X, DR_IMG_TILE_Y);
  if (prm.radius == 1) hipLaunchKernelGGL(k_firefly<1>, dim3(tl.grid), block, 0, s, im, w, h, prm, tl.tilesX, tl.ntiles);
  else hipLaunchKernelGGL(k_firefly<2>, dim3(tl.grid), block, 0, s, im, w, h, prm, tl.tilesX, tl.ntiles);
  ST(hipGetLastError());
  return DR_OK;
}

}  // namespace

extern "C" int dr_firefly_device(const void* rgb_dev, const void* normal_dev, const void* depth_dev, int32_t w, int32_t h,
                                 const DrFireflyParams* params, void* out_dev, void* removed_dev, void* hip_stream) {
  const char* who = "dr_firefly_device";
  const FireImages im = {(const float*)rgb_dev, (const float*)normal_dev, (const float*)depth_dev, (float*)out_dev, (float*)removed_dev};
  int rc = fire_check_images(who, im, w, h, params);
  if (rc != DR_OK || (rc = ready(who)) != DR_OK) return rc;
  return run(who, im, w, h, *params, (hipStream_t)hip_stream);
}

extern "C" int dr_firefly(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h, const DrFireflyParams* params,
                          float* out, float* removed) {
  const char* who = "dr_firefly";
  const FireImages host = {rgb, normal, depth, out, removed};
  int rc = fire_check_images(who, host, w, h, params);
  if (rc != DR_OK || (rc = ready(who)) != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  Buf<float> dRgb, dNormal, dDepth, dOut, dRemoved;
  ST(dRgb.alloc(3 * n));
  ST(dNormal.alloc(3 * n));
  ST(dDepth.alloc(n));
  ST(dOut.alloc(3 * n));
  if (removed) ST(dRemoved.alloc(n));
  hipStream_t s = 0;
  ST(dRgb.upload(rgb, 3 * n, s));
  ST(dNormal.upload(normal, 3 * n, s));
  ST(dDepth.upload(depth, n, s));
  const FireImages im = {dRgb.p, dNormal.p, dDepth.p, dOut.p, dRemoved.p};
  if ((rc = run(who, im, w, h, *params, s)) != DR_OK) return rc;
  ST(dOut.download(out, 3 * n, s));
  if (removed) ST(dRemoved.download(removed, n, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}
