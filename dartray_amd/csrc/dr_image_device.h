// dr_image_device.h -- what the device units of the image-space stages share ("what an image stage is made of"): the
// device buffer of a host-buffer entry and the ST macro, the 64 x 4 tile walk of the lane-per-pixel kernels, the pack kernel, and the
// scratch and dr_init checks of a *_device entry.  For .hip units only; the host + device rules are dr_image.h's.
#ifndef DR_IMAGE_DEVICE_H
#define DR_IMAGE_DEVICE_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "dr_image.h"

// A device allocation that lives as long as one host-buffer entry, and its copies on the entry's stream
template <class T>
struct Buf {
  T* p = nullptr;
  hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
  hipError_t upload(const T* from, size_t n, hipStream_t s) { return hipMemcpyAsync(p, from, n * sizeof(T), hipMemcpyHostToDevice, s); }
  hipError_t download(T* to, size_t n, hipStream_t s) const { return hipMemcpyAsync(to, p, n * sizeof(T), hipMemcpyDeviceToHost, s); }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};
// a HIP call of the entry point `who`: its failure is the entry's
#define ST(x)                                                                                          \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess) return dr_fail(DR_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e_)); \
  } while (0)

// The tile walk: 64 x 4 tiles whose rows are contiguous in x, so a wave is 64 neighbours of one image row.  A workgroup of 64 x 4 lanes
// walks the tiles t = blockIdx.x, + gridDim.x, ... < ntiles, so that no image shape needs more workgroups than a launch may have.
#define DR_IMG_TILE_X 64  // one wave = one row of the tile
#define DR_IMG_TILE_Y 4
#define DR_IMG_MAX_GRID (1u << 20)

struct ImgTiles {
  uint64_t tilesX, ntiles;
  unsigned grid;
};
inline ImgTiles img_tiles(int32_t w, int32_t h) {
  const uint64_t tilesX = ((uint64_t)w + DR_IMG_TILE_X - 1) / DR_IMG_TILE_X, tilesY = ((uint64_t)h + DR_IMG_TILE_Y - 1) / DR_IMG_TILE_Y;
  return ImgTiles{tilesX, tilesX * tilesY, (unsigned)std::min<uint64_t>(tilesX * tilesY, DR_IMG_MAX_GRID)};
}
// This lane's pixel of tile t; false: it lies outside the image, and the lane skips the tile before any access
__device__ inline bool img_tile_pixel(uint64_t t, uint64_t tilesX, int32_t w, int32_t h, uint64_t* x, uint64_t* y) {
  *x = (t % tilesX) * DR_IMG_TILE_X + threadIdx.x;
  *y = (t / tilesX) * DR_IMG_TILE_Y + threadIdx.y;
  return *x < (uint64_t)w && *y < (uint64_t)h;
}

namespace {  // a kernel belongs to the unit that launches it

// lane = pixel: the images of `in` (DnInputs, DnpInputs) become two planes of 16-byte texels, so that a tap is two 16-byte loads
template <class Inputs>
__global__ void __launch_bounds__(256) k_image_pack(Inputs in, uint64_t n, DnTexel* colour, DnTexel* guide) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256u) {
    colour[p] = in.colour((size_t)p);
    guide[p] = in.guide((size_t)p);
  }
}

template <class Inputs>
int img_pack(const char* who, const Inputs& in, uint64_t n, DnTexel* colour, DnTexel* guide, hipStream_t s) {
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255u) / 256u, DR_IMG_MAX_GRID);
  hipLaunchKernelGGL(k_image_pack<Inputs>, dim3(grid), dim3(256), 0, s, in, n, colour, guide);
  ST(hipGetLastError());
  return DR_OK;
}

}  // namespace

// The scratch protocol of a *_device entry whose other arguments have passed the stage's check.  A NULL scratch_dev asks for the size:
// *scratch_bytes becomes `need`.  A buffer must hold `need` bytes and start at a 16-byte boundary.  true: the entry returns *rc.
inline bool img_scratch(const char* who, const void* scratch_dev, uint64_t* scratch_bytes, uint64_t need, int* rc) {
  *rc = DR_OK;
  if (!scratch_dev) {
    *scratch_bytes = need;
    return true;
  }
  if (*scratch_bytes < need) *rc = img_refuse(who, "the scratch buffer is too small");
  else if ((uintptr_t)scratch_dev % 16u != 0) *rc = img_refuse(who, "the scratch buffer is not 16-byte aligned");
  return *rc != DR_OK;
}

// The last check of every entry that launches: DR_OK, or the refusal of a process that has not called dr_init
inline int img_device_ready(const char* who) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, std::string(who) + ": called before dr_init");
  return DR_OK;
}

#endif
