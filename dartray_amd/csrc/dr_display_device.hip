// dr_display_device.hip -- the display transform ON THE GPU: dr_display and dr_display_exposure (host buffers) and
// dr_display_device (device buffers, asynchronous on a stream, no wait on the host between the histogram and the encode).
//   k_display_hist     lane = pixel, grid-stride.  A workgroup keeps the 2048 bins in LDS (8 KiB) and adds to them with LDS atomics; before
//                      that each wave takes the bin of its first counted lane, finds the lanes that share it with one ballot and adds their
//                      number with ONE atomic (an image of one luminance is one atomic per wave instead of 64 on one address); the other
//                      lanes add 1 each.  At the end the workgroup adds its non-zero bins to the global counts with integer atomics: the
//                      counts do not depend on any order.
//   k_display_pick     one workgroup of 256 lanes, eight bins each: an inclusive scan of the 256 partial sums in LDS, and the one lane whose
//                      run crosses the rank walks its eight bins and writes the scale
//   k_display_encode   lane = pixel, grid-stride: 12 bytes in, 4 out.  The 256-word encode table arrives by value in the kernel's arguments
//                      and is copied to LDS, because the search index diverges across lanes; the scale is read from device memory (auto) or
//                      is an argument (manual exposure, where the two kernels above do not run)
// The per-pixel rules are dr_display.h's, the ones the host loop runs (dr_display_host.cpp): the outputs are byte-identical
// (tests/test_gpu_display.py).  Every pixel index is checked against n before its loads.
#include "dr_display.h"
#include "dr_image_device.h"

#ifndef DR_DISPLAY_HIST_COMBINE
#define DR_DISPLAY_HIST_COMBINE 1  // 0: every lane its own LDS atomic (tools/measure_display.py builds that variant beside this one)
#endif

namespace {

#define DR_DSP_BLOCK 256
#define DR_DSP_HIST_GRID 1024u    // 256 CUs x 4: fewer workgroups, fewer merges into the global counts
#define DR_DSP_ENCODE_GRID 2048u  // 256 CUs x 8
#define DR_DSP_SCRATCH ((uint64_t)DR_DISPLAY_BINS * sizeof(uint32_t) + 16u)  // the counts, then the scale in a 16-byte slot

__global__ void __launch_bounds__(DR_DSP_BLOCK) k_display_hist(const float* rgb, uint64_t n, uint32_t* hist) {
  __shared__ uint32_t bins[DR_DISPLAY_BINS];
  for (uint32_t i = threadIdx.x; i < DR_DISPLAY_BINS; i += DR_DSP_BLOCK) bins[i] = 0u;
  __syncthreads();
  // every lane of a wave makes the same number of rounds (the ballots need them all); a lane past the end counts nothing
  for (uint64_t base = (uint64_t)blockIdx.x * DR_DSP_BLOCK; base < n; base += (uint64_t)gridDim.x * DR_DSP_BLOCK) {
    const uint64_t p = base + threadIdx.x;
    uint32_t b = DR_DISPLAY_BINS;
    if (p < n) b = dsp_bin(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
#if DR_DISPLAY_HIST_COMBINE
    const uint64_t counted = __ballot(b < DR_DISPLAY_BINS);
    if (counted != 0) {  // the same in every lane of the wave
      const int leader = __ffsll((unsigned long long)counted) - 1;
      const uint32_t lb = (uint32_t)__shfl((int)b, leader);
      const uint64_t same = __ballot(b == lb);
      if ((int)(threadIdx.x & 63u) == leader) atomicAdd(&bins[lb], (uint32_t)__popcll((unsigned long long)same));
      if (b == lb) b = DR_DISPLAY_BINS;
    }
#endif
    if (b < DR_DISPLAY_BINS) atomicAdd(&bins[b], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < DR_DISPLAY_BINS; i += DR_DSP_BLOCK) {
    const uint32_t c = bins[i];
    if (c != 0u) atomicAdd(&hist[i], c);
  }
}

__global__ void __launch_bounds__(DR_DSP_BLOCK) k_display_pick(const uint32_t* hist, uint32_t permille, float key, float* scale) {
  __shared__ uint32_t run[DR_DSP_BLOCK];  // n < 2^31: no sum leaves 32 bits
  const uint32_t t = threadIdx.x, per = DR_DISPLAY_BINS / DR_DSP_BLOCK;
  uint32_t mine[DR_DISPLAY_BINS / DR_DSP_BLOCK], sum = 0u;
  for (uint32_t i = 0; i < per; ++i) {
    mine[i] = hist[t * per + i];
    sum += mine[i];
  }
  run[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < DR_DSP_BLOCK; d <<= 1) {
    const uint32_t add = t >= d ? run[t - d] : 0u;
    __syncthreads();
    run[t] += add;
    __syncthreads();
  }
  const uint32_t n = run[DR_DSP_BLOCK - 1];
  if (n == 0u) {
    if (t == 0) *scale = 1.0f;
    return;
  }
  const uint64_t rank = dsp_rank(n, permille);
  uint64_t upto = run[t] - sum;  // the counts before this lane's bins
  if (upto <= rank && rank < (uint64_t)run[t]) {  // one lane: the runs are non-decreasing and end at n > rank
    for (uint32_t i = 0; i < per; ++i) {
      upto += mine[i];
      if (upto > rank) {
        *scale = dsp_scale_of_bin(t * per + i, key);
        break;
      }
    }
  }
}

__global__ void __launch_bounds__(DR_DSP_BLOCK) k_display_encode(const float* rgb, uint64_t n, DrDisplayParams prm, DspTable table,
                                                                 const float* scale_dev, float scale_arg, uint32_t* out) {
  __shared__ uint32_t lut[DR_DISPLAY_TABLE];
  static_assert(DR_DISPLAY_TABLE == DR_DSP_BLOCK, "one word per lane");
  lut[threadIdx.x] = table.w[threadIdx.x];
  __syncthreads();
  const float scale = scale_dev ? *scale_dev : scale_arg;
  for (uint64_t p = (uint64_t)blockIdx.x * DR_DSP_BLOCK + threadIdx.x; p < n; p += (uint64_t)gridDim.x * DR_DSP_BLOCK)
    out[p] = dsp_pixel(lut, prm, scale, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
}

unsigned grid_for(uint64_t n, unsigned cap) { return (unsigned)std::min<uint64_t>((n + DR_DSP_BLOCK - 1) / DR_DSP_BLOCK, cap); }

// The counts and the scale of auto-exposure into the scratch buffer: a memset and two launches
int run_exposure(const char* who, const float* rgb, uint64_t n, const DrDisplayParams& prm, void* scratch, hipStream_t s) {
  uint32_t* hist = (uint32_t*)scratch;
  float* scale = (float*)(hist + DR_DISPLAY_BINS);
  ST(hipMemsetAsync(hist, 0, DR_DISPLAY_BINS * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_display_hist, dim3(grid_for(n, DR_DSP_HIST_GRID)), dim3(DR_DSP_BLOCK), 0, s, rgb, n, hist);
  ST(hipGetLastError());
  hipLaunchKernelGGL(k_display_pick, dim3(1), dim3(DR_DSP_BLOCK), 0, s, (const uint32_t*)hist, prm.permille, prm.key, scale);
  ST(hipGetLastError());
  return DR_OK;
}

// The launches of one call, on device buffers that the caller has checked
int run(const char* who, const float* rgb, int32_t w, int32_t h, const DrDisplayParams& prm, void* out, void* scratch, hipStream_t s) {
  const uint64_t n = (uint64_t)w * (uint64_t)h;
  const float* scale_dev = nullptr;
  if (prm.auto_exposure) {
    const int rc = run_exposure(who, rgb, n, prm, scratch, s);
    if (rc != DR_OK) return rc;
    scale_dev = (const float*)((const uint32_t*)scratch + DR_DISPLAY_BINS);
  }
  hipLaunchKernelGGL(k_display_encode, dim3(grid_for(n, DR_DSP_ENCODE_GRID)), dim3(DR_DSP_BLOCK), 0, s, rgb, n, prm, dsp_table(prm.encode),
                     scale_dev, prm.exposure, (uint32_t*)out);
  ST(hipGetLastError());
  return DR_OK;
}

}  // namespace

extern "C" int dr_display_device(const void* rgb_dev, int32_t w, int32_t h, const DrDisplayParams* params, void* out_dev, void* scratch_dev,
                                 uint64_t* scratch_bytes, void* hip_stream) {
  const char* who = "dr_display_device";
  if (!scratch_bytes || !params) return img_refuse(who, "a null pointer");
  int rc = scratch_dev ? dsp_check_images(who, rgb_dev, w, h, params, out_dev, true) : img_refuse(who, dsp_check(params, w, h));
  if (rc != DR_OK) return rc;
  if (img_scratch(who, scratch_dev, scratch_bytes, DR_DSP_SCRATCH, &rc)) return rc;
  if ((uintptr_t)out_dev % 4u != 0) return img_refuse(who, "out is not 4-byte aligned");
  const size_t n = (size_t)w * (size_t)h;
  if (dn_overlap(out_dev, 4 * n, scratch_dev, (size_t)DR_DSP_SCRATCH)) return img_refuse(who, "out overlaps the scratch buffer");
  if (dn_overlap(rgb_dev, 3 * n * sizeof(float), scratch_dev, (size_t)DR_DSP_SCRATCH)) return img_refuse(who, "rgb overlaps the scratch buffer");
  if ((rc = img_device_ready(who)) != DR_OK) return rc;
  return run(who, (const float*)rgb_dev, w, h, *params, out_dev, scratch_dev, (hipStream_t)hip_stream);
}

extern "C" int dr_display(const float* rgb, int32_t w, int32_t h, const DrDisplayParams* params, uint8_t* out) {
  const char* who = "dr_display";
  int rc = dsp_check_images(who, rgb, w, h, params, out, true);
  if (rc != DR_OK || (rc = img_device_ready(who)) != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  Buf<float> dRgb;
  Buf<uint32_t> dOut, scratch;
  ST(dRgb.alloc(3 * n));
  ST(dOut.alloc(n));
  ST(scratch.alloc((size_t)DR_DSP_SCRATCH / sizeof(uint32_t)));
  hipStream_t s = 0;
  ST(dRgb.upload(rgb, 3 * n, s));
  if ((rc = run(who, dRgb.p, w, h, *params, dOut.p, scratch.p, s)) != DR_OK) return rc;
  ST(dOut.download((uint32_t*)out, n, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}

extern "C" int dr_display_exposure(const float* rgb, int32_t w, int32_t h, const DrDisplayParams* params, float* scale, uint32_t* hist) {
  const char* who = "dr_display_exposure";
  int rc = dsp_check_images(who, rgb, w, h, params, nullptr, false);
  if (rc != DR_OK) return rc;
  if (!scale) return img_refuse(who, "a null pointer");
  if ((rc = img_device_ready(who)) != DR_OK) return rc;
  const size_t n = (size_t)w * (size_t)h;
  Buf<float> dRgb;
  Buf<uint32_t> scratch;
  ST(dRgb.alloc(3 * n));
  ST(scratch.alloc((size_t)DR_DSP_SCRATCH / sizeof(uint32_t)));
  hipStream_t s = 0;
  ST(dRgb.upload(rgb, 3 * n, s));
  if ((rc = run_exposure(who, dRgb.p, n, *params, scratch.p, s)) != DR_OK) return rc;
  ST(hipMemcpyAsync(scale, scratch.p + DR_DISPLAY_BINS, sizeof(float), hipMemcpyDeviceToHost, s));
  if (hist) ST(scratch.download(hist, DR_DISPLAY_BINS, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}
