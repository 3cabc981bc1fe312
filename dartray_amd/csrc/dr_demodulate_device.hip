// dr_demodulate_device.hip -- demodulation ON THE GPU: dr_demodulate / dr_remodulate (host buffers) and
// dr_demodulate_device / dr_remodulate_device (device buffers, asynchronous on a stream).
//   k_demodulate, k_remodulate   lane = pixel, one launch each, grid-stride over the w * h pixels in raster order (k_image_pack's walk: a
//                                pixel reads no neighbour, so there is no tile and no LDS).  A wave reads 64 pixels = 768 contiguous bytes
//                                of each image that is present and writes 768 contiguous bytes: every byte of every 128-byte line it
//                                touches is used, once.  An absent image (NULL) is a uniform branch and costs no load.
// The per-pixel rules are dr_demodulate.h's, the ones the host loops run (dr_demodulate_host.cpp): the outputs are byte-identical
// (tests/test_gpu_demodulate.py).  No scratch buffer, no pack pass: the images travel as kernel arguments, as in dr_firefly_device.hip.
#include "dr_demodulate.h"
#include "dr_image_device.h"

namespace dr_host {
extern int g_device;  // dr_api.hip: dr_init's device, -1 before it
}

namespace {

// (dr_firefly_device.hip's: a process with a visible GPU that never called dr_init is refused too)
int ready(const char* who) {
  if (dr_host::g_device < 0) return dr_fail(DR_ERR_NO_DEVICE, std::string(who) + ": called before dr_init");
  return img_device_ready(who);
}

__global__ void __launch_bounds__(256) k_demodulate(DemodImages im, float eps, uint64_t n) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256u) demod_pixel(im, eps, (size_t)p);
}

__global__ void __launch_bounds__(256) k_remodulate(DemodImages im, float eps, uint64_t n) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256u) remod_pixel(im, eps, (size_t)p);
}

// The launch of one call, on device buffers that the caller has checked
int run(const char* who, bool re, const DemodImages& im, int32_t w, int32_t h, const DrDemodulateParams& prm, hipStream_t s) {
  const uint64_t n = (uint64_t)w * (uint64_t)h;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255u) / 256u, DR_IMG_MAX_GRID);
  if (re) hipLaunchKernelGGL(k_remodulate, dim3(grid), dim3(256), 0, s, im, prm.eps, n);
  else hipLaunchKernelGGL(k_demodulate, dim3(grid), dim3(256), 0, s, im, prm.eps, n);
  ST(hipGetLastError());
  return DR_OK;
}

int on_device(const char* who, bool re, const void* rgb_dev, const void* emission_dev, const void* albedo_dev, int32_t w, int32_t h,
              const DrDemodulateParams* params, void* out_dev, void* hip_stream) {
  const DemodImages im = {(const float*)rgb_dev, (const float*)emission_dev, (const float*)albedo_dev, (float*)out_dev};
  int rc = demod_check_images(who, im, w, h, params);
  if (rc != DR_OK || (rc = ready(who)) != DR_OK) return rc;
  return run(who, re, im, w, h, *params, (hipStream_t)hip_stream);
}

int on_host_buffers(const char* who, bool re, const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h,
                    const DrDemodulateParams* params, float* out) {
  const DemodImages host = {rgb, emission, albedo, out};
  int rc = demod_check_images(who, host, w, h, params);
  if (rc != DR_OK || (rc = ready(who)) != DR_OK) return rc;
  const size_t n = 3 * (size_t)w * (size_t)h;
  Buf<float> dRgb, dEmission, dAlbedo, dOut;
  ST(dRgb.alloc(n));
  if (emission) ST(dEmission.alloc(n));
  if (albedo) ST(dAlbedo.alloc(n));
  ST(dOut.alloc(n));
  hipStream_t s = 0;
  ST(dRgb.upload(rgb, n, s));
  if (emission) ST(dEmission.upload(emission, n, s));
  if (albedo) ST(dAlbedo.upload(albedo, n, s));
  const DemodImages im = {dRgb.p, dEmission.p, dAlbedo.p, dOut.p};
  if ((rc = run(who, re, im, w, h, *params, s)) != DR_OK) return rc;
  ST(dOut.download(out, n, s));
  ST(hipStreamSynchronize(s));
  return DR_OK;
}

}  // namespace

extern "C" int dr_demodulate_device(const void* rgb_dev, const void* emission_dev, const void* albedo_dev, int32_t w, int32_t h,
                                    const DrDemodulateParams* params, void* out_dev, void* hip_stream) {
  return on_device("dr_demodulate_device", false, rgb_dev, emission_dev, albedo_dev, w, h, params, out_dev, hip_stream);
}

extern "C" int dr_remodulate_device(const void* rgb_dev, const void* emission_dev, const void* albedo_dev, int32_t w, int32_t h,
                                    const DrDemodulateParams* params, void* out_dev, void* hip_stream) {
  return on_device("dr_remodulate_device", true, rgb_dev, emission_dev, albedo_dev, w, h, params, out_dev, hip_stream);
}

extern "C" int dr_demodulate(const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h, const DrDemodulateParams* params,
                             float* out) {
  return on_host_buffers("dr_demodulate", false, rgb, emission, albedo, w, h, params, out);
}

extern "C" int dr_remodulate(const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h, const DrDemodulateParams* params,
                             float* out) {
  return on_host_buffers("dr_remodulate", true, rgb, emission, albedo, w, h, params, out);
}
